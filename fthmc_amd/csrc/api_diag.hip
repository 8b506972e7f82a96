// extern "C" entry points of libfthmc_hip.so (include/fthmc_hip.h): the event timers and cycle-stamp profilers of single kernels.
// They open their calls as every entry point does (api_call.h), and they synchronize: measurement tools, never part of a captured sequence.
#include "api_call.h"
#include <stdlib.h>

namespace {

// Event timing of `reps` calls of launch() behind two untimed warm-up calls: *ms_avg = milliseconds per call.  The events are
// created here, after the caller's last early return, and destroyed on every path.
template <class Launch> int time_launches(int reps, hipStream_t s, double* ms_avg, Launch launch) {
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess) return FTHMC_ERR_LAUNCH;
    if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); return FTHMC_ERR_LAUNCH; }
    int rc = FTHMC_OK;
    for (int it = -2; it < reps && rc == FTHMC_OK; ++it) {
        if (it == 0) (void)hipEventRecord(e0, s);
        rc = launch();
    }
    (void)hipEventRecord(e1, s);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *ms_avg = (double)ms / reps;
    return rc;
}

// Cycle stamps of a profiled launch, read back and averaged: dbg = nrec records of nslot stamps on the device;
// out[k] = sum over the records of (stamp k - stamp ref(k)) / denom, where both were written (ref(k) < 0: stamp k itself), k >= k0
template <class Ref> int mean_stamps(const long long* dbg, size_t nrec, int nslot, int k0, size_t denom, hipStream_t s, double* out, Ref ref) {
    const size_t bytes = nrec * nslot * sizeof(long long);
    long long* h = (long long*)malloc(bytes);
    if (!h) return FTHMC_ERR_ARG;
    if (hipMemcpyAsync(h, dbg, bytes, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) { free(h); return FTHMC_ERR_LAUNCH; }
    for (int k = 0; k < nslot; ++k) out[k] = 0.0;
    for (size_t r = 0; r < nrec; ++r)
        for (int k = k0; k < nslot; ++k) {
            const int q = ref(k);
            const long long t = h[r * nslot + k], t0 = q < 0 ? 0 : h[r * nslot + q];
            if (t && (q < 0 || t0)) out[k] += (double)(t - t0) / denom;
        }
    free(h);
    return FTHMC_OK;
}

}  // namespace

extern "C" {

int fthmc_time_kernel(int kind, const double* x, const double* w, const fthmc_arch_t* arch, int B, int L, int mu, int off, int act,
                      double beta, int reps, double* ms_avg_host, void* ws, size_t ws_bytes, void* stream) {
    if (!x || !ms_avg_host || bad_shape(B, L) || reps < 1 || kind < 0 || kind > 3) return FTHMC_ERR_ARG;
    if (kind < 2 && !w) return FTHMC_ERR_ARG;
    Ctx C; WS W; FT_TRY(open_call(arch, stream, &C));
    if (C.gen() && kind < 2) return FTHMC_ERR_UNSUPPORTED;         // the tuned kernels serve the default net shape
    FT_TRY(open_ws(C, ws, ws_bytes, B, L, 1, false, &W));
    const hipStream_t s = C.s;
    FlowLayerArgs a{};
    if (kind < 2) {
        FT_TRY(use_weights(C, w, 1, W.wint));
        FT_TRY(launch_wilson_gp(x, B, L, beta, W.gp, s));
        a = FlowLayerArgs(W.wint, B, L, mu, off, act);
        a.x = x; a.y = W.X; a.logj_part = W.lj_part;
        a.up_gp = W.gp; a.glogj_const = -1.0; a.gp_part = W.gp_part; a.gp_out = W.gp2;
#ifdef FT_DIAG
        if (const char* e = getenv("FTHMC_DBG_STOP")) a.dbg_stop = atoi(e);
#endif
        if (C.mfma) {            // the hot path: forward stashes, backward reads the stash
            a.stash = W.stash;
            a.logj_part = nullptr;       // ... and asks for no log J: exactly what a layer of a force sweep launches (the SWEEP / FS instances)
            FT_TRY(launch_flow_fwd_mfma(a, s));
            // the forward as layers 1 .. nl - 1 of a sweep launch it: in place on the work buffer (sweep_forward)
            if (kind == 0 && flow_fwd_inplace_ok(L, act)) {
                if (hipMemcpyAsync(W.X, x, W.n2 * sizeof(double), hipMemcpyDeviceToDevice, s) != hipSuccess) return FTHMC_ERR_LAUNCH;
                a.x = W.X; a.inplace = 1;
            }
        }
    } else {
        int64_t* seeds = reinterpret_cast<int64_t*>(W.scal);             // B int64 seeds = 0 .. (any values do)
        if (hipMemsetAsync(seeds, 0, (size_t)B * sizeof(int64_t), s) != hipSuccess) return FTHMC_ERR_LAUNCH;
        FT_TRY(launch_random_momenta(seeds, B, 2 * L * L, W.va, nullptr, s));
    }
    return time_launches(reps, s, ms_avg_host, [&] {
        if (kind == 0) return flow_fwd(C, a, s);
        if (kind == 1) return a.stash ? launch_flow_bwd_gather(a, s) : launch_flow_bwd(a, false, s);
        if (kind == 2) return launch_leap_step(x, W.va, W.xa, W.vb, B, L, beta, 0.05, 0.1, s);
        return launch_hmc_trajectory_fused(x, W.va, W.scal + B, B, L, beta, 0.1, 10, W.xa, nullptr, nullptr, nullptr, nullptr, s);
    });
}

int fthmc_time_small(const double* x, const double* v, const double* u, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L, int act,
                     double beta, double dt, int nstep, int reps, double* ms_avg_host, void* ws, size_t ws_bytes, void* stream) {
    if (!x || !v || !u || !w || !ms_avg_host || bad_shape(B, L) || n_layers < 1 || nstep < 1 || reps < 1) return FTHMC_ERR_ARG;
    Ctx C; WS W; FT_TRY(open_call(arch, stream, &C));
    if (!C.small(L, n_layers)) return FTHMC_ERR_UNSUPPORTED;
    FT_TRY(open_ws(C, ws, ws_bytes, B, L, n_layers, false, &W));
    FT_TRY(use_weights(C, w, n_layers, W.wint));
    SmallArgs a = small_args(x, W, n_layers, B, act, beta, 3);
    a.v = v; a.u = u; a.dt = dt; a.nstep = nstep; a.x_out = W.xb;
    // H0 is evaluated in the launch (no state_in): nstep force sweeps + 2 action sweeps
    return time_launches(reps, C.s, ms_avg_host, [&] { return launch_ft_small(a, L, C.s); });
}

int fthmc_small_profile(const double* x, const double* v, const double* u, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L,
                        int act, double beta, double dt, int nstep, double* cycles_host32, void* ws, size_t ws_bytes,
                        void* stream) {
    if (!x || !v || !u || !w || !cycles_host32 || bad_shape(B, L) || n_layers < 1 || nstep < 1) return FTHMC_ERR_ARG;
    Ctx C; WS W; FT_TRY(open_call(arch, stream, &C));
    if (!C.small(L, n_layers)) return FTHMC_ERR_UNSUPPORTED;
    FT_TRY(open_ws(C, ws, ws_bytes, B, L, n_layers, false, &W));
    const hipStream_t s = C.s;
    long long* dbg = reinterpret_cast<long long*>(W.gw_part);            // unused by the force path; B * 32 stamps fit
    if (hipMemsetAsync(dbg, 0, (size_t)B * 32 * sizeof(long long), s) != hipSuccess) return FTHMC_ERR_LAUNCH;
    FT_TRY(use_weights(C, w, n_layers, W.wint));
    SmallArgs a = small_args(x, W, n_layers, B, act, beta, 3);
    a.v = v; a.u = u; a.dt = dt; a.nstep = nstep; a.x_out = W.xb; a.dbg = dbg;
    FT_TRY(launch_ft_small(a, L, s));
    return mean_stamps(dbg, (size_t)B, 32, 0, (size_t)B, s, cycles_host32, [](int) { return -1; });
}

int fthmc_profile_stages(int kind, const double* x, const double* w, const fthmc_arch_t* arch, int B, int L, int mu, int off, int act,
                         double beta, double* cycles_host16, void* ws, size_t ws_bytes, void* stream) {
    if (!x || !w || !cycles_host16 || bad_shape(B, L) || kind < 0 || kind > 3) return FTHMC_ERR_ARG;
    Ctx C; WS W; FT_TRY(open_call(arch, stream, &C));
    if (C.gen()) return FTHMC_ERR_UNSUPPORTED;                     // the tuned kernels serve the default net shape
    const bool train = kind >= 2;                                  // kind 2: the backward in training mode (also writes A.gz); 3: k_flow_wgrad behind it
    FT_TRY(open_ws(C, ws, ws_bytes, B, L, 1, train, &W));
    const hipStream_t s = C.s;
    const size_t nrec = (size_t)B * (kind >= 1 ? flow_gather_geom() : flow_fwd_geom(true)).ntiles(L);
    // stamp buffer: a workspace region the profiled launch does not write (B * ntiles * 16 stamps fit in either)
    long long* dbg = reinterpret_cast<long long*>(train ? W.gp_part : W.gw_part);
    if (hipMemsetAsync(dbg, 0, nrec * 16 * sizeof(long long), s) != hipSuccess) return FTHMC_ERR_LAUNCH;
    FT_TRY(use_weights(C, w, 1, W.wint));
    FT_TRY(launch_wilson_gp(x, B, L, beta, W.gp, s));
    FlowLayerArgs a(W.wint, B, L, mu, off, act);
    a.x = x; a.y = W.X; a.logj_part = train ? W.lj_part : nullptr;                       // kind 0, 1: the launch of a force sweep
    a.up_gp = W.gp; a.glogj_const = -1.0; a.gp_part = W.gp_part; a.gp_out = W.gp2; a.dbg = dbg;
    if (kind == 0) a.stash = W.stash;             // the forward as a force sweep launches it: with the activation stash, without log J
    if (kind == 0 && flow_fwd_inplace_ok(L, act)) {                // ... in place on the work buffer, as layers 1 .. nl - 1 are
        if (hipMemcpyAsync(W.X, x, W.n2 * sizeof(double), hipMemcpyDeviceToDevice, s) != hipSuccess) return FTHMC_ERR_LAUNCH;
        a.x = W.X; a.inplace = 1;
    }
    if (kind >= 1) {                              // stash backward needs the forward's stash first
        a.stash = W.stash; a.stash_h = train ? 1 : 0; a.gw_part = W.gw_part; a.gz = train ? W.gz : nullptr; a.dbg = nullptr;
        FT_TRY(launch_flow_fwd_mfma(a, s));
        a.dbg = kind == 3 ? nullptr : dbg;
    }
    FT_TRY(kind == 0 ? launch_flow_fwd_mfma(a, s) : launch_flow_bwd_gather(a, s));
    size_t nused = nrec;                                           // records the profiled launch stamps
    if (kind == 3) { a.dbg = dbg; a.tpw = flow_wgrad_tpw(B, L, 1); nused = (size_t)flow_wgrad_nparts(B, L, a.tpw); FT_TRY(launch_flow_wgrad(a, s)); }
    // forward 7..12 (-DFT_DIAG builds): inside conv1 / conv2; backward, slots 6..13: per-wave arrival at the first barrier
    return mean_stamps(dbg, nrec, 16, 1, nused, s, cycles_host16, [kind](int k) {
        return k == 15 ? 14 : kind == 3 ? k - 1 : (kind >= 1 && k >= 6) ? 0 : (kind == 0 && k == 7) ? 1 : (kind == 0 && k == 11) ? 2 : k - 1;
    });
}

}  // extern "C"
