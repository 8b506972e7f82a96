// extern "C" entry points of libfthmc_hip.so (include/fthmc_hip.h), first order, and the host-side kernel sequencing behind them.
// Every function only enqueues work on the caller's stream; scratch comes from the caller's workspace, so the whole sequence of a
// trajectory can be captured into a hipGraph by the caller.  How a call is opened: api_call.h; the second order and force
// training: api_second_order.hip; the timers and profilers: api_diag.hip.
#include "api_call.h"
#include "topo_int.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

namespace fthmc {
static thread_local char g_last_error[256] = "";
void note_hip_error(hipError_t e, const char* file, int line) {
    snprintf(g_last_error, sizeof(g_last_error), "%s (%s:%d)", hipGetErrorString(e), file, line);
}
}  // namespace fthmc

namespace {

// one layer on the plain kernels for the fields and stripe of `a`, the first stash region its scratch; l: its place in the caller's weights
GenLayerArgs gen_one_layer(const Ctx& C, const WS& W, int l, const FlowLayerArgs& a) {
    GenLayerArgs g = gen_args(C, gen_ws(C, W, a.B, a.L), l, a.B, a.L, a.act, false);
    g.mu = a.mu; g.off = a.off; g.x = a.pin ? nullptr : a.x; g.pin = a.pin; g.y = a.y; g.pout = a.pout; g.tol = a.tol;
    return g;
}

// One layer forward (rev: inverse) and the sum of its log J partials: logJ[b] = (accumulate ? logJ[b] : 0) + sum over the tiles
// (logJ null: no sum).  `a` carries the fields, weights and stripe; l: the layer's place in the caller's weights.
int layer_forward(const Ctx& C, const WS& W, int l, FlowLayerArgs a, bool rev, double* logJ, int accumulate = 0) {
    if (C.gen()) {                                // any other net shape (flow_generic.hip)
        GenLayerArgs g = gen_one_layer(C, W, l, a);
        g.logj = logJ; g.logj_accumulate = accumulate;
        if (a.stash) g.stash = a.stash;
        return launch_gen_fwd(g, rev, C.s);
    }
    a.logj_part = W.lj_part;
    FT_TRY(rev ? flow_rev(C, a, C.s) : flow_fwd(C, a, C.s));
    if (logJ) FT_TRY(launch_sum_parts(W.lj_part, a.B, flow_fwd_geom(C.mfma).ntiles(a.L), 1.0, accumulate, logJ, C.s));
    return FTHMC_OK;
}

// One layer backward from its stash (a.stash; a.gp_out = the plaquette gradient behind the layer); gw != null: also the layer's
// weight gradient, from the pre-activation gradients the backward kernel leaves in W.gz (two kernels and the reduction)
int layer_backward_stash(const WS& W, FlowLayerArgs a, double* gw, hipStream_t s) {
    a.gw_part = W.gw_part;
    a.gz = gw ? W.gz : nullptr;
    FT_TRY(launch_flow_bwd_gather(a, s));
    if (gw) {
        a.tpw = flow_wgrad_tpw(a.B, a.L, 1);
        FT_TRY(launch_flow_wgrad(a, s));
        FT_TRY(launch_reduce_gw(W.gw_part, flow_wgrad_nparts(a.B, a.L, a.tpw), 1.0, 0, gw, W.gw_tmp, s));
    }
    return FTHMC_OK;
}

// VJP of one layer (plain or MFMA kernels), seeded by a.up_link and a.glogj, into W.gp: the layer's plaquette gradient alone (no upstream
// gP field); gw (optional): its weight gradient.  stash: the caller's activation stash; null: the layer runs forward once first (a.x / a.pin)
int layer_vjp(const Ctx& C, const WS& W, FlowLayerArgs a, const double* stash, double* gw) {
    if (C.gen()) {
        GenLayerArgs g = gen_one_layer(C, W, 0, a);
        if (stash) g.stash = const_cast<double*>(stash);
        else FT_TRY(launch_gen_fwd(g, false, C.s));               // fills the layer's planes
        g.up_link = a.up_link; g.glogj = a.glogj; g.gp_out = W.gp; g.gw = gw;
        return launch_gen_bwd(g, C.s);
    }
    a.gw_part = W.gw_part;
    if (stash) { a.stash = const_cast<double*>(stash); a.stash_h = 1; }
    else {                                                        // forward with the stash (no link update, no log J)
        a.stash = W.stash; a.stash_h = gw ? 1 : 0;
        // link level with weight gradients: the launch of fthmc_flow_layer_fwd_stash (links into W.X, log J partials; nobody reads them)
        // -- on the exact tiles that is the training-sweep instance of the forward, and the instances of one kernel round their
        // stash differently in the last bit (fp contraction follows the code around it): so this call and the two-call route
        // give the same bits on every shape.  Without them the workspace holds the force stash only (no h1, h2): another
        // instance than a caller's stash came from, equal to round-off.
        if (gw && !a.pin) { a.y = W.X; a.logj_part = W.lj_part; }
        FT_TRY(launch_flow_fwd_mfma(a, C.s));
        a.y = nullptr; a.logj_part = nullptr;
    }
    a.gp_out = W.gp;
    return layer_backward_stash(W, a, gw, C.s);
}

// a forward layer whose output field IS its input field updates only the links it changes, where the kernel has that instance
inline bool layer_inplace(const Ctx& C, int L, int act) { return C.mfma && !C.gen() && flow_fwd_inplace_ok(L, act); }

// Forward sweep x -> X[0..nl-1] (X[l] = output of layer l).  logdet (device [B]) optional.
// MFMA variant on the exact tiles (flow_fwd_inplace_ok): no checkpoints -- layer 0 maps the caller's field (never written) into
// the LAST region of w.X, layers 1 .. nl - 1 update that region in place, each touching only the links it changes (flow_fwd.hip
// INPL); phys_field() names the same region either way.  Nothing behind such a sweep reads a checkpoint: the stash backward
// kernels (flow_bwd_gather.hip, flow_bwd_train.hip, flow_wgrad.hip) never dereference FlowLayerArgs::x.  The VALU variant
// (its backward recomputes each layer from X[l - 1]), the ragged and non-silu shapes and the plain kernels keep the chain.
// parts_only: leave the log J partials of every layer in w.lj_part ([layer][chain][tile]) and skip the summing launch (the
// caller folds them into its own reduction: launch_traj_energy); tuned kernels only.
int sweep_forward(const Ctx& C, const double* x, const WS& w, int nl, int B, int L, int act, double* logdet,
                  hipStream_t s, bool stash = false, bool train = false, bool parts_only = false) {
    // any other net shape: plain kernels, one stash region per layer
    if (C.gen()) return gen_forward<double>(C, gen_ws(C, w, B, L), x, nl, B, L, act, stash, logdet);
    const bool inplace = layer_inplace(C, L, act);
    for (int l = 0; l < nl; ++l) {
        FlowLayerArgs a(w.wint, l, B, L, act);
        a.stash = stash ? w.stash + (size_t)l * flow_stash_doubles(B, L, train) : nullptr;
        a.stash_h = train ? 1 : 0;
        // the layers behind this one write their stash before the backward reads this one's: beyond STASH_FAR_BYTES of it the
        // 256 MB Infinity Cache will have let go of this layer's (the forward then stores it past the caches: flow_fwd.hip)
        a.stash_far = stash && (size_t)(nl - 1 - l) * flow_stash_doubles(B, L, train) * sizeof(double) >= STASH_FAR_BYTES ? 1 : 0;
        a.x = l == 0 ? x : w.X + (size_t)(l - 1) * w.n2;
        a.y = w.X + (size_t)l * w.n2;
        if (inplace) { a.y = w.X + (size_t)(nl - 1) * w.n2; if (l > 0) { a.x = a.y; a.inplace = 1; } }
        // logJ partials of all layers side by side, summed by ONE launch behind the sweep (layer by layer, in order)
        a.logj_part = (logdet || parts_only) ? w.lj_part + (size_t)l * B * flow_fwd_geom(C.mfma).ntiles(L) : nullptr;
        FT_TRY(flow_fwd(C, a, s));
    }
    if (logdet && nl > 0) FT_TRY(launch_sum_parts(w.lj_part, B, flow_fwd_geom(C.mfma).ntiles(L), 1.0, 0, logdet, s, nl));
    return FTHMC_OK;
}

inline const double* phys_field(const double* x, const WS& w, int nl) { return flowed_field<double>(x, w.X, nl, w.n2); }

// S_eff (and friends) of x; leaves the flowed field (phys_field) in w.X
int eval_action(const Ctx& C, const double* x, const WS& w, int nl, int B, int L, int act, double beta,
                double* S_eff, double* logdet, double* plaq, double* Q, hipStream_t s) {
    double* ld = logdet ? logdet : w.scal + (size_t)SC_LOGDET * B;
    if (nl > 0) FT_TRY(sweep_forward(C, x, w, nl, B, L, act, ld, s));
    double* S = w.scal + (size_t)SC_S * B;
    FT_TRY(launch_action_charge(phys_field(x, w, nl), B, L, beta, S, Q, plaq, s, w.act_part));
    if (S_eff) FT_TRY(launch_lincomb(S, 1.0, nl > 0 ? ld : nullptr, -1.0, 0.0, S_eff, B, s));
    return FTHMC_OK;
}

// The bias V(Q_m) of the flowed field (metadynamics) as force_gp and ft_md_ws take it: the table and sums[B][2]
struct FlowBias { MetaTab T; double* sums; };
// The defect of the flowed field (boundary-condition tempering through the flow) as force_gp and ft_md_ws take it
struct FlowDefect { const double* g_b; DefectLine df; };

// Plaquette-gradient field of sum_b S_eff (scaled): gp = scale*beta*sin P(F(x)) + sum_l gP_l,
// with dL/dlogJ = glogj.  gw != null also accumulates weight gradients (training).
// beta_b (optional): per-chain beta in place of beta_scaled (the per-chain-beta trajectories: fthmc_*_pb)
// bias (optional): the seed is beta sin P + c_b cos P of the flowed field, c_b from the chain's sin sum (launch_meta_sums, launch_meta_gp)
// defect (optional, no bias beside it): the seed is w sin P of the flowed field, w = g_b on the defect and beta elsewhere (launch_defect_gp: one pass)
int force_gp(const Ctx& C, const double* x, const WS& w, int nl, int B, int L, int act, double beta_scaled,
             double glogj, double* gw, hipStream_t s, bool have_forward = false, const double* beta_b = nullptr,
             const FlowBias* bias = nullptr, const FlowDefect* defect = nullptr) {
    auto seed = [&](double* gp) {
        if (defect) return launch_defect_gp(phys_field(x, w, nl), B, L, beta_scaled, defect->g_b, defect->df, gp, s);
        if (!bias) return launch_wilson_gp(phys_field(x, w, nl), B, L, beta_scaled, gp, s, beta_b);
        FT_TRY(launch_meta_sums(phys_field(x, w, nl), B, L, bias->sums, s));
        return launch_meta_gp(phys_field(x, w, nl), B, L, beta_scaled, bias->sums, bias->T, gp, s);
    };
    if (C.gen()) {                                // any other net shape (flow_generic.hip)
        if (nl > 0 && !have_forward) FT_TRY(sweep_forward(C, x, w, nl, B, L, act, nullptr, s, true));
        return gen_backward<double>(C, gen_ws(C, w, B, L), nl, B, L, act, nullptr, glogj, gw, seed);
    }
    // MFMA path without weight gradients: the forward sweep stashes act'(z1), act'(z2), s per site
    // and the backward kernels read them back instead of recomputing the network
    // (training: the caller ran the forward with the h planes stashed too, have_forward = true)
    const bool mfma = C.mfma;
    const bool stash = mfma && (gw == nullptr ? !have_forward : have_forward);
    const bool train = gw != nullptr && stash;
    if (nl > 0 && !have_forward) FT_TRY(sweep_forward(C, x, w, nl, B, L, act, nullptr, s, stash));
    // stash path: gather-form backward, gP ping-pongs between two fields and ends in w.gp
    double* gcur = (stash && (nl & 1)) ? w.gp2 : w.gp;
    double* galt = gcur == w.gp ? w.gp2 : w.gp;
    FT_TRY(seed(gcur));
    // training on the tiled-exactly shapes: the layer's backward and its weight gradients in ONE kernel (flow_bwd_train.hip: the
    // pre-activation gradients never leave LDS), one partial per workgroup
    const bool fused = gw && train && fused_train_bwd(C.A, B, L);
    const int npf = fused ? (int)flow_bwd_train_nparts(B, L) : 0;
    // the layers' partials side by side and ONE reduction behind the sweep (two launches instead of two per layer), where the
    // workspace has the rows (a training layout: ws_layout)
    const bool one_reduction = fused && (size_t)nl * npf <= w.gw_rows && (size_t)nl * flow_reduce_groups(npf) <= w.gw_tmp_rows;
    for (int l = nl - 1; l >= 0; --l) {
        FlowLayerArgs a(w.wint, l, B, L, act);
        if (!stash) a.x = l == 0 ? x : w.X + (size_t)(l - 1) * w.n2;  // the VALU backward recomputes the layer; the stash kernels read no field
        a.up_gp = gcur;
        a.glogj_const = glogj;
        a.gp_part = w.gp_part;
        a.gw_part = w.gw_part;
        double* gwl = gw ? gw + (size_t)l * FTHMC_W_PER_LAYER : nullptr;
        if (!stash) {                                                 // VALU variant: scatter form + gather
            FT_TRY(launch_flow_bwd(a, gw != nullptr, s));
            if (gw) FT_TRY(launch_reduce_gw(w.gw_part, B * flow_geom(false).ntiles(L), 1.0, 0, gwl, w.gw_tmp, s));
            FT_TRY(launch_gather_gp(w.gp_part, B, L, flow_geom(false), 1, gcur, s));
            continue;
        }
        a.stash = w.stash + (size_t)l * flow_stash_doubles(B, L, train);
        a.gp_out = galt;
        if (fused) {
            if (one_reduction) a.gw_part = w.gw_part + (size_t)l * npf * FLOW_GW_STRIDE;
            FT_TRY(launch_flow_bwd_train(a, s));
            if (!one_reduction) FT_TRY(launch_reduce_gw(w.gw_part, npf, 1.0, 0, gwl, w.gw_tmp, s));
        } else {
            FT_TRY(layer_backward_stash(w, a, gwl, s));
        }
        std::swap(gcur, galt);
    }
    if (one_reduction && nl > 0) FT_TRY(launch_reduce_gw(w.gw_part, npf, 1.0, 0, gw, w.gw_tmp, s, nl, (size_t)npf * FLOW_GW_STRIDE));
    return FTHMC_OK;
}

// The MD of a schedule (integrator.h) in the latent field: x += b0 v, then per stage one force evaluation and KICK(a, b), or
// SHIFT(c): the shifted field goes to `xshift` and the next stage's force is evaluated there (w.xa and w.va are untouched by
// it; the leapfrog has no such stage and reads no `xshift`).  nl = 0 is the plain Wilson MD (launch_wilson_gp + kick).  Result
// in w.xa / w.va.  xreg (optional): regularize(result x), written by the last kick (the end point of a trajectory,
// ipynb/ft_hmc.py:426) -- it may be `xshift` itself: nothing reads the shifted field once the kick behind it has its gP.
int ft_md_ws(const Ctx& C, const double* x, const double* v, const WS& w, int nl, int B, int L, int act, double beta,
             const Sched& sc, hipStream_t s, double* xshift, double* xreg = nullptr, const double* beta_b = nullptr,
             const FlowBias* bias = nullptr, const FlowDefect* defect = nullptr) {
    FT_TRY(launch_axpy_copy(x, v, sc.b0, w.xa, w.va, w.n2, s));
    const double* xe = w.xa;                                               // where this stage's force is evaluated
    for (int it = 0; it < sc.n; ++it) {
        const SchedStage st = sc.stage(it);
        FT_TRY(force_gp(C, xe, w, nl, B, L, act, beta, -1.0, nullptr, s, false, beta_b, bias, defect));
        if (st.kind == FT_STAGE_SHIFT) {
            FT_TRY(launch_shift_from_gp(w.gp, w.xa, xshift, B, L, st.a, s));
            xe = xshift;
        } else {
            FT_TRY(launch_kick_from_gp(w.gp, w.va, w.xa, nullptr, B, L, st.a, st.b, s, it == sc.n - 1 ? xreg : nullptr));
            xe = w.xa;
        }
    }
    return FTHMC_OK;
}

// the schedule of an entry point's (integrator, dt, nstep): FTHMC_ERR_UNSUPPORTED for an unknown integrator
inline int sched_of(int integrator, double dt, int nstep, Sched* sc) {
    const int n = make_sched(integrator, dt, nstep, sc);
    return n >= 1 ? FTHMC_OK : (n == -2 ? FTHMC_ERR_UNSUPPORTED : FTHMC_ERR_ARG);
}

// plain leapfrog; result pointers returned through xo/po (ping-pong inside the workspace)
int leapfrog_ws(const double* x, const double* p, const WS& w, int B, int L, double beta, double dt,
                int nstep, double** xo, double** po, hipStream_t s, const double* beta_b = nullptr) {
    const double* xi = x; const double* pi = p;
    double* xs[2] = {w.xa, w.xb}; double* ps[2] = {w.va, w.vb};
    int cur = 0;
    for (int k = 0; k < nstep; ++k) {
        FT_TRY(launch_leap_step(xi, pi, xs[cur], ps[cur], B, L, beta, k == 0 ? 0.5 * dt : dt, dt, s, beta_b));
        xi = xs[cur]; pi = ps[cur]; cur ^= 1;
    }
    // final half drift into the free x buffer
    FT_TRY(launch_axpy(xi, pi, 0.5 * dt, xs[cur], w.n2, s));
    *xo = xs[cur]; *po = const_cast<double*>(pi);
    return FTHMC_OK;
}

// the result pair of an MD entry point
inline int copy_pair(double* x_out, const double* xo, double* v_out, const double* vo, size_t n2, hipStream_t s) {
    if (hipMemcpyAsync(x_out, xo, n2 * sizeof(double), hipMemcpyDeviceToDevice, s) != hipSuccess ||
        hipMemcpyAsync(v_out, vo, n2 * sizeof(double), hipMemcpyDeviceToDevice, s) != hipSuccess)
        return FTHMC_ERR_LAUNCH;
    return FTHMC_OK;
}

// The bare MD behind fthmc_leapfrog / fthmc_md (`plain`: no flow, no weights, never the one-launch path) and fthmc_ft_leapfrog_v /
// fthmc_ft_md_v.  fthmc_leapfrog keeps the fused launch_leap_step steps (leapfrog_ws); everything else is ft_md_ws.
int md_call(bool plain, const double* x, const double* v, const double* w, const fthmc_arch_t* arch, int nl, int B, int L, int act,
            double beta, double dt, int nstep, int integrator, double* x_out, double* v_out, void* ws, size_t ws_bytes,
            void* stream, uint64_t wver) {
    FT_TRY(check_flow_call(x && v && x_out && v_out && nstep >= 1, w, nl, B, L, act));
    const bool leap = integrator == FTHMC_INT_LEAPFROG;
    Sched sc;
    FT_TRY(sched_of(integrator, dt, nstep, &sc));
    Ctx C; WS W; FT_TRY(open_call(arch, stream, &C));
    FT_TRY(open_ws(C, ws, ws_bytes, B, L, nl, false, &W));
    const hipStream_t s = C.s;
    if (plain && leap) {
        double *xo, *po;
        FT_TRY(leapfrog_ws(x, v, W, B, L, beta, dt, nstep, &xo, &po, s));
        return copy_pair(x_out, xo, v_out, po, W.n2, s);
    }
    if (!plain) {
        FT_TRY(use_weights(C, w, nl, W.wint, wver));
        if (C.small(L, nl)) {                                            // the whole MD in one launch
            SmallArgs a = small_args(x, W, nl, B, act, beta, 2);
            a.v = v; a.dt = dt; a.nstep = nstep; a.x_out = x_out; a.v_out = v_out;
            return leap ? launch_ft_small(a, L, s) : launch_ft_small_sched(a, sc, L, s);
        }
    }
    FT_TRY(ft_md_ws(C, x, v, W, nl, B, L, act, beta, sc, s, W.xb));
    return copy_pair(x_out, W.xa, v_out, W.va, W.n2, s);
}

// ---------------------------------------------------------------- metadynamics (meta.hip; no reference counterpart)
// The table of a call, or FTHMC_ERR_ARG: what every fthmc_meta_* and fthmc_ft_meta_* call refuses about it.  `wall`: the wall's
// stiffness (fthmc_meta_deposit: a hill's height, held to the same rule)
inline int meta_tab(const double* vtab, int B, int G, int nb, double qmax, double wall, MetaTab* T) {
    if (!vtab || G < 1 || B % G != 0 || nb < 2 || nb > 65536 || !isfinite(qmax) || !(qmax > 0.0) || !isfinite(wall) || !(wall >= 0.0))
        return FTHMC_ERR_ARG;
    *T = MetaTab{vtab, B / G, nb, qmax, wall};
    return FTHMC_OK;
}
// The optional bias of a trajectory call: the table, the path the caller asked for (the plain sequence: fthmc_meta_trajectory) and
// where Q_m and V(Q_m) of x_new go (each optional)
struct BiasArg { MetaTab T; int path; double *qm_out, *vb_out; };

// the sequenced paths launch the plain kernels' shapes (launch_kick_from_gp, launch_shift_from_gp, k_meta_gp: the chain on grid y)
constexpr int META_SEQ_MAX_B = 65535;

// Plain HMC: H0, MD, H1, Metropolis -- the one sequence behind fthmc_hmc_trajectory, _int and _pb and, with a bias, behind
// fthmc_meta_trajectory.  beta_b: per-chain beta (null: the scalar `beta`; the kernels that take beta_b are handed beta = 0.0
// beside it).  bias (optional): V(Q_m) in every force (ft_md_ws' FlowBias) and behind either energy, and the (Q_m, V) pairs of
// the two ends through the Metropolis kernel beside the field; any L, x_new may be x on the sequenced path.
int hmc_trajectory_call(const double* x, const double* v, const double* u, int B, int L, double beta, const double* beta_b, double dt,
                        int nstep, int integrator, const BiasArg* bias, double* x_new, double* dH, double* acc, double* H0, double* H1,
                        void* ws, size_t ws_bytes, void* stream) {
    if (!x || !v || !u || !x_new || bad_shape(B, L) || nstep < 1 || (bias && beta_b)) return FTHMC_ERR_ARG;
    const bool pb = beta_b != nullptr, leap = integrator == FTHMC_INT_LEAPFROG;
    if (pb) beta = 0.0;
    Sched sc;
    FT_TRY(sched_of(integrator, dt, nstep, &sc));
    Ctx C; FT_TRY(open_call(nullptr, stream, &C));
    const hipStream_t s = C.s;
    // L <= HMC_RESIDENT_MAXL (x_new must not alias x): one persistent launch per trajectory, state in LDS / registers.  The scalar-beta leapfrog
    // has a kernel of its own, the schedule-driven one serves every other integrator and per-chain beta with every integrator,
    // the biased one every integrator (path 1: the caller insists on it, 2: on the sequence).
    const bool one_launch = L <= HMC_RESIDENT_MAXL && C.mfma && x_new != x;
    if (bias) {
        if (bias->path == 1 || (bias->path == 0 && one_launch))
            return launch_meta_trajectory(x, v, u, B, L, beta, sc, bias->T, x_new, dH, acc, H0, H1, bias->qm_out, bias->vb_out, s);
        if (B > META_SEQ_MAX_B) return FTHMC_ERR_UNSUPPORTED;
    } else if (one_launch) {
        return leap && !pb ? launch_hmc_trajectory_fused(x, v, u, B, L, beta, dt, nstep, x_new, dH, acc, H0, H1, s)
                           : launch_hmc_trajectory_sched(x, v, u, B, L, beta, sc, x_new, dH, acc, H0, H1, s, beta_b);
    }
    MWS M{};                                                         // unbiased: no sums, no pairs (null, 0 rows)
    FT_TRY(bias ? open_meta_ws(C, ws, ws_bytes, B, L, 0, true, &M) : open_ws(C, ws, ws_bytes, B, L, 0, false, &M.W));
    const WS& W = M.W;
    const FlowBias fb{bias ? bias->T : MetaTab{}, M.sums};
    double* S = W.scal + (size_t)SC_S * B; double* K = W.scal + (size_t)SC_K * B;
    auto energy = [&](const double* xf, const double* vf, double* h, double* qv) {     // h = S_W(xf) + K(vf) / 2 [+ V(Q_m(xf))]
        FT_TRY(launch_action_charge(xf, B, L, beta, S, nullptr, nullptr, s, nullptr, beta_b));
        FT_TRY(launch_kinetic(vf, B, L, K, s));
        FT_TRY(launch_lincomb(S, 1.0, K, 0.5, 0.0, h, B, s));
        if (!bias) return FTHMC_OK;
        FT_TRY(launch_meta_sums(xf, B, L, M.sums, s));
        return launch_meta_energy(M.sums, B, fb.T, h, qv, s);
    };
    double* h0 = H0 ? H0 : W.scal + (size_t)SC_H0 * B;
    double* h1 = H1 ? H1 : W.scal + (size_t)SC_H1 * B;
    FT_TRY(energy(x, v, h0, M.qv_old));
    double *xo = W.xb, *po = W.va;
    if (leap && !bias) {                                             // the fused launch_leap_step steps, then xr = regularize(x_)
        FT_TRY(leapfrog_ws(x, v, W, B, L, beta, dt, nstep, &xo, &po, s, beta_b));
        FT_TRY(launch_wrap(xo, xo, W.n2, 1, s));
    } else {                                                         // the flowed schedule with zero layers: the shifted field
        FT_TRY(ft_md_ws(C, x, v, W, 0, B, L, 0, beta, sc, s, W.xb, W.xb, beta_b, bias ? &fb : nullptr));      // and then the regularized end point in W.xb
    }
    FT_TRY(energy(xo, po, h1, M.qv_new));
    FT_TRY(launch_metropolis(x, xo, u, h0, h1, B, L, 0, x_new, dH, acc, M.qv_old, M.qv_new, M.qv_sel, bias ? 2 : 0, s));
    if (!bias) return FTHMC_OK;
    const size_t row = (size_t)B * sizeof(double);
    if (bias->qm_out && hipMemcpyAsync(bias->qm_out, M.qv_sel, row, hipMemcpyDeviceToDevice, s) != hipSuccess) return FTHMC_ERR_LAUNCH;
    if (bias->vb_out && hipMemcpyAsync(bias->vb_out, M.qv_sel + B, row, hipMemcpyDeviceToDevice, s) != hipSuccess) return FTHMC_ERR_LAUNCH;
    return FTHMC_OK;
}

// ---------------------------------------------------------------- boundary-condition tempering (defect.hip; no reference counterpart)
// The workspace of fthmc_defect_trajectory's sequenced path: a first-order layout without layers and behind it the (C, Dsum, Q) rows
// of the two ends and of the selected one, [3][B] each
struct DWS { WS W; double *old, *neu, *sel; size_t total; };
DWS defect_layout(Carver& c, int B, int L) {
    DWS d{};
    d.W = ws_layout(flow_arch_default(), c, B, L, 0);
    if (d.W.total == 0) return d;
    d.old = c.take((size_t)3 * B); d.neu = c.take((size_t)3 * B); d.sel = c.take((size_t)3 * B);
    d.total = c.total();
    return d;
}
// what every fthmc_defect_* call refuses about the defect and the couplings
inline bool bad_defect(int L, double beta, const double* g_b, int i0, int j0, int Ld) {
    return !g_b || !isfinite(beta) || Ld < 0 || Ld > L || i0 < 0 || i0 >= L || j0 < 0 || j0 >= L;
}

// Plain HMC with a defect: H0, MD, H1, Metropolis -- hmc_trajectory_call's per-chain-beta sequence (the schedule with zero layers: ft_md_ws)
// with the weighted plane in every force, (beta - g_b) Dsum behind either energy and the (C, Dsum, Q) rows of the two ends through the
// Metropolis kernel beside the field; a sibling of that sequence, which keeps its launches.  Any L, x_new may be x on the sequenced path.
int defect_trajectory_call(const double* x, const double* v, const double* u, int B, int L, double beta, const double* g_b,
                           const DefectLine& df, double dt, int nstep, int integrator, int path, double* x_new, double* dH, double* acc,
                           double* H0, double* H1, double* csum_out, double* dsum_out, double* q_out, void* ws, size_t ws_bytes,
                           void* stream) {
    Sched sc;
    FT_TRY(sched_of(integrator, dt, nstep, &sc));
    Ctx C; FT_TRY(open_call(nullptr, stream, &C));
    const hipStream_t s = C.s;
    const bool one_launch = L <= HMC_RESIDENT_MAXL && C.mfma && x_new != x;       // as hmc_trajectory_call chooses
    if (path == 1 || (path == 0 && one_launch))
        return launch_defect_trajectory(x, v, u, B, L, beta, g_b, df, sc, x_new, dH, acc, H0, H1, csum_out, dsum_out, q_out, s);
    if (B > META_SEQ_MAX_B) return FTHMC_ERR_UNSUPPORTED;
    Carver c(ws, ws_bytes);
    const DWS D = defect_layout(c, B, L);
    FT_TRY(check_ws(D.total, ws, ws_bytes));
    const WS& W = D.W;
    double* S = W.scal + (size_t)SC_S * B; double* K = W.scal + (size_t)SC_K * B;
    auto energy = [&](const double* xf, const double* vf, double* h, double* sums) {   // h = (-beta) C + K(vf) / 2 + (beta - g_b) Dsum
        FT_TRY(launch_defect_sums(xf, B, L, beta, df, S, sums, s));
        FT_TRY(launch_kinetic(vf, B, L, K, s));
        FT_TRY(launch_lincomb(S, 1.0, K, 0.5, 0.0, h, B, s));
        return launch_defect_energy(sums, B, beta, g_b, h, s);
    };
    double* h0 = H0 ? H0 : W.scal + (size_t)SC_H0 * B;
    double* h1 = H1 ? H1 : W.scal + (size_t)SC_H1 * B;
    FT_TRY(energy(x, v, h0, D.old));
    FT_TRY(launch_axpy_copy(x, v, sc.b0, W.xa, W.va, W.n2, s));        // ft_md_ws' loop with the weighted plane as its force's seed
    const double* xe = W.xa;
    for (int it = 0; it < sc.n; ++it) {
        const SchedStage st = sc.stage(it);
        FT_TRY(launch_defect_gp(xe, B, L, beta, g_b, df, W.gp, s));
        if (st.kind == FT_STAGE_SHIFT) {
            FT_TRY(launch_shift_from_gp(W.gp, W.xa, W.xb, B, L, st.a, s));
            xe = W.xb;
        } else {
            FT_TRY(launch_kick_from_gp(W.gp, W.va, W.xa, nullptr, B, L, st.a, st.b, s, it == sc.n - 1 ? W.xb : nullptr));
            xe = W.xa;
        }
    }
    FT_TRY(energy(W.xb, W.va, h1, D.neu));                            // W.xb: the regularized end point
    // rows 1 and 2 of the selected end (Dsum, Q) leave through the Metropolis kernel itself, row 0 (C) by one copy
    FT_TRY(launch_metropolis(x, W.xb, u, h0, h1, B, L, 0, x_new, dH, acc, D.old, D.neu, D.sel, 3, s, dsum_out, q_out));
    if (csum_out && hipMemcpyAsync(csum_out, D.sel, (size_t)B * sizeof(double), hipMemcpyDeviceToDevice, s) != hipSuccess) return FTHMC_ERR_LAUNCH;
    return FTHMC_OK;
}

// ---------------------------------------------------------------- per-chain beta and replica exchange (no reference counterpart)
// The beta-free triple (log det J, C = sum cos P, Q) of x into `trip` -- carried over (state_in) or evaluated -- and S_eff of it
// at beta_b into `seff`: the general branch's eval_action + launch_lincomb with beta read per chain
int pb_eval(const Ctx& C, const double* x, const WS& W, int nl, int B, int L, int act, const double* beta_b,
            const double* state_in, double* trip, double* seff, hipStream_t s) {
    if (state_in) {
        if (hipMemcpyAsync(trip, state_in, (size_t)3 * B * sizeof(double), hipMemcpyDeviceToDevice, s) != hipSuccess) return FTHMC_ERR_LAUNCH;
    } else {
        if (nl > 0) FT_TRY(sweep_forward(C, x, W, nl, B, L, act, trip, s));
        else if (hipMemsetAsync(trip, 0, (size_t)B * sizeof(double), s) != hipSuccess) return FTHMC_ERR_LAUNCH;
        FT_TRY(launch_action_charge(phys_field(x, W, nl), B, L, 0.0, nullptr, trip + 2 * B, nullptr, s, W.act_part, beta_b, trip + B));
    }
    return launch_pb_from_state(trip, beta_b, B, L, nl > 0, seff, nullptr, s);
}

// What every fthmc_ft_meta_* call refuses about its arguments -- FTHMC_ERR_ARG, the table included; FTHMC_ERR_UNSUPPORTED for the
// activation behind it -- and what it then opens in the ABI's order: FTHMC_ERR_UNSUPPORTED, the workspace (the first-order layout
// and sums[B][2] behind it), the weights.  seq_always: the force and action entry points, which never take the one-launch path.
int check_ft_meta_args(bool ptrs_ok, const double* w, int nl, int B, int L, int act, const double* vtab, int G, int nb, double qmax,
                       double wall, MetaTab* T) {
    if (meta_tab(vtab, B, G, nb, qmax, wall, T) != FTHMC_OK) return FTHMC_ERR_ARG;
    return check_flow_call(ptrs_ok, w, nl, B, L, act);
}
int open_ft_meta_call(const fthmc_arch_t* arch, void* stream, void* ws, size_t ws_bytes, const double* w, int nl, int B, int L,
                      bool seq_always, uint64_t wver, Ctx* C, MWS* M) {
    FT_TRY(open_call(arch, stream, C));
    if ((seq_always || !C->small(L, nl)) && B > META_SEQ_MAX_B) return FTHMC_ERR_UNSUPPORTED;
    if (C->A.is_default() && nl > 0 && B > (1 << 20)) return FTHMC_ERR_UNSUPPORTED;     // (open_ws: the default net's kernels)
    FT_TRY(open_meta_ws(*C, ws, ws_bytes, B, L, nl, false, M));
    return use_weights(*C, w, nl, M->W.wint, wver);
}

// The workspace of the fthmc_ft_defect_* calls: a first-order layout and behind it the (C, Dsum, Q) rows launch_defect_sums leaves
struct FDWS { WS W; double* sums; size_t total; };
FDWS ft_defect_layout(const FlowArch& A, Carver& c, int B, int L, int nl) {
    FDWS d{};
    d.W = ws_layout(A, c, B, L, nl);
    if (d.W.total == 0) return d;
    d.sums = c.take((size_t)3 * B);
    d.total = c.total();
    return d;
}
// The optional defect of a flowed trajectory call: the couplings, the line and where Dsum of x_new goes (optional)
struct DefectArg { const double* g_b; DefectLine df; double* dsum_out; };
// What every fthmc_ft_defect_* call refuses about its arguments -- FTHMC_ERR_ARG, the defect included; FTHMC_ERR_UNSUPPORTED for the
// activation behind it -- and what it then opens in the ABI's order: FTHMC_ERR_UNSUPPORTED (the sequenced kernels put the chain on
// grid y), the workspace (the first-order layout and the three rows behind it), the weights.  seq_always: the force and action entry
// points, which never take the one-launch path.
int check_ft_defect_args(bool ptrs_ok, const double* w, int nl, int B, int L, int act, double beta, const double* g_b, int i0, int j0, int Ld) {
    if (bad_defect(L, beta, g_b, i0, j0, Ld)) return FTHMC_ERR_ARG;
    return check_flow_call(ptrs_ok, w, nl, B, L, act);
}
int open_ft_defect_call(const fthmc_arch_t* arch, void* stream, void* ws, size_t ws_bytes, const double* w, int nl, int B, int L,
                        bool seq_always, uint64_t wver, Ctx* C, FDWS* D) {
    FT_TRY(open_call(arch, stream, C));
    if ((seq_always || !C->small(L, nl)) && B > META_SEQ_MAX_B) return FTHMC_ERR_UNSUPPORTED;
    if (C->A.is_default() && nl > 0 && B > (1 << 20)) return FTHMC_ERR_UNSUPPORTED;     // (open_ws: the default net's kernels)
    Carver c(ws, ws_bytes);
    *D = ft_defect_layout(C->A, c, B, L, nl);
    FT_TRY(check_ws(D->total, ws, ws_bytes));
    return use_weights(*C, w, nl, D->W.wint, wver);
}

// The flowed trajectory: H0, MD, H1, Metropolis, plaq / Q of x_new -- the one sequence behind fthmc_ft_trajectory_v, _int_v and
// _pb_v and, with a bias, behind fthmc_ft_meta_trajectory_v.  beta_b: per-chain beta (null: the scalar `beta`); the state triples
// are then BETA-FREE (log det J, sum cos P, Q) instead of (S_eff, plaq, Q), and the kernels that take beta_b are handed
// beta = 0.0 beside it.  bias (optional, FTHMC_MODE_MD and scalar beta only): V(Q_m) of the physical field in every force
// (ft_md_ws' FlowBias) and behind either end's energy; the state has a fourth row, Q_m, and is TABLE-FREE -- [4][B] = (S_eff
// unbiased, plaq, Q, Q_m): V of a carried Q_m is looked up in the table of this call.
// dfa (optional, FTHMC_MODE_MD, scalar beta, no bias): the defect of the physical field -- w sin P seeds every force
// (ft_md_ws' FlowDefect), (beta - g_b) Dsum goes behind either end's energy; the state has a fourth row, Dsum, and is G-FREE --
// [4][B] = (S_eff of the periodic action, plaq, Q, Dsum).
int ft_trajectory_call(const double* x, const double* v, const double* u, const double* w, const fthmc_arch_t* arch, int nl, int B,
                       int L, int act, double beta, const double* beta_b, double dt, int nstep, int integrator, int mode,
                       const BiasArg* bias, double* x_new, double* dH, double* acc, double* H0, double* H1, double* plaq, double* Q,
                       const double* state_in, double* state_out, void* ws, size_t ws_bytes, void* stream, uint64_t wver,
                       const DefectArg* dfa = nullptr) {
    FT_TRY(check_flow_call(x && v && u && x_new && nstep >= 1, w, nl, B, L, act));
    const bool pb = beta_b != nullptr, leap = integrator == FTHMC_INT_LEAPFROG;
    if (pb) beta = 0.0;
    if (mode != FTHMC_MODE_MD && mode != FTHMC_MODE_LITERAL) return FTHMC_ERR_UNSUPPORTED;
    // FTHMC_MODE_LITERAL discards the MD: no integrator to choose, and no per-chain form of it
    if (mode == FTHMC_MODE_LITERAL && (!leap || pb)) return FTHMC_ERR_UNSUPPORTED;
    const bool md = mode == FTHMC_MODE_MD;
    if ((bias || dfa) && (pb || !md)) return FTHMC_ERR_UNSUPPORTED;
    if (bias && dfa) return FTHMC_ERR_UNSUPPORTED;
    Sched sc;
    FT_TRY(sched_of(integrator, dt, nstep, &sc));
    Ctx C; MWS M{}; FDWS D{};
    if (dfa) { FT_TRY(open_ft_defect_call(arch, stream, ws, ws_bytes, w, nl, B, L, false, wver, &C, &D)); M.W = D.W; }
    else FT_TRY(bias ? open_ft_meta_call(arch, stream, ws, ws_bytes, w, nl, B, L, false, wver, &C, &M)
                     : open_flow_call(arch, stream, ws, ws_bytes, w, nl, B, L, false, wver, &C, &M.W));
    const WS& W = M.W;
    const hipStream_t s = C.s;
    const FlowBias fb{bias ? bias->T : MetaTab{}, M.sums};
    const FlowBias* fbp = bias ? &fb : nullptr;
    const FlowDefect fd{dfa ? dfa->g_b : nullptr, dfa ? dfa->df : DefectLine{}};
    const FlowDefect* fdp = dfa ? &fd : nullptr;
    if (md && C.small(L, nl)) {                                      // the whole trajectory in one launch
        SmallArgs a = small_args(x, W, nl, B, act, beta, 3);
        a.v = v; a.u = u; a.dt = dt; a.nstep = nstep; a.x_out = x_new; a.state_in = state_in; a.state_out = state_out;
        a.dH = dH; a.acc = acc; a.H0 = H0; a.H1 = H1; a.plaq = plaq; a.Q = Q;
        // five instances of k_ft_small: the biased one, the one with a defect and per-chain beta run the schedule-driven one with
        // every integrator, the leapfrog included
        if (dfa) return launch_ft_small_defect(a, sc, dfa->g_b, dfa->df, dfa->dsum_out, L, s);
        if (bias) return launch_ft_small_meta(a, sc, fb.T, bias->qm_out, bias->vb_out, L, s);
        if (pb) return launch_ft_small_pb(a, sc, beta_b, L, s);
        return leap ? launch_ft_small(a, L, s) : launch_ft_small_sched(a, sc, L, s);
    }
    double* K = W.scal + (size_t)SC_K * B;
    double* h0 = H0 ? H0 : W.scal + (size_t)SC_H0 * B;
    double* h1 = H1 ? H1 : W.scal + (size_t)SC_H1 * B;
    // per-chain state rows: of x (old), of the proposal (neu), of x_new (sel) -- three in W.scal (slots SC_OLD0.., SC_NEW0..: 3
    // consecutive); with a bias four and V behind them where launch_meta_energy leaves it, in W.vb: the momentum ping-pong field
    // no flowed sequence touches (2 L^2 >= 32 rows of B); with a defect four as well, Dsum the fourth, in the same places
    const bool four = bias || dfa;
    const int nrow = four ? 4 : 3;
    double* old = four ? W.vb : W.scal + (size_t)SC_OLD0 * B;
    double* neu = four ? W.vb + (size_t)5 * B : W.scal + (size_t)SC_NEW0 * B;
    double* sel = state_out ? state_out : (four ? W.vb + (size_t)10 * B : W.scal + (size_t)SC_S * B);
    double* qm_sel = sel + (size_t)3 * B;
    const size_t row = (size_t)B * sizeof(double);
    // V(Q_m) into an end's energy and Q_m into its fourth row: of the field (sums) or of the carried state; no bias: nothing.
    // With a defect: (beta - g_b) Dsum into the energy and Dsum into the fourth row -- launch_defect_energy reads Dsum one row behind
    // the pointer it is given, so the state's own fourth row serves it
    auto add_bias = [&](const double* xphys, double* rows, double* h) {
        if (dfa) {
            if (xphys) {
                FT_TRY(launch_defect_sums(xphys, B, L, beta, dfa->df, nullptr, D.sums, s));
                if (hipMemcpyAsync(rows + (size_t)3 * B, D.sums + B, row, hipMemcpyDeviceToDevice, s) != hipSuccess) return (int)FTHMC_ERR_LAUNCH;
            }
            return launch_defect_energy(rows + (size_t)2 * B, B, beta, dfa->g_b, h, s);
        }
        if (!bias) return (int)FTHMC_OK;
        if (!xphys) return launch_meta_energy_qm(rows + (size_t)3 * B, B, fb.T, h, nullptr, s);
        FT_TRY(launch_meta_sums(xphys, B, L, M.sums, s));
        return launch_meta_energy(M.sums, B, fb.T, h, rows + (size_t)3 * B, s);
    };
    if (four && state_in && hipMemcpyAsync(old + (size_t)3 * B, state_in + (size_t)3 * B, row, hipMemcpyDeviceToDevice, s) != hipSuccess)
        return FTHMC_ERR_LAUNCH;
    const bool tuned = md && C.A.is_default() && nl > 0;
    if (tuned) {
        // tuned kernels: the scalars of either end of the trajectory come from ONE launch each (launch_traj_energy: log det J
        // from the sweep's partials, S_W / Q / plaq of the flowed field, the kinetic term, H), the first drift and the copy of
        // the momenta are one pass, the last kick also writes the regularized end point, the Metropolis kernel hands plaq / Q
        // out itself: 5 small launches per trajectory where there were 15.  A schedule's shifted field lives in the proposal
        // buffer (xshift = xreg = W.xb); the leapfrog has no SHIFT stage and reads no shift buffer.
        const int np = flow_fwd_geom(C.mfma).ntiles(L);
        if (!state_in) FT_TRY(sweep_forward(C, x, W, nl, B, L, act, nullptr, s, false, false, true));
        FT_TRY(launch_traj_energy(phys_field(x, W, nl), B, L, beta, W.lj_part, np, nl, state_in, v, old, h0, s, beta_b));
        FT_TRY(add_bias(state_in ? nullptr : phys_field(x, W, nl), old, h0));
        FT_TRY(ft_md_ws(C, x, v, W, nl, B, L, act, beta, sc, s, W.xb, W.xb, beta_b, fbp, fdp));
        FT_TRY(sweep_forward(C, W.xb, W, nl, B, L, act, nullptr, s, false, false, true));
        FT_TRY(launch_traj_energy(phys_field(W.xb, W, nl), B, L, beta, W.lj_part, np, nl, nullptr, W.va, neu, h1, s, beta_b));
        FT_TRY(add_bias(phys_field(W.xb, W, nl), neu, h1));
    } else {                                                         // other net shapes, no layers, FTHMC_MODE_LITERAL
        double* seff = W.scal + (size_t)SC_SEFF * B;                 // per-chain beta: S_eff beside the beta-free triple
        if (pb) {
            FT_TRY(pb_eval(C, x, W, nl, B, L, act, beta_b, state_in, old, seff, s));
        } else if (state_in) {    // chained trajectories: S_eff and observables of x are the previous call's state_out
            if (hipMemcpyAsync(old, state_in, 3 * row, hipMemcpyDeviceToDevice, s) != hipSuccess) return FTHMC_ERR_LAUNCH;
        } else {
            FT_TRY(eval_action(C, x, W, nl, B, L, act, beta, old, nullptr, old + B, old + 2 * B, s));
        }
        FT_TRY(launch_kinetic(v, B, L, K, s));
        FT_TRY(launch_lincomb(pb ? seff : old, 1.0, K, 0.5, 0.0, h0, B, s));
        FT_TRY(add_bias(state_in ? nullptr : phys_field(x, W, nl), old, h0));
        const double* vend = W.va;
        if (!md) {
            FT_TRY(launch_axpy(x, v, 0.5 * dt, W.xa, W.n2, s));       // ft_hmc.py:187 (Q2)
            FT_TRY(launch_wrap(W.xa, W.xb, W.n2, 0, s));              // wrap (ft_hmc.py:208)
            vend = v;
        } else if (leap && !pb) {                                     // scalar-beta leapfrog: the last kick writes no xreg,
            FT_TRY(ft_md_ws(C, x, v, W, nl, B, L, act, beta, sc, s, nullptr, nullptr, nullptr, fbp, fdp));
            FT_TRY(launch_wrap(W.xa, W.xb, W.n2, 1, s));              // a launch of its own regularizes (ipynb/ft_hmc.py:426)
        } else {                                                      // schedules and per-chain beta: xreg inside the last kick
            FT_TRY(ft_md_ws(C, x, v, W, nl, B, L, act, beta, sc, s, W.xb, W.xb, beta_b, fbp, fdp));
        }
        if (pb) FT_TRY(pb_eval(C, W.xb, W, nl, B, L, act, beta_b, nullptr, neu, seff, s));
        else FT_TRY(eval_action(C, W.xb, W, nl, B, L, act, beta, neu, nullptr, neu + B, neu + 2 * B, s));
        FT_TRY(launch_kinetic(vend, B, L, K, s));
        FT_TRY(launch_lincomb(pb ? seff : neu, 1.0, K, 0.5, 0.0, h1, B, s));
        FT_TRY(add_bias(phys_field(W.xb, W, nl), neu, h1));
    }
    // The state of x_new without another sweep: selected per chain.  Who hands plaq / Q out: the Metropolis kernel both on the
    // tuned branch and with a bias; per-chain beta: Q (the triple's third row) from the kernel on either branch, plaq from the
    // triple's second row and beta_b; the scalar unbiased general branch: two copies out of `sel`.
    const bool both = four || (tuned && !pb);
    FT_TRY(launch_metropolis(x, W.xb, u, h0, h1, B, L, 0, x_new, dH, acc, old, neu, sel, nrow, s, both ? plaq : nullptr,
                             both || pb ? Q : nullptr));
    if (bias) {                                                      // Q_m of x_new: the fourth row; V of it from this call's table
        if (bias->qm_out && hipMemcpyAsync(bias->qm_out, qm_sel, row, hipMemcpyDeviceToDevice, s) != hipSuccess) return FTHMC_ERR_LAUNCH;
        if (bias->vb_out) FT_TRY(launch_meta_energy_qm(qm_sel, B, fb.T, nullptr, bias->vb_out, s));
    } else if (dfa) {                                                // Dsum of x_new: the fourth row
        if (dfa->dsum_out && hipMemcpyAsync(dfa->dsum_out, qm_sel, row, hipMemcpyDeviceToDevice, s) != hipSuccess) return FTHMC_ERR_LAUNCH;
    } else if (pb) {
        if (plaq) FT_TRY(launch_pb_from_state(sel, beta_b, B, L, nl > 0, nullptr, plaq, s));
    } else if (!tuned) {
        if (plaq && hipMemcpyAsync(plaq, sel + B, row, hipMemcpyDeviceToDevice, s) != hipSuccess) return FTHMC_ERR_LAUNCH;
        if (Q && hipMemcpyAsync(Q, sel + 2 * B, row, hipMemcpyDeviceToDevice, s) != hipSuccess) return FTHMC_ERR_LAUNCH;
    }
    return FTHMC_OK;
}

}  // namespace

extern "C" {

#ifndef FTHMC_SRC_SHA
#define FTHMC_SRC_SHA "unknown"
#endif
// "... src <fingerprint>": the kernel sources this library was built from (tools/csrc_sha.py, csrc/Makefile)
#ifdef FT_DRYRUN      // the sanitizer build (make san): launches are no-ops -- the name says so, fthmc_amd/_lib.py refuses to load it as the product
#define FTHMC_BUILD_KIND " DRYRUN (host-side sanitizer build: launches nothing)"
#else
#define FTHMC_BUILD_KIND ""
#endif
const char* fthmc_version(void) { return "fthmc_hip 0.5 (gfx950) src " FTHMC_SRC_SHA FTHMC_BUILD_KIND; }

int fthmc_set_variant(int v) {
    if (v != 0 && v != 1) return FTHMC_ERR_ARG;
    if (const char* e = getenv("FTHMC_LEAP_ROWS")) set_leap_rows(atoi(e) != 0);     // measurement switch, read with the variant
    set_flow_variant(v);
    return FTHMC_OK;
}
int fthmc_get_variant(void) { return get_flow_variant(); }

int fthmc_arch_params(const fthmc_arch_t* arch) {
    Ctx C;
    if (make_ctx(arch, nullptr, &C) != FTHMC_OK) return FTHMC_ERR_UNSUPPORTED;
    return C.A.params();
}

int fthmc_set_small_path(int on) {
    if (on != 0 && on != 1) return FTHMC_ERR_ARG;
    set_small_path(on);
    return FTHMC_OK;
}
int fthmc_get_small_path(void) { return get_small_path(); }

const char* fthmc_last_error(void) { return fthmc::g_last_error; }

const char* fthmc_strerror(int code) {
    switch (code) {
        case FTHMC_OK: return "ok";
        case FTHMC_ERR_ARG: return "bad argument (null pointer or shape; L must be a multiple of 4)";
        case FTHMC_ERR_UNSUPPORTED: return "unsupported configuration";
        case FTHMC_ERR_LAUNCH: return "HIP launch failed";
        case FTHMC_ERR_WS: return "workspace too small (see fthmc_ws_bytes)";
        default: return "unknown error";
    }
}

static size_t ws_bytes_of(const fthmc_arch_t* arch, int B, int L, int n_layers, bool train) {
    Ctx C; Carver c;
    if (B <= 0 || L <= 0 || n_layers < 0 || make_ctx(arch, nullptr, &C) != FTHMC_OK) return 0;
    return ws_layout(C.A, c, B, L, n_layers, train).total * sizeof(double);
}
size_t fthmc_ws_bytes(const fthmc_arch_t* arch, int B, int L, int n_layers) { return ws_bytes_of(arch, B, L, n_layers, false); }
size_t fthmc_train_ws_bytes(const fthmc_arch_t* arch, int B, int L, int n_layers) { return ws_bytes_of(arch, B, L, n_layers, true); }

int fthmc_wrap(const double* x, double* out, size_t n, void* stream) {
    if (!x || !out) return FTHMC_ERR_ARG;
    return launch_wrap(x, out, n, 0, ft_stream(stream));
}
int fthmc_regularize(const double* x, double* out, size_t n, void* stream) {
    if (!x || !out) return FTHMC_ERR_ARG;
    return launch_wrap(x, out, n, 1, ft_stream(stream));
}
int fthmc_plaquettes(const double* x, double* P, int B, int L, void* stream) {
    if (!x || !P || bad_shape(B, L)) return FTHMC_ERR_ARG;
    return launch_plaq(x, P, B, L, ft_stream(stream));
}
int fthmc_wilson_action_charge(const double* x, int B, int L, double beta, double* S, double* Q,
                               double* plaq, void* stream) {
    if (!x || bad_shape(B, L)) return FTHMC_ERR_ARG;
    return launch_action_charge(x, B, L, beta, S, Q, plaq, ft_stream(stream));
}
int fthmc_wilson_force(const double* x, int B, int L, double beta, double* F, void* stream) {
    if (!x || !F || bad_shape(B, L)) return FTHMC_ERR_ARG;
    return launch_wilson_force(x, B, L, beta, F, ft_stream(stream));
}
int fthmc_kinetic(const double* v, int B, int L, double* K, void* stream) {
    if (!v || !K || bad_shape(B, L)) return FTHMC_ERR_ARG;
    return launch_kinetic(v, B, L, K, ft_stream(stream));
}

int fthmc_stats_accumulate(const double* acc, const double* plaq, const double* Q, double* qold, const double* dH, int B,
                           double* vec8, void* stream) {
    if (!acc || !plaq || !Q || !qold || !dH || !vec8 || B <= 0) return FTHMC_ERR_ARG;
    return launch_stats_accumulate(acc, plaq, Q, qold, dH, B, vec8, ft_stream(stream));
}

int fthmc_random_momenta(const int64_t* seeds, int B, int n_per_chain, double* v, double* u, void* stream) {
    // n_per_chain: at most a field of the largest lattice (the launcher and k_random_momenta form (n + 1) / 2 in int)
    if (!seeds || !v || B <= 0 || B > FTHMC_MAX_B || n_per_chain <= 0 || n_per_chain > 2 * FTHMC_MAX_L * FTHMC_MAX_L) return FTHMC_ERR_ARG;
    return launch_random_momenta(seeds, B, n_per_chain, v, u, ft_stream(stream));
}

size_t fthmc_ws_head_bytes(void) { return Carver().up(wint_doubles(0)) * sizeof(double); }

int fthmc_pack_weights(const double* w, const fthmc_arch_t* arch, int n_layers, uint64_t weights_version, void* ws, size_t ws_bytes,
                       void* stream) {
    if (!w || n_layers <= 0) return FTHMC_ERR_ARG;
    Ctx C;
    FT_TRY(open_call(arch, stream, &C));
    Carver c(ws, ws_bytes);
    double* wint = c.take(wint_doubles(n_layers));        // the expansion is the first region of every first-order layout whatever B, L
    FT_TRY(check_ws(c.total(), ws, ws_bytes));
    return use_weights(C, w, n_layers, wint, weights_version);
}

int fthmc_chain_seeds(int64_t seed, int64_t lo, int B, int64_t traj, int64_t* counter, int advance, int64_t* seeds, void* stream) {
    if (!seeds || B <= 0 || (advance && !counter)) return FTHMC_ERR_ARG;
    return launch_chain_seeds(seed, lo, B, traj, counter, advance, seeds, ft_stream(stream));
}

int fthmc_random_uniform(const int64_t* seeds, int B, int n_per_chain, double lo, double hi, double* out, void* stream) {
    if (!seeds || !out || B <= 0 || n_per_chain <= 0 || !(hi > lo)) return FTHMC_ERR_ARG;
    return launch_random_uniform(seeds, B, n_per_chain, lo, hi, out, ft_stream(stream));
}

int fthmc_train_metrics(const double* xi, const double* x, const double* logq, const double* logp, int B, int L,
                        double beta, double dkl_factor, double* row, void* ws, size_t ws_bytes, void* stream) {
    if (!xi || !x || !logq || !logp || !row || bad_shape(B, L) || !(beta != 0.0)) return FTHMC_ERR_ARG;
    Ctx C; WS W; FT_TRY(open_call(nullptr, stream, &C));
    FT_TRY(open_ws(C, ws, ws_bytes, B, L, 0, false, &W));
    const hipStream_t s = C.s;
    double* q = W.scal + (size_t)SC_Q * B; double* qi = W.scal + (size_t)SC_OLD0 * B;
    FT_TRY(launch_action_charge(x, B, L, beta, nullptr, q, nullptr, s, W.act_part));
    FT_TRY(launch_action_charge(xi, B, L, beta, nullptr, qi, nullptr, s, W.act_part));
    return launch_train_metrics(logq, logp, q, qi, B, 1.0 / (beta * L * L), dkl_factor, row, s);
}

int fthmc_adam_step(double* w, const double* gw, double* exp_avg, double* exp_avg_sq, double* hyper, size_t n,
                    double beta1, double beta2, double eps, double weight_decay, int decoupled, void* stream) {
    if (!w || !gw || !exp_avg || !exp_avg_sq || !hyper || n == 0) return FTHMC_ERR_ARG;
    if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0)) return FTHMC_ERR_ARG;
    return launch_adam(w, gw, exp_avg, exp_avg_sq, hyper, n, beta1, beta2, eps, weight_decay, decoupled != 0, ft_stream(stream));
}

int fthmc_leapfrog(const double* x, const double* p, int B, int L, double beta, double dt, int nstep,
                   double* x_out, double* p_out, void* ws, size_t ws_bytes, void* stream) {
    return md_call(true, x, p, nullptr, nullptr, 0, B, L, 0, beta, dt, nstep, FTHMC_INT_LEAPFROG, x_out, p_out, ws, ws_bytes, stream, 0);
}

int fthmc_hmc_trajectory(const double* x, const double* v, const double* u, int B, int L, double beta,
                         double dt, int nstep, double* x_new, double* dH, double* acc, double* H0,
                         double* H1, void* ws, size_t ws_bytes, void* stream) {
    return hmc_trajectory_call(x, v, u, B, L, beta, nullptr, dt, nstep, FTHMC_INT_LEAPFROG, nullptr, x_new, dH, acc, H0, H1, ws, ws_bytes, stream);
}

int fthmc_integrator_forces(int integrator, int nstep) { return integrator_forces(integrator, nstep); }

int fthmc_integrator_schedule(int integrator, double dt, int nstep, double* b0, int* kind, double* a, double* b, int cap) {
    return expand_sched(integrator, dt, nstep, b0, kind, a, b, cap);
}

int fthmc_md(const double* x, const double* p, int B, int L, double beta, double dt, int nstep, int integrator,
             double* x_out, double* p_out, void* ws, size_t ws_bytes, void* stream) {
    return md_call(true, x, p, nullptr, nullptr, 0, B, L, 0, beta, dt, nstep, integrator, x_out, p_out, ws, ws_bytes, stream, 0);
}

int fthmc_hmc_trajectory_int(const double* x, const double* v, const double* u, int B, int L, double beta, double dt, int nstep,
                             int integrator, double* x_new, double* dH, double* acc, double* H0, double* H1,
                             void* ws, size_t ws_bytes, void* stream) {
    return hmc_trajectory_call(x, v, u, B, L, beta, nullptr, dt, nstep, integrator, nullptr, x_new, dH, acc, H0, H1, ws, ws_bytes, stream);
}

int fthmc_flow_layer_fwd(const double* x, const double* w, const fthmc_arch_t* arch, int B, int L, int mu, int off, int act,
                         double* y, double* logJ, void* ws, size_t ws_bytes, void* stream) {
    FT_TRY(check_layer_call(x && w && y, B, L, mu, off, act));
    Ctx C; WS W; FT_TRY(open_flow_call(arch, stream, ws, ws_bytes, w, 1, B, L, false, 0, &C, &W));
    FlowLayerArgs a(W.wint, B, L, mu, off, act);
    a.x = x; a.y = y;
    a.inplace = y == x && layer_inplace(C, L, act);
    return layer_forward(C, W, 0, a, false, logJ);
}

int fthmc_flow_layer_rev(const double* y, const double* w, const fthmc_arch_t* arch, int B, int L, int mu, int off, int act,
                         double tol, double* x, double* logJ, void* ws, size_t ws_bytes, void* stream) {
    FT_TRY(check_layer_call(y && w && x, B, L, mu, off, act));
    Ctx C; WS W; FT_TRY(open_flow_call(arch, stream, ws, ws_bytes, w, 1, B, L, false, 0, &C, &W));
    FlowLayerArgs a(W.wint, B, L, mu, off, act);
    a.x = y; a.y = x; a.tol = tol;
    return layer_forward(C, W, 0, a, true, logJ);
}

// plaquette-level map: the coupling kernel with the plaquette field as input and output (MFMA kernels only)
static int plaq_coupling(const double* P, const double* w, const fthmc_arch_t* arch, int B, int L, int mu, int off, int act, double tol,
                         bool rev, double* out, double* logJ, void* ws, size_t ws_bytes, void* stream) {
    FT_TRY(check_layer_call(P && w && out, B, L, mu, off, act));
    Ctx C; WS W; FT_TRY(open_call(arch, stream, &C));
    if (!C.mfma && C.A.is_default()) return FTHMC_ERR_UNSUPPORTED;
    FT_TRY(open_ws(C, ws, ws_bytes, B, L, 1, false, &W));
    FT_TRY(use_weights(C, w, 1, W.wint));
    FlowLayerArgs a(W.wint, B, L, mu, off, act);
    a.x = P; a.pin = P; a.pout = out; a.tol = tol;
    return layer_forward(C, W, 0, a, rev, logJ);
}

int fthmc_plaq_coupling_fwd(const double* P, const double* w, const fthmc_arch_t* arch, int B, int L, int mu, int off, int act,
                            double* fP, double* logJ, void* ws, size_t ws_bytes, void* stream) {
    return plaq_coupling(P, w, arch, B, L, mu, off, act, 0.0, false, fP, logJ, ws, ws_bytes, stream);
}

int fthmc_plaq_coupling_rev(const double* fP, const double* w, const fthmc_arch_t* arch, int B, int L, int mu, int off, int act,
                            double tol, double* P, double* logJ, void* ws, size_t ws_bytes, void* stream) {
    return plaq_coupling(fP, w, arch, B, L, mu, off, act, tol, true, P, logJ, ws, ws_bytes, stream);
}

// VJP of the plaquette-level map fP = NCPPlaqCouplingLayer.forward(P) (layers.py:348-371): gP = d/dP [sum gfP fP + sum_b glogJ logJ],
// gw (optional) the same wrt the weights.  fP = P + delta at the active sites and P elsewhere, so
//     gP = gfP + (the link-level layer's plaquette gradient for the upstream link gradient gy[mu] = +-gfP),
// i.e. the link-level backward kernels serve it unchanged: the upstream gradient is dressed as that link field
// (launch_plane_from), the forward runs on the plaquette field itself (FlowLayerArgs::pin), gP = W.gp + gfP.
int fthmc_plaq_coupling_bwd(const double* P, const double* w, const fthmc_arch_t* arch, const double* gfP, const double* glogJ,
                            int B, int L, int mu, int off, int act, double* gP, double* gw, void* ws, size_t ws_bytes, void* stream) {
    FT_TRY(check_layer_call(P && w && gfP && glogJ && gP, B, L, mu, off, act));
    Ctx C; WS W; FT_TRY(open_call(arch, stream, &C));
    if (!C.mfma && C.A.is_default()) return FTHMC_ERR_UNSUPPORTED;          // as fthmc_plaq_coupling_fwd: MFMA kernels (or the plain ones)
    FT_TRY(open_ws(C, ws, ws_bytes, B, L, 1, gw != nullptr, &W));
    FT_TRY(use_weights(C, w, 1, W.wint));
    double* fake = W.xa;                                                     // [B][2][L][L]: only plane mu is read
    FT_TRY(launch_plane_from(gfP, B, L, mu, mu == 0 ? 1.0 : -1.0, fake, C.s));
    FlowLayerArgs a(W.wint, B, L, mu, off, act);
    a.x = P; a.pin = P; a.up_link = fake; a.glogj = glogJ;
    FT_TRY(layer_vjp(C, W, a, nullptr, gw));
    return launch_axpy(W.gp, gfP, 1.0, gP, (size_t)B * L * L, C.s);
}

// VJP of one layer.  `stash` != null: the forward's activation stash (fthmc_flow_layer_fwd_stash) -- nothing is recomputed;
// else the layer is run forward first from `x`.
static int layer_bwd_impl(const double* x, const double* stash, const double* w, const fthmc_arch_t* arch, const double* gy, const double* glogJ,
                          int B, int L, int mu, int off, int act, double* gx, double* gw, void* ws, size_t ws_bytes, void* stream) {
    FT_TRY(check_layer_call((x || stash) && w && gy && glogJ && gx, B, L, mu, off, act));
    Ctx C; WS W; FT_TRY(open_call(arch, stream, &C));
    const bool mfma = C.mfma;
    if (stash && !mfma && C.A.is_default()) return FTHMC_ERR_UNSUPPORTED;      // the VALU variant has no stash
    FT_TRY(open_ws(C, ws, ws_bytes, B, L, 1, gw != nullptr && mfma, &W));
    FT_TRY(use_weights(C, w, 1, W.wint));
    const hipStream_t s = C.s;
    FlowLayerArgs a(W.wint, B, L, mu, off, act);
    a.x = x; a.up_link = gy; a.glogj = glogJ;
    a.gp_part = W.gp_part; a.gw_part = W.gw_part;
    if (C.gen() || mfma) {                                        // the plain kernels, or the gather-form backward on a stash
        FT_TRY(layer_vjp(C, W, a, stash, gw));
        return launch_adj_add(W.gp, gy, B, L, gx, s);
    }
    FT_TRY(launch_flow_bwd(a, gw != nullptr, s));                 // VALU variant: scatter form + gather
    if (gw) FT_TRY(launch_reduce_gw(W.gw_part, B * flow_geom(false).ntiles(L), 1.0, 0, gw, W.gw_tmp, s));
    FT_TRY(launch_gather_gp(W.gp_part, B, L, flow_geom(false), 0, W.gp, s));
    return launch_adj_add(W.gp, gy, B, L, gx, s);
}

int fthmc_flow_layer_bwd(const double* x, const double* w, const fthmc_arch_t* arch, const double* gy, const double* glogJ,
                         int B, int L, int mu, int off, int act, double* gx, double* gw, void* ws,
                         size_t ws_bytes, void* stream) {
    if (!x) return FTHMC_ERR_ARG;
    return layer_bwd_impl(x, nullptr, w, arch, gy, glogJ, B, L, mu, off, act, gx, gw, ws, ws_bytes, stream);
}

size_t fthmc_layer_stash_bytes(const fthmc_arch_t* arch, int B, int L) {
    Ctx C;
    if (B <= 0 || L <= 0 || make_ctx(arch, nullptr, &C) != FTHMC_OK) return 0;
    if (C.gen()) return C.A.stash_doubles(B, L) * sizeof(double);
    return C.mfma ? flow_stash_doubles(B, L, true) * sizeof(double) : 0;
}

int fthmc_flow_layer_fwd_stash(const double* x, const double* w, const fthmc_arch_t* arch, int B, int L, int mu, int off, int act, double* y,
                               double* logJ, double* stash, void* ws, size_t ws_bytes, void* stream) {
    FT_TRY(check_layer_call(x && w && y && stash, B, L, mu, off, act));
    if (fthmc_layer_stash_bytes(arch, B, L) == 0) return FTHMC_ERR_UNSUPPORTED;        // the VALU variant has no stash
    Ctx C; WS W; FT_TRY(open_flow_call(arch, stream, ws, ws_bytes, w, 1, B, L, false, 0, &C, &W));
    FlowLayerArgs a(W.wint, B, L, mu, off, act);
    a.x = x; a.y = y; a.stash = stash; a.stash_h = 1;
    a.inplace = y == x && layer_inplace(C, L, act);
    return layer_forward(C, W, 0, a, false, logJ);
}

int fthmc_flow_layer_bwd_stash(const double* stash, const double* w, const fthmc_arch_t* arch, const double* gy, const double* glogJ, int B, int L,
                               int mu, int off, int act, double* gx, double* gw, void* ws, size_t ws_bytes, void* stream) {
    if (!stash) return FTHMC_ERR_ARG;
    return layer_bwd_impl(nullptr, stash, w, arch, gy, glogJ, B, L, mu, off, act, gx, gw, ws, ws_bytes, stream);
}

int fthmc_flow_forward_v(const double* x, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L, int act,
                       double* y, double* logdet, void* ws, size_t ws_bytes, void* stream, uint64_t weights_version) {
    FT_TRY(check_flow_call(x != nullptr, w, n_layers, B, L, act));
    Ctx C; WS W; FT_TRY(open_flow_call(arch, stream, ws, ws_bytes, w, n_layers, B, L, false, weights_version, &C, &W));
    const hipStream_t s = C.s;
    double* ld = logdet ? logdet : W.scal + (size_t)SC_LOGDET * B;
    if (n_layers == 0 && hipMemsetAsync(ld, 0, (size_t)B * sizeof(double), s) != hipSuccess) return FTHMC_ERR_LAUNCH;
    if (C.small(L, n_layers)) {
        SmallArgs a = small_args(x, W, n_layers, B, act, 1.0, 0);
        a.x_out = y; a.logdet = ld;
        return launch_ft_small(a, L, s);
    }
    FT_TRY(sweep_forward(C, x, W, n_layers, B, L, act, ld, s));
    if (y && hipMemcpyAsync(y, phys_field(x, W, n_layers), W.n2 * sizeof(double),
                            hipMemcpyDeviceToDevice, s) != hipSuccess) return FTHMC_ERR_LAUNCH;
    return FTHMC_OK;
}

int fthmc_flow_forward(const double* x, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L, int act,
                       double* y, double* logdet, void* ws, size_t ws_bytes, void* stream) {
    return fthmc_flow_forward_v(x, w, arch, n_layers, B, L, act, y, logdet, ws, ws_bytes, stream, 0);
}

int fthmc_flow_reverse_v(const double* y, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L, int act, double tol,
                       double* x, double* logdet, void* ws, size_t ws_bytes, void* stream, uint64_t weights_version) {
    FT_TRY(check_flow_call(y && x, w, n_layers, B, L, act));
    Ctx C; WS W; FT_TRY(open_flow_call(arch, stream, ws, ws_bytes, w, n_layers, B, L, false, weights_version, &C, &W));
    const hipStream_t s = C.s;
    double* ld = logdet ? logdet : W.scal + (size_t)SC_LOGDET * B;
    if (hipMemsetAsync(ld, 0, (size_t)B * sizeof(double), s) != hipSuccess) return FTHMC_ERR_LAUNCH;
    // The last layer maps y -> x, the others run in place on x.  In place is safe: a layer only rewrites its ACTIVE links,
    // every plaquette the kernel USES (the frozen ones of its window, the active ones of its own tile) is built from
    // links the layer never writes plus the workgroup's own active links, which it loads before it stores them; the
    // active / passive plaquettes of the halo, which a neighbour's update can tear, are never read.
    const double* src = y;
    for (int l = n_layers - 1; l >= 0; --l) {
        FlowLayerArgs a(W.wint, l, B, L, act);
        a.x = src; a.y = x; a.tol = tol;
        FT_TRY(layer_forward(C, W, l, a, true, ld, 1));
        src = x;
    }
    if (n_layers == 0 && x != y && hipMemcpyAsync(x, y, W.n2 * sizeof(double), hipMemcpyDeviceToDevice, s) != hipSuccess)
        return FTHMC_ERR_LAUNCH;
    return FTHMC_OK;
}

int fthmc_flow_reverse(const double* y, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L, int act, double tol,
                       double* x, double* logdet, void* ws, size_t ws_bytes, void* stream) {
    return fthmc_flow_reverse_v(y, w, arch, n_layers, B, L, act, tol, x, logdet, ws, ws_bytes, stream, 0);
}

int fthmc_ft_action_v(const double* x, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L, int act, double beta,
                    double* S_eff, double* logdet, double* plaq, double* Q, void* ws, size_t ws_bytes,
                    void* stream, uint64_t weights_version) {
    FT_TRY(check_flow_call(x != nullptr, w, n_layers, B, L, act));
    Ctx C; WS W; FT_TRY(open_flow_call(arch, stream, ws, ws_bytes, w, n_layers, B, L, false, weights_version, &C, &W));
    const hipStream_t s = C.s;
    if (n_layers == 0 && logdet && hipMemsetAsync(logdet, 0, (size_t)B * sizeof(double), s) != hipSuccess) return FTHMC_ERR_LAUNCH;
    if (C.small(L, n_layers)) {
        SmallArgs a = small_args(x, W, n_layers, B, act, beta, 0);
        a.S_eff = S_eff; a.logdet = logdet; a.plaq = plaq; a.Q = Q;
        return launch_ft_small(a, L, s);
    }
    return eval_action(C, x, W, n_layers, B, L, act, beta, S_eff, logdet, plaq, Q, s);
}

int fthmc_ft_action(const double* x, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L, int act, double beta,
                    double* S_eff, double* logdet, double* plaq, double* Q, void* ws, size_t ws_bytes,
                    void* stream) {
    return fthmc_ft_action_v(x, w, arch, n_layers, B, L, act, beta, S_eff, logdet, plaq, Q, ws, ws_bytes, stream, 0);
}

int fthmc_ft_force_v(const double* x, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L, int act, double beta,
                   double* F, void* ws, size_t ws_bytes, void* stream, uint64_t weights_version) {
    FT_TRY(check_flow_call(x && F, w, n_layers, B, L, act));
    Ctx C; WS W; FT_TRY(open_flow_call(arch, stream, ws, ws_bytes, w, n_layers, B, L, false, weights_version, &C, &W));
    const hipStream_t s = C.s;
    if (C.small(L, n_layers)) {
        SmallArgs a = small_args(x, W, n_layers, B, act, beta, 1);
        a.F = F;
        return launch_ft_small(a, L, s);
    }
    FT_TRY(force_gp(C, x, W, n_layers, B, L, act, beta, -1.0, nullptr, s));
    return launch_kick_from_gp(W.gp, nullptr, nullptr, F, B, L, 0.0, 0.0, s);
}

int fthmc_ft_force(const double* x, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L, int act, double beta,
                   double* F, void* ws, size_t ws_bytes, void* stream) {
    return fthmc_ft_force_v(x, w, arch, n_layers, B, L, act, beta, F, ws, ws_bytes, stream, 0);
}

int fthmc_ft_leapfrog_v(const double* x, const double* v, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L,
                      int act, double beta, double dt, int nstep, double* x_out, double* v_out,
                      void* ws, size_t ws_bytes, void* stream, uint64_t weights_version) {
    return md_call(false, x, v, w, arch, n_layers, B, L, act, beta, dt, nstep, FTHMC_INT_LEAPFROG, x_out, v_out, ws, ws_bytes, stream,
                   weights_version);
}

int fthmc_ft_leapfrog(const double* x, const double* v, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L,
                      int act, double beta, double dt, int nstep, double* x_out, double* v_out,
                      void* ws, size_t ws_bytes, void* stream) {
    return fthmc_ft_leapfrog_v(x, v, w, arch, n_layers, B, L, act, beta, dt, nstep, x_out, v_out, ws, ws_bytes, stream, 0);
}

int fthmc_ft_trajectory_v(const double* x, const double* v, const double* u, const double* w, const fthmc_arch_t* arch, int n_layers,
                        int B, int L, int act, double beta, double dt, int nstep, int mode, double* x_new,
                        double* dH, double* acc, double* H0, double* H1, double* plaq, double* Q,
                        const double* state_in, double* state_out,
                        void* ws, size_t ws_bytes, void* stream, uint64_t weights_version) {
    return ft_trajectory_call(x, v, u, w, arch, n_layers, B, L, act, beta, nullptr, dt, nstep, FTHMC_INT_LEAPFROG, mode, nullptr, x_new, dH, acc,
                              H0, H1, plaq, Q, state_in, state_out, ws, ws_bytes, stream, weights_version);
}

int fthmc_ft_md_v(const double* x, const double* v, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L,
                  int act, double beta, double dt, int nstep, double* x_out, double* v_out,
                  void* ws, size_t ws_bytes, void* stream, int integrator, uint64_t weights_version) {
    return md_call(false, x, v, w, arch, n_layers, B, L, act, beta, dt, nstep, integrator, x_out, v_out, ws, ws_bytes, stream,
                   weights_version);
}

int fthmc_ft_trajectory_int_v(const double* x, const double* v, const double* u, const double* w, const fthmc_arch_t* arch, int n_layers,
                              int B, int L, int act, double beta, double dt, int nstep, int mode, double* x_new,
                              double* dH, double* acc, double* H0, double* H1, double* plaq, double* Q,
                              const double* state_in, double* state_out,
                              void* ws, size_t ws_bytes, void* stream, int integrator, uint64_t weights_version) {
    return ft_trajectory_call(x, v, u, w, arch, n_layers, B, L, act, beta, nullptr, dt, nstep, integrator, mode, nullptr, x_new, dH, acc,
                              H0, H1, plaq, Q, state_in, state_out, ws, ws_bytes, stream, weights_version);
}

// per-chain beta (replica exchange): a null beta_b would mean "scalar beta" to the sequencers, so it is refused here
int fthmc_ft_trajectory_pb_v(const double* x, const double* v, const double* u, const double* w, const fthmc_arch_t* arch, int n_layers,
                             int B, int L, int act, const double* beta_b, double dt, int nstep, int mode, double* x_new,
                             double* dH, double* acc, double* H0, double* H1, double* plaq, double* Q,
                             const double* state_in, double* state_out,
                             void* ws, size_t ws_bytes, void* stream, int integrator, uint64_t weights_version) {
    if (!beta_b) return FTHMC_ERR_ARG;
    return ft_trajectory_call(x, v, u, w, arch, n_layers, B, L, act, 0.0, beta_b, dt, nstep, integrator, mode, nullptr, x_new, dH, acc,
                              H0, H1, plaq, Q, state_in, state_out, ws, ws_bytes, stream, weights_version);
}

int fthmc_hmc_trajectory_pb(const double* x, const double* v, const double* u, int B, int L, const double* beta_b, double dt, int nstep,
                            int integrator, double* x_new, double* dH, double* acc, double* H0, double* H1,
                            void* ws, size_t ws_bytes, void* stream) {
    if (!beta_b) return FTHMC_ERR_ARG;
    return hmc_trajectory_call(x, v, u, B, L, 0.0, beta_b, dt, nstep, integrator, nullptr, x_new, dH, acc, H0, H1, ws, ws_bytes, stream);
}

int fthmc_replica_swap(const double* betas, int K, int M, int parity, const double* C, const double* u, double* beta_b, int32_t* rung,
                       int32_t* chain_of, double* swap_acc, double* d, void* stream) {
    if (K < 2 || M < 1 || (long long)K * M > FTHMC_MAX_B || (parity != 0 && parity != 1) || !betas || !C || !u || !beta_b || !rung ||
        !chain_of)
        return FTHMC_ERR_ARG;
    return launch_replica_swap(betas, K, M, parity, C, u, beta_b, rung, chain_of, swap_acc, d, ft_stream(stream));
}

int fthmc_ladder_init(const double* betas_host, int K, int M, double* betas, double* beta_b, int32_t* rung, int32_t* chain_of,
                      void* stream) {
    if (K < 2 || M < 1 || (long long)K * M > FTHMC_MAX_B || !betas_host || !betas || !beta_b || !rung || !chain_of) return FTHMC_ERR_ARG;
    for (int k = 0; k + 1 < K; ++k) if (!(betas_host[k] < betas_host[k + 1])) return FTHMC_ERR_ARG;      // strictly increasing (NaN refused)
    return launch_ladder_init(betas_host, betas, K, M, beta_b, rung, chain_of, ft_stream(stream));
}

// Wilson loops (loops.hip): the argument checks and the three regions of the workspace; the kernels know nothing of `ws`
size_t fthmc_wilson_loops_ws_bytes(int B, int L, int Rmax, int Tmax) {
    if (bad_shape(B, L) || Rmax < 1 || Rmax > L || Tmax < 1 || Tmax > L) return 0;
    const LoopsGeom g = loops_geom(B, L, Rmax, Tmax);
    return g.ok ? g.total * sizeof(double) : 0;
}

int fthmc_wilson_loops(const double* x, int B, int L, int Rmax, int Tmax, double* W, double* Wmean, void* ws, size_t ws_bytes,
                       void* stream) {
    if (!x || !W || bad_shape(B, L) || Rmax < 1 || Rmax > L || Tmax < 1 || Tmax > L) return FTHMC_ERR_ARG;
    const LoopsGeom g = loops_geom(B, L, Rmax, Tmax);
    if (!g.ok || !ws || ws_bytes / sizeof(double) < g.total) return FTHMC_ERR_WS;
    double* prefix = static_cast<double*>(ws);
    return launch_wilson_loops(x, B, L, Rmax, Tmax, W, Wmean, prefix, prefix + g.prefix, prefix + g.prefix + g.part, ft_stream(stream));
}

// Heatbath / overrelaxation sweeps (local.hip): the argument checks and the choice of the path; no workspace
int fthmc_local_update(const double* x, int B, int L, double beta, const double* beta_b, const int64_t* seeds, int n_hb, int n_or,
                       int nsweep, int64_t sweep0, int classes, double* x_out, void* stream) {
    if (!x || !x_out || bad_shape(B, L) || n_hb < 0 || n_or < 0 || nsweep < 0 || sweep0 < 0 || classes < 1 || classes > 15) return FTHMC_ERR_ARG;
    if (n_hb > 0 && !seeds) return FTHMC_ERR_ARG;                                       // overrelaxation draws nothing
    // the heatbath-sweep index is one 32-bit word of the Philox counter: every index the call uses must fit
    const long long last = (long long)nsweep * (long long)n_hb;                         // < 2^62
    if (sweep0 > (1LL << 32) || last > (1LL << 32) - sweep0) return FTHMC_ERR_ARG;
    const bool resident = L <= LU_MAXL && get_small_path() != 0;
    return launch_local_update(x, B, L, beta, beta_b, seeds, n_hb, n_or, nsweep, (uint32_t)sweep0, classes, x_out, resident, ft_stream(stream));
}

// Annealing (local.hip): the argument checks and the choice of the path; no workspace
int fthmc_anneal(const double* x, int B, int L, const double* betas, int n_step, const int64_t* seeds, int n_hb, int n_or, int nsweep,
                 int64_t sweep0, int path, const double* work_in, double* x_out, double* work_out, double* c_trace, void* stream) {
    if (!x || !x_out || !betas || !work_out || bad_shape(B, L) || n_step < 0 || n_step > AN_MAX_STEPS || n_hb < 0 || n_or < 0 || nsweep < 0 ||
        sweep0 < 0 || path < 0 || path > 2)
        return FTHMC_ERR_ARG;
    if (n_hb > 0 && !seeds) return FTHMC_ERR_ARG;                                       // overrelaxation draws nothing
    if (n_step > 0 && n_hb + n_or == 0) return FTHMC_ERR_ARG;                           // a step that moves no link
    if (path == 1 && L > LU_MAXL) return FTHMC_ERR_ARG;
    // the heatbath-sweep index is one 32-bit word of the Philox counter: every index the ramp uses must fit
    const long long per = (long long)nsweep * (long long)n_hb;                          // < 2^62
    if (sweep0 > (1LL << 32) || (n_step > 0 && per > ((1LL << 32) - sweep0) / n_step)) return FTHMC_ERR_ARG;
    const bool resident = path == 1 || (path == 0 && L <= LU_MAXL && get_small_path() != 0);
    return launch_anneal(x, B, L, betas, n_step, seeds, n_hb, n_or, nsweep, (uint32_t)sweep0, work_in, x_out, work_out, c_trace, resident,
                         ft_stream(stream));
}

// Instanton hits (topo.hip): the argument checks, the choice of the launch shape and the workspace of the split one:
// part[B][nw][2] doubles | k[B] int32
static bool instanton_split(int B, int L, int path) { return path == 2 || (path == 0 && B < 64 && L >= 128); }
size_t fthmc_instanton_ws_bytes(int B, int L, int path) {
    if (bad_shape(B, L) || path < 0 || path > 2 || !instanton_split(B, L, path)) return 0;
    // rounded like every other workspace size (a multiple of 256 bytes), so that a caller may carve one allocation into workspaces
    return Carver().up(instanton_part_doubles(B, L) + ((size_t)B * sizeof(int32_t) + 7) / 8) * sizeof(double);
}
int fthmc_instanton_hit(const double* x, int B, int L, double beta, const double* beta_b, const int64_t* seeds, int n_hit, int64_t hit0,
                        int path, double* x_out, int32_t* k_out, int32_t* nacc_out, double* cs_out, void* ws, size_t ws_bytes, void* stream) {
    if (!x || !x_out || bad_shape(B, L) || n_hit < 0 || n_hit > IT_MAX_HITS || path < 0 || path > 2) return FTHMC_ERR_ARG;
    if (n_hit > 0 && !seeds) return FTHMC_ERR_ARG;                                       // no hit draws nothing
    // the hit index is one 32-bit word of the Philox counter: every index the call uses must fit
    if (hit0 < 0 || hit0 > (1LL << 32) - n_hit) return FTHMC_ERR_ARG;
    const bool split = instanton_split(B, L, path);
    double* part = nullptr;
    int32_t* kbuf = nullptr;
    if (split) {
        if (!ws || ws_bytes < fthmc_instanton_ws_bytes(B, L, path)) return FTHMC_ERR_WS;
        part = static_cast<double*>(ws);
        kbuf = reinterpret_cast<int32_t*>(part + instanton_part_doubles(B, L));
    }
    return launch_instanton(x, B, L, beta, beta_b, seeds, n_hit, (uint32_t)hit0, split, x_out, k_out, nacc_out, cs_out, part, kbuf,
                            ft_stream(stream));
}

// Metadynamics HMC (meta.hip): the argument checks; the choice of the path and the workspace of the sequenced one are hmc_trajectory_call's
size_t fthmc_meta_ws_bytes(int B, int L, int path) {
    if (bad_shape(B, L) || path < 0 || path > 2 || path == 1) return 0;             // the one-launch path needs none
    if (B > META_SEQ_MAX_B) return 0;                                               // the sequenced path does not serve it
    Carver c;
    return meta_layout(flow_arch_default(), c, B, L, 0, true).total * sizeof(double);
}
int fthmc_meta_trajectory(const double* x, const double* v, const double* u, int B, int L, double beta, double dt, int nstep, int integrator,
                          const double* vtab, int G, int nb, double qmax, double wall, int path, double* x_new, double* dH, double* acc,
                          double* H0, double* H1, double* qm_out, double* vb_out, void* ws, size_t ws_bytes, void* stream) {
    BiasArg bias{{}, path, qm_out, vb_out};
    if (meta_tab(vtab, B, G, nb, qmax, wall, &bias.T) != FTHMC_OK || path < 0 || path > 2) return FTHMC_ERR_ARG;
    if (path == 1 && (L > HMC_RESIDENT_MAXL || x_new == x)) return FTHMC_ERR_ARG;
    return hmc_trajectory_call(x, v, u, B, L, beta, nullptr, dt, nstep, integrator, &bias, x_new, dH, acc, H0, H1, ws, ws_bytes, stream);
}
int fthmc_meta_deposit(const double* qm, int B, int G, int nb, double qmax, double w, double* vtab, void* stream) {
    MetaTab T;
    if (!qm || B <= 0 || B > FTHMC_MAX_B || meta_tab(vtab, B, G, nb, qmax, w, &T) != FTHMC_OK) return FTHMC_ERR_ARG;
    return launch_meta_deposit(qm, B, G, nb, qmax, w, vtab, ft_stream(stream));
}
int fthmc_meta_force(const double* x, int B, int L, double beta, const double* vtab, int G, int nb, double qmax, double wall, double* F,
                     void* stream) {
    MetaTab T;
    if (!x || !F || bad_shape(B, L) || meta_tab(vtab, B, G, nb, qmax, wall, &T) != FTHMC_OK) return FTHMC_ERR_ARG;
    return launch_meta_force(x, B, L, beta, T, F, ft_stream(stream));
}
int fthmc_meta_action(const double* x, int B, int L, double beta, const double* vtab, int G, int nb, double qmax, double wall, double* S,
                      double* qm, double* vb, void* stream) {
    MetaTab T;
    if (!x || bad_shape(B, L) || meta_tab(vtab, B, G, nb, qmax, wall, &T) != FTHMC_OK) return FTHMC_ERR_ARG;
    return launch_meta_action(x, B, L, beta, T, S, qm, vb, ft_stream(stream));
}

// Boundary-condition tempering (defect.hip): the argument checks; the choice of the path and the workspace of the sequenced
// one are defect_trajectory_call's
size_t fthmc_defect_ws_bytes(int B, int L, int path) {
    if (bad_shape(B, L) || path < 0 || path > 2 || path == 1) return 0;             // the one-launch path needs none
    if (B > META_SEQ_MAX_B) return 0;                                               // the sequenced path does not serve it
    Carver c;
    return defect_layout(c, B, L).total * sizeof(double);
}
int fthmc_defect_trajectory(const double* x, const double* v, const double* u, int B, int L, double beta, const double* g_b, int i0, int j0,
                            int Ld, double dt, int nstep, int integrator, int path, double* x_new, double* dH, double* acc, double* H0,
                            double* H1, double* csum_out, double* dsum_out, double* q_out, void* ws, size_t ws_bytes, void* stream) {
    if (!x || !v || !u || !x_new || bad_shape(B, L) || nstep < 1 || bad_defect(L, beta, g_b, i0, j0, Ld) || path < 0 || path > 2)
        return FTHMC_ERR_ARG;
    if (path == 1 && (L > HMC_RESIDENT_MAXL || x_new == x)) return FTHMC_ERR_ARG;
    return defect_trajectory_call(x, v, u, B, L, beta, g_b, DefectLine{i0, j0, Ld}, dt, nstep, integrator, path, x_new, dH, acc, H0, H1,
                                  csum_out, dsum_out, q_out, ws, ws_bytes, stream);
}
int fthmc_defect_force(const double* x, int B, int L, double beta, const double* g_b, int i0, int j0, int Ld, double* F, void* stream) {
    if (!x || !F || bad_shape(B, L) || bad_defect(L, beta, g_b, i0, j0, Ld)) return FTHMC_ERR_ARG;
    return launch_defect_force(x, B, L, beta, g_b, DefectLine{i0, j0, Ld}, F, ft_stream(stream));
}
int fthmc_defect_action(const double* x, int B, int L, double beta, const double* g_b, int i0, int j0, int Ld, double* S, double* csum,
                        double* dsum, double* Q, void* stream) {
    if (!x || bad_shape(B, L) || bad_defect(L, beta, g_b, i0, j0, Ld)) return FTHMC_ERR_ARG;
    return launch_defect_action(x, B, L, beta, g_b, DefectLine{i0, j0, Ld}, S, csum, dsum, Q, ft_stream(stream));
}
int fthmc_defect_translate(const double* x, int B, int L, const int32_t* rung, int top, const int32_t* shift, double* x_out, void* stream) {
    if (!x || !x_out || x_out == x || !rung || !shift || bad_shape(B, L)) return FTHMC_ERR_ARG;
    return launch_defect_translate(x, B, L, rung, top, shift, x_out, ft_stream(stream));
}

// Metadynamics through the flow: the checks are check_ft_meta_args', the workspace open_ft_meta_call's
size_t fthmc_ft_meta_ws_bytes(const fthmc_arch_t* arch, int B, int L, int n_layers) {
    Ctx C; Carver c;
    if (B <= 0 || L <= 0 || n_layers < 0 || make_ctx(arch, nullptr, &C) != FTHMC_OK) return 0;
    return meta_layout(C.A, c, B, L, n_layers, false).total * sizeof(double);
}
int fthmc_ft_meta_trajectory_v(const double* x, const double* v, const double* u, const double* w, const fthmc_arch_t* arch, int n_layers,
                               int B, int L, int act, double beta, double dt, int nstep, int integrator, const double* vtab, int G,
                               int nb, double qmax, double wall, double* x_new, double* dH, double* acc, double* H0, double* H1,
                               double* plaq, double* Q, double* qm_out, double* vb_out, const double* state_in, double* state_out,
                               void* ws, size_t ws_bytes, void* stream, uint64_t weights_version) {
    BiasArg bias{{}, 0, qm_out, vb_out};
    FT_TRY(check_ft_meta_args(x && v && u && x_new && nstep >= 1, w, n_layers, B, L, act, vtab, G, nb, qmax, wall, &bias.T));
    return ft_trajectory_call(x, v, u, w, arch, n_layers, B, L, act, beta, nullptr, dt, nstep, integrator, FTHMC_MODE_MD, &bias, x_new, dH,
                              acc, H0, H1, plaq, Q, state_in, state_out, ws, ws_bytes, stream, weights_version);
}
int fthmc_ft_meta_force_v(const double* x, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L, int act, double beta,
                          const double* vtab, int G, int nb, double qmax, double wall, double* F, void* ws, size_t ws_bytes,
                          void* stream, uint64_t weights_version) {
    Ctx C; MWS M; FlowBias bias{};
    FT_TRY(check_ft_meta_args(x && F, w, n_layers, B, L, act, vtab, G, nb, qmax, wall, &bias.T));
    FT_TRY(open_ft_meta_call(arch, stream, ws, ws_bytes, w, n_layers, B, L, true, weights_version, &C, &M));
    bias.sums = M.sums;
    FT_TRY(force_gp(C, x, M.W, n_layers, B, L, act, beta, -1.0, nullptr, C.s, false, nullptr, &bias));
    return launch_kick_from_gp(M.W.gp, nullptr, nullptr, F, B, L, 0.0, 0.0, C.s);
}
int fthmc_ft_meta_action_v(const double* x, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L, int act, double beta,
                           const double* vtab, int G, int nb, double qmax, double wall, double* S_b, double* logdet, double* qm,
                           double* vbias, void* ws, size_t ws_bytes, void* stream, uint64_t weights_version) {
    Ctx C; MWS M; MetaTab T;
    FT_TRY(check_ft_meta_args(x != nullptr, w, n_layers, B, L, act, vtab, G, nb, qmax, wall, &T));
    FT_TRY(open_ft_meta_call(arch, stream, ws, ws_bytes, w, n_layers, B, L, true, weights_version, &C, &M));
    const WS& W = M.W;
    const hipStream_t s = C.s;
    const size_t row = (size_t)B * sizeof(double);
    if (n_layers == 0 && logdet && hipMemsetAsync(logdet, 0, row, s) != hipSuccess) return FTHMC_ERR_LAUNCH;
    double* sb = S_b ? S_b : W.vb + (size_t)2 * B;                   // S_eff first, V added in place
    FT_TRY(eval_action(C, x, W, n_layers, B, L, act, beta, sb, logdet, nullptr, nullptr, s));
    FT_TRY(launch_meta_sums(phys_field(x, W, n_layers), B, L, M.sums, s));
    FT_TRY(launch_meta_energy(M.sums, B, T, sb, W.vb, s));          // W.vb: (Q_m, V), [2][B]
    if (qm && hipMemcpyAsync(qm, W.vb, row, hipMemcpyDeviceToDevice, s) != hipSuccess) return FTHMC_ERR_LAUNCH;
    if (vbias && hipMemcpyAsync(vbias, W.vb + B, row, hipMemcpyDeviceToDevice, s) != hipSuccess) return FTHMC_ERR_LAUNCH;
    return FTHMC_OK;
}

// Boundary-condition tempering through the flow: the checks are check_ft_defect_args', the workspace open_ft_defect_call's
size_t fthmc_ft_defect_ws_bytes(const fthmc_arch_t* arch, int B, int L, int n_layers) {
    Ctx C; Carver c;
    if (B <= 0 || L <= 0 || n_layers < 0 || make_ctx(arch, nullptr, &C) != FTHMC_OK) return 0;
    return ft_defect_layout(C.A, c, B, L, n_layers).total * sizeof(double);
}
int fthmc_ft_defect_trajectory_v(const double* x, const double* v, const double* u, const double* w, const fthmc_arch_t* arch, int n_layers,
                                 int B, int L, int act, double beta, const double* g_b, int i0, int j0, int Ld, double dt, int nstep,
                                 int integrator, double* x_new, double* dH, double* acc, double* H0, double* H1, double* plaq, double* Q,
                                 double* dsum_out, const double* state_in, double* state_out, void* ws, size_t ws_bytes, void* stream,
                                 uint64_t weights_version) {
    const DefectArg dfa{g_b, DefectLine{i0, j0, Ld}, dsum_out};
    FT_TRY(check_ft_defect_args(x && v && u && x_new && nstep >= 1, w, n_layers, B, L, act, beta, g_b, i0, j0, Ld));
    return ft_trajectory_call(x, v, u, w, arch, n_layers, B, L, act, beta, nullptr, dt, nstep, integrator, FTHMC_MODE_MD, nullptr, x_new, dH,
                              acc, H0, H1, plaq, Q, state_in, state_out, ws, ws_bytes, stream, weights_version, &dfa);
}
int fthmc_ft_defect_force_v(const double* x, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L, int act, double beta,
                            const double* g_b, int i0, int j0, int Ld, double* F, void* ws, size_t ws_bytes, void* stream,
                            uint64_t weights_version) {
    Ctx C; FDWS D;
    FT_TRY(check_ft_defect_args(x && F, w, n_layers, B, L, act, beta, g_b, i0, j0, Ld));
    FT_TRY(open_ft_defect_call(arch, stream, ws, ws_bytes, w, n_layers, B, L, true, weights_version, &C, &D));
    const FlowDefect fd{g_b, DefectLine{i0, j0, Ld}};
    FT_TRY(force_gp(C, x, D.W, n_layers, B, L, act, beta, -1.0, nullptr, C.s, false, nullptr, nullptr, &fd));
    return launch_kick_from_gp(D.W.gp, nullptr, nullptr, F, B, L, 0.0, 0.0, C.s);
}
int fthmc_ft_defect_action_v(const double* x, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L, int act, double beta,
                             const double* g_b, int i0, int j0, int Ld, double* S, double* logdet, double* csum, double* dsum, double* Q,
                             void* ws, size_t ws_bytes, void* stream, uint64_t weights_version) {
    Ctx C; FDWS D;
    FT_TRY(check_ft_defect_args(x != nullptr, w, n_layers, B, L, act, beta, g_b, i0, j0, Ld));
    FT_TRY(open_ft_defect_call(arch, stream, ws, ws_bytes, w, n_layers, B, L, true, weights_version, &C, &D));
    const WS& W = D.W;
    const hipStream_t s = C.s;
    const size_t row = (size_t)B * sizeof(double);
    if (n_layers == 0 && logdet && hipMemsetAsync(logdet, 0, row, s) != hipSuccess) return FTHMC_ERR_LAUNCH;
    double* sb = S ? S : W.vb;                                       // S_eff of the periodic action first, the defect's term added in place
    FT_TRY(eval_action(C, x, W, n_layers, B, L, act, beta, sb, logdet, nullptr, nullptr, s));
    FT_TRY(launch_defect_sums(phys_field(x, W, n_layers), B, L, beta, DefectLine{i0, j0, Ld}, nullptr, D.sums, s));
    FT_TRY(launch_defect_energy(D.sums, B, beta, g_b, sb, s));
    if (csum && hipMemcpyAsync(csum, D.sums, row, hipMemcpyDeviceToDevice, s) != hipSuccess) return FTHMC_ERR_LAUNCH;
    if (dsum && hipMemcpyAsync(dsum, D.sums + B, row, hipMemcpyDeviceToDevice, s) != hipSuccess) return FTHMC_ERR_LAUNCH;
    if (Q && hipMemcpyAsync(Q, D.sums + 2 * (size_t)B, row, hipMemcpyDeviceToDevice, s) != hipSuccess) return FTHMC_ERR_LAUNCH;
    return FTHMC_OK;
}

int fthmc_ft_trajectory(const double* x, const double* v, const double* u, const double* w, const fthmc_arch_t* arch, int n_layers,
                        int B, int L, int act, double beta, double dt, int nstep, int mode, double* x_new,
                        double* dH, double* acc, double* H0, double* H1, double* plaq, double* Q,
                        const double* state_in, double* state_out,
                        void* ws, size_t ws_bytes, void* stream) {
    return fthmc_ft_trajectory_v(x, v, u, w, arch, n_layers, B, L, act, beta, dt, nstep, mode, x_new, dH, acc, H0, H1, plaq, Q, state_in, state_out, ws, ws_bytes, stream, 0);
}

int fthmc_train_grad(const double* xi, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L, int act, double beta,
                     double* x, double* logq, double* logp, double* gw, void* ws, size_t ws_bytes,
                     void* stream) {
    FT_TRY(check_flow_call(xi && w && n_layers >= 1, w, n_layers, B, L, act));
    Ctx C; WS W; FT_TRY(open_flow_call(arch, stream, ws, ws_bytes, w, n_layers, B, L, true, 0, &C, &W));
    const hipStream_t s = C.s;
    if (gw && C.small(L, n_layers)) {
        // small lattices: ONE launch runs the forward sweep (stash + h1, h2 + log J), the loss pieces and the backward sweep of
        // every chain (flow_small.hip, training sweep); then the weight gradients layer by layer from the gz it left behind
        SmallArgs a = small_args(xi, W, n_layers, B, act, beta, 4);
        a.x_out = x; a.logq = logq; a.logp = logp; a.gz = W.gz;
        FT_TRY(launch_ft_small(a, L, s));
        FlowLayerArgs f(nullptr, B, L, 0, 0, act);                    // every layer's weight gradient in ONE launch + one reduction
        f.stash = W.stash; f.gz = W.gz; f.gw_part = W.gw_part;
        f.nlb = n_layers;
        f.stash_lstride = flow_stash_doubles(B, L, true); f.gz_lstride = flow_gz_doubles(B, L);
        f.tpw = flow_wgrad_tpw(B, L, n_layers);
        f.gwp_lstride = (size_t)flow_wgrad_nparts(B, L, f.tpw) * FLOW_GW_STRIDE;
        FT_TRY(launch_flow_wgrad(f, s));
        return launch_reduce_gw(W.gw_part, flow_wgrad_nparts(B, L, f.tpw), 1.0, 0, gw, W.gw_tmp, s, n_layers, f.gwp_lstride);
    }
    double* ld = W.scal + (size_t)SC_LOGDET * B;
    double* S = W.scal + (size_t)SC_S * B;
    // one forward sweep serves both the outputs (x, logq, logp) and the backward pass; with the MFMA
    // kernels it stashes act', s and h of every layer for the weight-gradient backward
    const bool mfma = C.mfma || C.gen();       // paths whose backward reads the forward's stash
    FT_TRY(sweep_forward(C, xi, W, n_layers, B, L, act, ld, s, mfma && gw != nullptr, mfma && gw != nullptr));
    if (x || logq || logp) {
        FT_TRY(launch_action_charge(phys_field(xi, W, n_layers), B, L, beta, S, nullptr, nullptr, s, W.act_part));
        const double lp0 = -(double)(2 * L * L) * log(FT_TWO_PI);
        if (logq) FT_TRY(launch_lincomb(ld, -1.0, nullptr, 0.0, lp0, logq, B, s));
        if (logp) FT_TRY(launch_lincomb(S, -1.0, nullptr, 0.0, 0.0, logp, B, s));
        if (x && hipMemcpyAsync(x, phys_field(xi, W, n_layers), W.n2 * sizeof(double),
                                hipMemcpyDeviceToDevice, s) != hipSuccess) return FTHMC_ERR_LAUNCH;
    }
    if (gw) {
        // d mean_b(S_W - logdet) / dw : seed beta/B on the Wilson term, -1/B on every logJ
        FT_TRY(force_gp(C, xi, W, n_layers, B, L, act, beta / B, -1.0 / B, gw, s, /*have_forward=*/true));
    }
    return FTHMC_OK;
}

}  // extern "C"
