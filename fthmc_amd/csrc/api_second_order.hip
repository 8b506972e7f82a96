// extern "C" entry points of libfthmc_hip.so (include/fthmc_hip.h), second order: the VJPs of S_eff / log det J (plain kernels) and of the
// force (the same on dual numbers: api_call.h's sweeps), and force-norm training: the force's VJP at g = F, plain or fused (flow_dual.hip).
#include "api_call.h"

namespace {

int g_dual_path = 1;
// shared argument checks, context and workspace view of both VJPs
int vjp_begin(const double* x, const double* w, const fthmc_arch_t* arch, int nl, int B, int L, int act, const double* cot,
              const double* gx, const double* gw, void* ws, size_t ws_bytes, void* stream, Ctx* C, VWS* W) {
    FT_TRY(check_flow_call(x && cot && (gx || gw), w, nl, B, L, act));
    FT_TRY(open_call(arch, stream, C));
    FT_TRY(open_vjp_ws(*C, ws, ws_bytes, B, L, nl, W));
    return use_weights(*C, w, nl, nullptr);
}
// The force's VJP at the dual field V.xd = x + eps g: the first-order force sweep on dual numbers; the eps parts of its plaquette
// gradient (left in V.gp) and of its weight gradients (V.gw) are H g and d/dw <g, F>
int dual_force_sweep(const Ctx& C, const VWS& V, int nl, int B, int L, int act, double beta, bool want_gw) {
    const GenWS<Dual> G = gen_ws<Dual>(C, V, B, L);
    FT_TRY(gen_forward<Dual>(C, G, V.xd, nl, B, L, act, true, nullptr));
    const Dual* xphys = flowed_field<Dual>(V.xd, G.X, nl, (size_t)B * 2 * L * L);
    return gen_backward<Dual>(C, G, nl, B, L, act, nullptr, -1.0, want_gw ? V.gw : nullptr,
                              [&](Dual* gp) { return launch_gen_seed(xphys, nullptr, B, L, beta, gp, C.s); });
}

}  // namespace

namespace fthmc {
void set_dual_path(int v) { g_dual_path = v; }
int get_dual_path() { return g_dual_path; }
}  // namespace fthmc

extern "C" {

size_t fthmc_vjp_ws_bytes(const fthmc_arch_t* arch, int B, int L, int n_layers) {
    Ctx C; Carver c;
    if (bad_shape(B, L) || n_layers < 0 || make_ctx(arch, nullptr, &C) != FTHMC_OK || !pad_fits(C.A, L, n_layers)) return 0;
    return vjp_layout(C.A, c, B, L, n_layers).total * sizeof(double);
}

int fthmc_ft_action_vjp(const double* x, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L, int act,
                        double beta, const double* gS, const double* glogdet, double* gx, double* gw,
                        void* ws, size_t ws_bytes, void* stream) {
    Ctx C; VWS V; FT_TRY(vjp_begin(x, w, arch, n_layers, B, L, act, gS, gx, gw, ws, ws_bytes, stream, &C, &V));
    const hipStream_t s = C.s;
    const GenWS<double> G = gen_ws<double>(C, V, B, L);
    FT_TRY(gen_forward<double>(C, G, x, n_layers, B, L, act, true, nullptr));
    // d/d logJ of every layer, per chain: glogdet[b] - gS[b]
    if (n_layers > 0) FT_TRY(glogdet ? launch_lincomb(glogdet, 1.0, gS, -1.0, 0.0, V.glj, B, s)
                                     : launch_lincomb(gS, -1.0, nullptr, 0.0, 0.0, V.glj, B, s));
    const double* xphys = flowed_field<double>(x, G.X, n_layers, (size_t)B * 2 * L * L);
    FT_TRY(gen_backward<double>(C, G, n_layers, B, L, act, V.glj, 0.0, gw,
                                [&](double* gp) { return launch_gen_seed(xphys, gS, B, L, beta, gp, s); }));
    return gx ? launch_kick_from_gp(G.gp, nullptr, nullptr, gx, B, L, 0.0, 0.0, s) : FTHMC_OK;
}

int fthmc_ft_force_vjp(const double* x, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L, int act,
                       double beta, const double* g, double* gx, double* gw, void* ws, size_t ws_bytes, void* stream) {
    Ctx C; VWS V; FT_TRY(vjp_begin(x, w, arch, n_layers, B, L, act, g, gx, gw, ws, ws_bytes, stream, &C, &V));
    FT_TRY(launch_dual_pack(x, g, V.xd, (size_t)B * 2 * L * L, C.s));
    FT_TRY(dual_force_sweep(C, V, n_layers, B, L, act, beta, gw != nullptr));
    if (gw && n_layers > 0) FT_TRY(launch_dual_tangent(V.gw, gw, (size_t)n_layers * C.A.params(), C.s));
    return gx ? launch_dual_links(V.gp, gx, B, L, C.s) : FTHMC_OK;
}

// ---- force-norm training: sum_b |F_b|^2 and its weight gradient (ipynb/ft_hmc.py:253-299).  With xi fixed and F = d(sum S_eff)/dxi,
// d/dw sum_b |F_b|^2 = 2 d/dw <g, F> at g = F: one first-order force, then the dual sweep of fthmc_ft_force_vjp seeded with it.
int fthmc_set_dual_path(int on) {
    if (on < 0 || on > 3) return FTHMC_ERR_ARG;
    set_dual_path(on);
    return FTHMC_OK;
}
int fthmc_get_dual_path(void) { return get_dual_path(); }

int fthmc_train_force_path(const fthmc_arch_t* arch, int B, int L) {
    Ctx C;
    if (make_ctx(arch, nullptr, &C) != FTHMC_OK) return FTHMC_ERR_UNSUPPORTED;
    return force_dual_tile(C.A, B, L, get_dual_path()) >= 0 ? 1 : 0;
}

size_t fthmc_train_force_ws_bytes(const fthmc_arch_t* arch, int B, int L, int n_layers) {
    Ctx C; Carver c;
    if (bad_shape(B, L) || n_layers < 0 || make_ctx(arch, nullptr, &C) != FTHMC_OK || !pad_fits(C.A, L, n_layers)) return 0;
    return force_layout(C.A, c, B, L, n_layers, force_dual_tile(C.A, B, L, get_dual_path())).total * sizeof(double);
}

int fthmc_train_force_grad(const double* xi, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L,
                           int act, double beta, double* F, double* force_sq, double* gw,
                           void* ws, size_t ws_bytes, void* stream) {
    FT_TRY(check_flow_call(xi && force_sq, w, n_layers, B, L, act));
    Ctx C; FWS W; FT_TRY(open_call(arch, stream, &C));
    const int nl = n_layers, tile = force_dual_tile(C.A, B, L, get_dual_path());
    FT_TRY(open_force_ws(C, ws, ws_bytes, B, L, nl, tile, &W));
    const hipStream_t s = C.s;
    // the first-order force, as fthmc_ft_force computes it, in the front part of the workspace
    double* Fo = F ? F : W.F;
    FT_TRY(fthmc_ft_force_v(xi, w, arch, nl, B, L, act, beta, Fo, ws, W.first * sizeof(double), stream, 0));
    FT_TRY(launch_kinetic(Fo, B, L, force_sq, s));                       // sum over the links of F^2, one workgroup per chain
    if (!gw || nl == 0) return FTHMC_OK;
    const size_t n1 = (size_t)B * L * L, n2 = 2 * n1;
    if (tile < 0) {                                                      // the plain dual kernels: fthmc_ft_force_vjp's sweep at g = F
        FT_TRY(use_weights(C, w, nl, nullptr));
        FT_TRY(launch_dual_pack(xi, Fo, W.V.xd, n2, s));
        FT_TRY(dual_force_sweep(C, W.V, nl, B, L, act, beta, true));
        return launch_dual_tangent(W.V.gw, gw, (size_t)nl * C.A.params(), s, 2.0);
    }
    // the fused dual kernels (flow_dual.hip) on the weight expansion the force call has just left in the head
    const double* wint = static_cast<const double*>(ws);
    FT_TRY(launch_dual_pack(xi, Fo, W.xd, n2, s));
    auto layer = [&](int l) {
        FlowDualArgs a{};
        a.x = l == 0 ? W.xd : W.X + (size_t)(l - 1) * n2;
        a.wint = wint + (size_t)l * FLOW_WINT;
        a.B = B; a.L = L; a.mu = layer_mu(l); a.off = layer_off(l); a.act = act;
        return a;
    };
    for (int l = 0; l < nl; ++l) {
        FlowDualArgs a = layer(l);
        a.y = W.X + (size_t)l * n2;
        FT_TRY(launch_flow_dual_fwd(a, tile, s));
    }
    FT_TRY(launch_gen_seed(W.X + (size_t)(nl - 1) * n2, nullptr, B, L, beta, W.gp, s));
    const int np = flow_dual_nparts(B, L, tile);
    for (int l = nl - 1; l >= 0; --l) {
        FlowDualArgs a = layer(l);
        a.up_gp = W.gp; a.gp_part = W.gpp; a.gw_part = W.gwp; a.glogj_const = -1.0;
        FT_TRY(launch_flow_dual_bwd(a, tile, s));
        FT_TRY(launch_reduce_gw(W.gwp, np, 2.0, 0, gw + (size_t)l * FTHMC_W_PER_LAYER, W.gwt, s));
        if (l > 0) FT_TRY(launch_gather_gp_dual(W.gpp, B, L, tile, W.gp, s));      // nothing reads the plaquette gradient at xi
    }
    return FTHMC_OK;
}

}  // extern "C"
