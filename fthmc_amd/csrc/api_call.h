// How the entry points of api.hip, api_second_order.hip and api_diag.hip open a call -- the context, the argument checks, the
// caller's workspace carved into its family's regions (first order / training, second order, force training), the caller's
// weights -- and the sweeps of the plain kernels, which every family runs.  Host code; tests/hip/layout_walk.cpp walks the layouts.
#pragma once
#include "common.h"
#include "kernels.h"
#include "dual.h"
#include <utility>

using namespace fthmc;
#define FT_TRY(expr) do { int rc_ = (expr); if (rc_ != FTHMC_OK) return rc_; } while (0)

namespace {

// What a call runs with: the net's shape (an ARGUMENT of the call: fthmc_arch_t), the two process-wide debug switches read
// ONCE per call, the caller's canonical weights and stream.  Nothing below reads a global.
struct Ctx {
    FlowArch A;
    bool mfma;               // fthmc_set_variant: MFMA kernels (default) / VALU kernels
    bool small_on;           // fthmc_set_small_path
    const double* wcan;      // the caller's canonical weights (generic net shapes read them as they are)
    hipStream_t s;
    bool gen() const { return !A.is_default(); }
    bool small(int L, int nl) const { return small_on && mfma && A.is_default() && ft_small_shape(L, nl); }
};
inline int make_ctx(const fthmc_arch_t* arch, void* stream, Ctx* c) {
    c->A = flow_arch_default();
    if (arch) { int rc = make_flow_arch(arch->n_hidden, arch->hidden, arch->kernel_size, arch->n_mix, arch->final_tanh, &c->A); if (rc != FTHMC_OK) return rc; }
    c->mfma = get_flow_variant() == 1;
    c->small_on = get_small_path() != 0;
    c->wcan = nullptr;
    c->s = ft_stream(stream);
    return FTHMC_OK;
}
// Step 1 of a call, behind its argument checks: the context, with the stale (non-sticky) errors the host framework left dropped
inline int open_call(const fthmc_arch_t* arch, void* stream, Ctx* C) {
    (void)hipGetLastError();
    return make_ctx(arch, stream, C);
}

// FTHMC_MAX_B / FTHMC_MAX_L (fthmc_hip.h): the plain-lattice kernels (wilson.hip, rng.hip) hold the site count of a chain's
// field, 2 L^2, in int (launch_kinetic, launch_metropolis and its (2 L^2 + 2047) / 2048, k_leap_rows' plane offsets), and
// k_metropolis walks s < 2 L^2 with s += its y extent min(that / 2048, 16) * 256 <= 4096: all below 2^31 for L <= 32764, the
// last multiple of 4 before 2 L^2 reaches 2^31.  A chain is one workgroup of up to 1024 threads along x (k_action_charge,
// k_kinetic, k_traj_energy), whose extent in work-items must stay below 2^32
inline bool bad_shape(int B, int L) { return B <= 0 || B > FTHMC_MAX_B || L < 4 || L > FTHMC_MAX_L || (L % 4) != 0; }

// The precedence every entry point keeps: FTHMC_ERR_ARG, then FTHMC_ERR_UNSUPPORTED, then the workspace (open_ws and its kin:
// FTHMC_ERR_WS).  ptrs_ok: the call's own pointers and counts.
inline int check_layer_call(bool ptrs_ok, int B, int L, int mu, int off, int act) {            // one layer (mu, off)
    if (!ptrs_ok || bad_shape(B, L) || mu < 0 || mu > 1 || off < 0 || off > 3) return FTHMC_ERR_ARG;
    return act < 0 || act > 2 ? FTHMC_ERR_UNSUPPORTED : FTHMC_OK;
}
inline int check_flow_call(bool ptrs_ok, const double* w, int nl, int B, int L, int act) {     // a whole flow of nl layers
    if (!ptrs_ok || (nl > 0 && !w) || bad_shape(B, L) || nl < 0) return FTHMC_ERR_ARG;
    return act < 0 || act > 2 ? FTHMC_ERR_UNSUPPORTED : FTHMC_OK;
}

constexpr size_t ALIGN = 32;   // doubles (256 B)
// A caller's scratch handed out region by region, each rounded up to ALIGN doubles; a null scratch sizes a layout (null pointers,
// the same offsets).  A pointer is formed only where the region starts inside the scratch or at its end, so a layout is carved
// ONCE, before its size is compared with the caller's.  ovf: a size left size_t -- total() is 0.
struct Carver {
    double* base = nullptr;
    size_t avail = 0, o = 0;   // doubles of the caller's scratch; doubles handed out
    bool ovf = false;
    Carver() = default;
    Carver(void* ws, size_t ws_bytes) : base(static_cast<double*>(ws)), avail(ws_bytes / sizeof(double)) {}
    size_t mul(size_t a, size_t b) { size_t r = 0; ovf |= __builtin_mul_overflow(a, b, &r); return r; }
    size_t up(size_t n) { size_t p = 0; ovf |= __builtin_add_overflow(n, ALIGN - 1, &p); return p / ALIGN * ALIGN; }
    template <typename T = double> T* take(size_t count) {     // count elements of T: double, or Dual (two doubles)
        static_assert(sizeof(T) % sizeof(double) == 0, "regions are counted in doubles");
        T* p = base && !ovf && o <= avail ? reinterpret_cast<T*>(base + o) : nullptr;
        ovf |= __builtin_add_overflow(o, up(mul(count, sizeof(T) / sizeof(double))), &o);
        return p;
    }
    size_t total() const { return ovf || o > SIZE_MAX / sizeof(double) ? 0 : o; }     // doubles; in bytes it fits size_t too
};
// what a workspace view refuses, behind the argument checks: a size beyond size_t, then the caller's scratch
inline int check_ws(size_t total, const void* ws, size_t ws_bytes) {
    if (total == 0) return FTHMC_ERR_UNSUPPORTED;
    return !ws || ws_bytes / sizeof(double) < total ? FTHMC_ERR_WS : FTHMC_OK;
}
// beyond the ABI's limits (fthmc_hip.h: every entry point refuses them) the int arithmetic of kernels.h's geometry does not hold: no layout, total = 0
inline bool layout_shape(int B, int L, int nl) { return B >= 1 && B <= FTHMC_MAX_B && L >= 1 && L <= FTHMC_MAX_L && nl >= 0; }

struct WS {
    double *wint, *X, *gp, *gp2, *gp_part, *lj_part, *scal, *act_part, *xa, *va, *xb, *vb, *gw_part, *gw_tmp, *stash, *gz;
    double *hbuf, *gbuf;   // generic net shapes (flow_generic.hip): activation scratch, gradient ping-pong
    size_t n2;       // doubles per field batch: B * 2 * L * L
    size_t gw_rows, gw_tmp_rows;   // rows of FLOW_GW_STRIDE doubles in gw_part / gw_tmp
    size_t total;    // doubles; 0: the sizes overflow size_t
};
// scal slots, each B doubles
enum { SC_S = 0, SC_Q, SC_PLAQ, SC_LOGDET, SC_K, SC_H0, SC_H1, SC_OLD0, SC_OLD1, SC_OLD2, SC_NEW0, SC_NEW1, SC_NEW2, SC_SEFF, SC_N };

// The calls whose training backward computes the layer's weight gradients itself (flow_bwd_train.hip) and leaves every layer's
// partials side by side: ws_layout sizes the rows force_gp then finds
inline bool fused_train_bwd(const FlowArch& A, int B, int L) { return A.is_default() && flow_bwd_train_shape(L) && flow_stash_fits32(B, L, true); }

// the weight expansions: a FIXED head of FLOW_WHEAD_LAYERS layer regions in every layout (kernels.h: no call of any shape puts
// another region there, so the stamps of k_pack_weights vouch for what sits behind them), longer for deeper flows
inline size_t wint_doubles(int nl) { return (size_t)(nl > FLOW_WHEAD_LAYERS ? nl : FLOW_WHEAD_LAYERS) * FLOW_WINT; }

WS ws_layout(const FlowArch& A, Carver& c, int B, int L, int nl, bool train = false) {
    WS w{};
    if (!layout_shape(B, L, nl)) return w;
    const size_t n1 = (size_t)B * L * L, n2 = 2 * n1;
    const size_t nt = flow_ntiles_max(L);
    w.n2 = n2;
    w.wint = c.take(wint_doubles(nl));
    w.X = c.take(c.mul((size_t)nl, n2));
    w.gp = c.take(n1);
    w.gp2 = c.take(nl > 0 ? n1 : 0);                     // second plaquette-gradient field (gather-form backward)
    w.gp_part = c.take(nl > 0 ? (size_t)B * flow_gp_part_max(L) : 0);
    w.lj_part = c.take(c.mul((size_t)(nl > 0 ? nl : 1), (size_t)B * nt));   // logJ partials [layer][chain][tile] of a sweep
    w.scal = c.take((size_t)SC_N * B);
    w.act_part = c.take((size_t)32 * B);                 // launch_action_charge's wave sums (few chains of a large lattice)
    w.xa = c.take(n2); w.va = c.take(n2); w.xb = c.take(n2); w.vb = c.take(n2);
    // small lattices in training: the weight-gradient partials (and reduction rows) of ALL layers at once
    const size_t nlw = train && A.is_default() && ft_small_shape(L, nl) ? (size_t)nl : 1;
    w.gw_rows = nl > 0 ? nlw * B * nt : 0;
    w.gw_tmp_rows = nl > 0 ? nlw * FLOW_REDUCE_GROUPS : 0;
    if (train && nl > 0 && fused_train_bwd(A, B, L)) {                    // ONE reduction behind the sweep
        const size_t np = (size_t)flow_bwd_train_nparts(B, L), ng = (size_t)flow_reduce_groups((int)np);
        if (w.gw_rows < (size_t)nl * np) w.gw_rows = (size_t)nl * np;
        if (w.gw_tmp_rows < (size_t)nl * ng) w.gw_tmp_rows = (size_t)nl * ng;
    }
    w.gw_part = c.take(c.mul(w.gw_rows, FLOW_GW_STRIDE));
    w.gw_tmp = c.take(c.mul(w.gw_tmp_rows, FLOW_GW_STRIDE));
    const bool gen = !A.is_default();
    // activation stash of a force evaluation (generic shapes: every layer's planes, at least one region as scratch)
    w.stash = c.take(gen ? c.mul((size_t)(nl > 0 ? nl : 1), A.stash_doubles(B, L)) : c.mul((size_t)nl, flow_stash_doubles(B, L, train)));
    // training: pre-activation gradients of the layer in flight; small lattices (flow_small.hip: one launch runs all layers
    // forward and backward): of every layer
    w.gz = c.take(train && nl > 0 && !gen ? c.mul(flow_gz_doubles(B, L), ft_small_shape(L, nl) ? (size_t)nl : 1) : 0);
    w.hbuf = c.take(gen ? (size_t)B * A.cmax() * L * L : 0);
    w.gbuf = c.take(gen ? (size_t)2 * B * A.cmax() * L * L : 0);
    w.total = c.total();
    return w;
}
// Step 2, first order and training: the workspace view.  First the chain count the default net's kernels take, flow_shape_ok's B <= 2^20
// (kernels.h, fthmc_hip.h): their launchers refuse it too, but only behind the weight expansion -- here nothing has been enqueued yet
inline int open_ws(const Ctx& C, void* ws, size_t ws_bytes, int B, int L, int nl, bool train, WS* W) {
    if (C.A.is_default() && nl > 0 && B > (1 << 20)) return FTHMC_ERR_ARG;
    Carver c(ws, ws_bytes);
    *W = ws_layout(C.A, c, B, L, nl, train);
    return check_ws(W->total, ws, ws_bytes);
}
// The workspace of the metadynamics calls (fthmc_meta_*, fthmc_ft_meta_*): a first-order layout and behind it sums[B][2]; pairs
// (the plain sequence): the (Q_m, V) pairs of the two ends and of the selected one, [2][B] each
struct MWS { WS W; double *sums, *qv_old, *qv_new, *qv_sel; size_t total; };
MWS meta_layout(const FlowArch& A, Carver& c, int B, int L, int nl, bool pairs) {
    MWS m{};
    m.W = ws_layout(A, c, B, L, nl);
    if (m.W.total == 0) return m;
    m.sums = c.take((size_t)2 * B);
    if (pairs) { m.qv_old = c.take((size_t)2 * B); m.qv_new = c.take((size_t)2 * B); m.qv_sel = c.take((size_t)2 * B); }
    m.total = c.total();
    return m;
}
inline int open_meta_ws(const Ctx& C, void* ws, size_t ws_bytes, int B, int L, int nl, bool pairs, MWS* M) {
    Carver c(ws, ws_bytes);
    *M = meta_layout(C.A, c, B, L, nl, pairs);
    return check_ws(M->total, ws, ws_bytes);
}

// Workspace of the second-order entry points (fthmc_ft_action_vjp, fthmc_ft_force_vjp): the head of every layout (the weight
// expansions and their stamps, fthmc_ws_head_bytes()) is skipped and never written; behind it, regions sized in dual numbers (the
// action VJP runs the double kernels in their first halves): the dual input x + eps g, every layer's output and activation
// stash, the generic kernels' scratch, the gP ping-pong, the dual weight gradients and the per-chain log J coefficients.
struct VWS { Dual *xd, *X, *stash, *hbuf, *gbuf, *gp, *gp2, *gw; double* glj; size_t total; };
// head false: the regions start where the carver stands (fthmc_train_force_grad puts them behind a whole force workspace)
VWS vjp_layout(const FlowArch& A, Carver& c, int B, int L, int nl, bool head = true) {
    VWS w{};
    if (!layout_shape(B, L, nl)) return w;
    if (head) (void)c.take(wint_doubles(0));
    const size_t n1 = (size_t)B * L * L, n2 = 2 * n1, nh = nl > 0 ? n1 * A.cmax() : 0;
    w.xd = c.take<Dual>(n2);
    w.X = c.take<Dual>(c.mul((size_t)nl, n2));
    w.stash = c.take<Dual>(nl > 0 ? c.mul((size_t)nl, A.stash_doubles(B, L)) : 0);
    w.hbuf = c.take<Dual>(nh);
    w.gbuf = c.take<Dual>(2 * nh);
    w.gp = c.take<Dual>(n1);
    w.gp2 = c.take<Dual>(n1);
    w.gw = c.take<Dual>(c.mul((size_t)nl, (size_t)A.params()));
    w.glj = reinterpret_cast<double*>(c.take<Dual>(B));
    w.total = c.total();
    return w;
}
// the plain kernels pad circularly: a pad wider than the lattice is refused (as torch's Conv2d refuses it)
inline bool pad_fits(const FlowArch& A, int L, int nl) { return nl == 0 || A.k / 2 <= L; }
// Step 2, second order
inline int open_vjp_ws(const Ctx& C, void* ws, size_t ws_bytes, int B, int L, int nl, VWS* W) {
    if (!pad_fits(C.A, L, nl)) return FTHMC_ERR_UNSUPPORTED;
    Carver c(ws, ws_bytes);
    *W = vjp_layout(C.A, c, B, L, nl);
    return check_ws(W->total, ws, ws_bytes);
}

// the tile of the fused dual kernels that serves a call (flow_dual.hip), -1: the plain dual kernels; path: fthmc_set_dual_path
inline int force_dual_tile(const FlowArch& A, int B, int L, int path) {
    if (path == 0 || !A.is_default()) return -1;
    // 8 x 16 tiles where they divide the lattice and give every CU a workgroup (measured: config 3 9.6 vs 11.8 ms, config-5 shard
    // 75 vs 92 ms; config 2, 64 such tiles on 256 CUs: 0.41 vs 0.33 ms), 8 x 8 tiles otherwise
    const bool wide = flow_dual_shape(B, L, 1) && (path == 3 || (path == 1 && (long)B * flow_dual_geom(1).ntiles(L) >= 256));
    if (wide) return 1;
    return flow_dual_shape(B, L, 0) ? 0 : -1;
}
// Workspace of fthmc_train_force_grad: a whole workspace of fthmc_ft_force first (the head with the weight expansions included:
// the first-order sweep runs there as in any force call), behind it the force itself and the regions of the dual sweep -- the
// fused kernels' (dual input, checkpoint chain, plaquette gradient, its partial windows, the weight-gradient partial rows and
// the reduction's rows) or the plain kernels' (vjp_layout).
struct FWS { size_t first; double* F; Dual *xd, *X, *gp, *gpp; double *gwp, *gwt; VWS V; size_t total; };
FWS force_layout(const FlowArch& A, Carver& c, int B, int L, int nl, int tile) {
    FWS w{};
    if (ws_layout(A, c, B, L, nl).total == 0) return w;
    w.first = c.o;
    const size_t n1 = (size_t)B * L * L, n2 = 2 * n1;
    w.F = c.take(n2);
    if (tile < 0) {
        w.V = vjp_layout(A, c, B, L, nl, false);
        w.total = w.V.total;
        return w;
    }
    w.xd = c.take<Dual>(n2);
    w.X = c.take<Dual>(c.mul((size_t)nl, n2));
    w.gp = c.take<Dual>(n1);
    const FlowGeom g = flow_dual_geom(tile);
    w.gpp = c.take<Dual>(nl > 0 ? (size_t)B * g.ntiles(L) * g.n0() : 0);
    w.gwp = c.take(nl > 0 ? (size_t)flow_dual_nparts(B, L, tile) * FLOW_GW_STRIDE : 0);
    w.gwt = c.take(nl > 0 ? (size_t)FLOW_REDUCE_GROUPS * FLOW_GW_STRIDE : 0);
    w.total = c.total();
    return w;
}
// Step 2, force training
inline int open_force_ws(const Ctx& C, void* ws, size_t ws_bytes, int B, int L, int nl, int tile, FWS* W) {
    if (!pad_fits(C.A, L, nl)) return FTHMC_ERR_UNSUPPORTED;
    Carver c(ws, ws_bytes);
    *W = force_layout(C.A, c, B, L, nl, tile);
    return check_ws(W->total, ws, ws_bytes);
}

// The tuned kernels read their own expansion (k_pack_weights -> wint, the head of the workspace), the kernels for other net
// shapes (flow_generic.hip) read the canonical layout itself.
// wver: the caller's statement of the weights' content version (the `_v` entry points; 0 = none: expand).  The library keeps
// nothing between calls: the launch compares the token of (version, address of w) with the stamps the last expansion left in
// the workspace and expands the layers whose stamps differ -- a stale or wrong version costs an expansion, never a result.
inline unsigned long long weights_token(const double* w, uint64_t wver) {
    if (wver == 0) return 0ull;
    unsigned long long z = (unsigned long long)wver ^ ((unsigned long long)(uintptr_t)w * 0xD6E8FEB86659FD93ull);
    z ^= z >> 32; z *= 0xD6E8FEB86659FD93ull; z ^= z >> 32;            // a 64-bit mix: versions 1, 2, 3 ... do not look alike
    return z | 2ull;                                                     // never 0
}
// Step 3 (optional).  wint null: a call the plain kernels serve whatever the net's shape (second order)
inline int use_weights(Ctx& C, const double* w, int nl, double* wint, uint64_t wver = 0) {
    C.wcan = w;
    return wint && C.A.is_default() ? launch_pack_weights(w, nl, wint, C.s, weights_token(w, wver)) : FTHMC_OK;
}
// Steps 1 to 3 in one, for the first-order entry points that have nothing to refuse between them
inline int open_flow_call(const fthmc_arch_t* arch, void* stream, void* ws, size_t ws_bytes, const double* w, int nl, int B, int L,
                          bool train, uint64_t wver, Ctx* C, WS* W) {
    FT_TRY(open_call(arch, stream, C));
    FT_TRY(open_ws(*C, ws, ws_bytes, B, L, nl, train, W));
    return use_weights(*C, w, nl, W->wint, wver);
}

inline int flow_rev(const Ctx& C, const FlowLayerArgs& a, hipStream_t s) {
    return C.mfma ? launch_flow_rev_mfma(a, s) : launch_flow_rev(a, s);
}
inline int flow_fwd(const Ctx& C, const FlowLayerArgs& a, hipStream_t s) {
    return C.mfma ? launch_flow_fwd_mfma(a, s) : launch_flow_fwd(a, s);
}
// small lattices: the fused single-launch path (flow_small.hip)
inline SmallArgs small_args(const double* x, const WS& w, int nl, int B, int act, double beta, int mode) {
    SmallArgs a{};
    a.x = x; a.wint = w.wint; a.stash = w.stash; a.beta = beta; a.mode = mode; a.B = B; a.nl = nl; a.act = act;
    return a;
}

// Their regions: of a first-order workspace (T = double) or a second-order one (Dual; double: the first halves); lstride: per-layer stash stride
template <typename T> struct GenWS { T *X, *stash, *hbuf, *gbuf, *gp, *gp2; size_t lstride; };
inline GenWS<double> gen_ws(const Ctx& C, const WS& w, int B, int L) {
    return {w.X, w.stash, w.hbuf, w.gbuf, w.gp, w.gp2, C.A.stash_doubles(B, L)};
}
template <typename T> GenWS<T> gen_ws(const Ctx& C, const VWS& v, int B, int L) {
    return {reinterpret_cast<T*>(v.X), reinterpret_cast<T*>(v.stash), reinterpret_cast<T*>(v.hbuf), reinterpret_cast<T*>(v.gbuf),
            reinterpret_cast<T*>(v.gp), reinterpret_cast<T*>(v.gp2), C.A.stash_doubles(B, L)};
}
// layer l of a sweep: weights, scratch and stripe; own_region: the layer's own stash region (else the first, as scratch)
template <typename T>
GenLayerArgsT<T> gen_args(const Ctx& C, const GenWS<T>& V, int l, int B, int L, int act, bool own_region) {
    GenLayerArgsT<T> g{};
    g.arch = C.A;
    g.w = C.wcan + (size_t)l * C.A.params();
    g.stash = V.stash + (own_region ? (size_t)l * V.lstride : 0); g.hbuf = V.hbuf; g.gbuf = V.gbuf;
    g.B = B; g.L = L; g.mu = layer_mu(l); g.off = layer_off(l); g.act = act;
    return g;
}
// the field behind nl layers of a sweep from x
template <typename T> const T* flowed_field(const T* x, const T* X, int nl, size_t n2) { return nl == 0 ? x : X + (size_t)(nl - 1) * n2; }
// Forward: x -> X[0 .. nl - 1] (X[l] = output of layer l); own_region: every layer's activations kept for a backward sweep; logdet ([B], double) optional
template <typename T>
int gen_forward(const Ctx& C, const GenWS<T>& V, const T* x, int nl, int B, int L, int act, bool own_region, T* logdet) {
    const size_t n2 = (size_t)B * 2 * L * L;
    for (int l = 0; l < nl; ++l) {
        GenLayerArgsT<T> g = gen_args(C, V, l, B, L, act, own_region);
        g.x = l == 0 ? x : V.X + (size_t)(l - 1) * n2;
        g.y = V.X + (size_t)l * n2;
        g.logj = logdet; g.logj_accumulate = l > 0;
        FT_TRY(launch_gen_fwd(g, false, C.s));
    }
    return FTHMC_OK;
}
// Backward behind gen_forward(own_region): seed(g) writes the plaquette gradient at the flowed field, then layer by layer between V.gp and
// V.gp2, so that the walk ENDS in V.gp: the plaquette gradient at x.  d/d logJ = glogj[b] (null: glogj_const); gw (optional): all layers'.
template <typename T, class Seed>
int gen_backward(const Ctx& C, const GenWS<T>& V, int nl, int B, int L, int act, const double* glogj, double glogj_const, T* gw, Seed seed) {
    T* gcur = (nl & 1) ? V.gp2 : V.gp;
    T* galt = gcur == V.gp ? V.gp2 : V.gp;
    FT_TRY(seed(gcur));
    for (int l = nl - 1; l >= 0; --l) {
        GenLayerArgsT<T> g = gen_args(C, V, l, B, L, act, true);
        g.up_gp = gcur; g.glogj = glogj; g.glogj_const = glogj_const; g.gp_out = galt;
        g.gw = gw ? gw + (size_t)l * C.A.params() : nullptr;
        FT_TRY(launch_gen_bwd(g, C.s));
        std::swap(gcur, galt);
    }
    return FTHMC_OK;
}

}  // namespace
