// Test-only device probe (tests/test_device_math_gpu.py, tests/test_dual_math_gpu.py, tests/test_rng_gpu.py): the kernels' own fp64
// math helpers (common.h, flow_common.h), their dual-number overloads (dual.h), the tan-mixture transform on double and on Dual
// (flow_transform.h), integer index helpers (flow_mfma_common.h) and the draws of the random streams from raw words
// (rng_common.h), applied elementwise to arrays, exactly as the headers define them -- nothing is copied.  Built by
// `make -C fthmc_amd/csrc probe` with the kernels' CXXFLAGS (same FP-contraction policy), never linked into
// libfthmc_hip.so.  Every launcher takes HOST arrays, copies them in and out, and returns the first HIP error (0 = success).
#include <hip/hip_runtime.h>
#include <utility>
#include "../../fthmc_amd/csrc/common.h"
#include "../../fthmc_amd/csrc/flow_common.h"
#include "../../fthmc_amd/csrc/flow_mfma_common.h"
#include "../../fthmc_amd/csrc/flow_transform.h"
#include "../../fthmc_amd/csrc/dual.h"
#include "../../fthmc_amd/csrc/rng_common.h"

using namespace fthmc_flow;

enum {
    P_SIGMOID = 0, P_SIGMOID4, P_EXP, P_EXPN4, P_EXPN2, P_ACT, P_ACT4, P_SINCOS, P_ATAN, P_RCP, P_WRAP, P_WRAP_PM_PI,
    P_REGULARIZE, P_COMPOSITE, P_INVERSE, P_ADJOINT, P_NOPS
};

// scalar ops: one element per thread; the N-wide forms (sigmoid4, ft_expN, act_eval4): N consecutive elements per thread; the
// transform's inverse and adjoint: one record of 4 / 8 consecutive elements per thread
template <int OP>
__global__ void k_math(const double* __restrict__ x, const double* __restrict__ s, double* o0, double* o1, double* o2, int n, int act) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (OP == P_SIGMOID4 || OP == P_EXPN4 || OP == P_ACT4) {
        if (4 * t >= n) return;
        const double z[4] = {x[4 * t], x[4 * t + 1], x[4 * t + 2], x[4 * t + 3]};
        double a[4], b[4] = {0.0, 0.0, 0.0, 0.0};
        if (OP == P_SIGMOID4) sigmoid4(z, a);
        else if (OP == P_EXPN4) ft_expN<4>(z, a);
        else act_eval4(z, act, a, b);
        for (int q = 0; q < 4; ++q) { o0[4 * t + q] = a[q]; if (OP == P_ACT4) o1[4 * t + q] = b[q]; }
        return;
    }
    if (OP == P_EXPN2) {
        if (2 * t >= n) return;
        const double z[2] = {x[2 * t], x[2 * t + 1]};
        double e[2];
        ft_expN<2>(z, e);
        o0[2 * t] = e[0]; o0[2 * t + 1] = e[1];
        return;
    }
    if (OP == P_INVERSE) {
        // mix_inverse as flow_fwd.hip's REV instances call it: x = (P', t, s_0, s_1), s[0] = tol -> o0 = (root, mean_k 1 / D_k there)
        if (4 * t >= n) return;
        const double ea[4] = {x[4 * t + 2], -x[4 * t + 2], x[4 * t + 3], -x[4 * t + 3]};
        double eo[4], fp;
        ft_expN<4>(ea, eo);
        o0[4 * t] = mix_inverse(ft_wrap(x[4 * t] - x[4 * t + 1]), NMIX, s[4 * t],
                                [&](int k) { return ExpPair{eo[2 * k], eo[2 * k + 1]}; }, fp);
        o0[4 * t + 1] = fp;
        return;
    }
    if (OP == P_ADJOINT) {
        // MixAdjoint from a stash record: x = (A_0 B_0 C_0 E_0 A_1 B_1 C_1 E_1), s = (gd, cb) -> o0 = (dL/ds_0, dL/ds_1, dir)
        if (8 * t >= n) return;
        double tc[8];
        for (int q = 0; q < 8; ++q) tc[q] = x[8 * t + q];
        const MixAdjoint<double> adj(s[8 * t], s[8 * t + 1], tc, NMIX);
        o0[8 * t] = adj.gs(tc[0], tc[1]); o0[8 * t + 1] = adj.gs(tc[4], tc[5]); o0[8 * t + 2] = adj.dir();
        return;
    }
    if (t >= n) return;
    const double v = x[t];
    if (OP == P_SIGMOID) o0[t] = ft_sigmoid(v);
    if (OP == P_EXP) o0[t] = ft_exp(v);
    if (OP == P_ACT) { double h, d; act_eval(v, act, h, d); o0[t] = h; o1[t] = d; }
    if (OP == P_SINCOS) { double sn, cs; ft_sincos(v, &sn, &cs); o0[t] = sn; o1[t] = cs; }
    if (OP == P_ATAN) o0[t] = ft_atan(v);
    if (OP == P_RCP) o0[t] = ft_rcp(v);
    if (OP == P_WRAP) o0[t] = ft_wrap(v);
    if (OP == P_WRAP_PM_PI) o0[t] = ft_wrap_pm_pi(v);
    if (OP == P_REGULARIZE) o0[t] = ft_regularize(v);
    if (OP == P_COMPOSITE) {
        // one mixture component of the tan-mixture transform as the MFMA forward evaluates it (flow_fwd.hip: the sincos of P / 2
        // in the plaquette stage, then MixComp): x = P, s = s_k
        double sn, cs;
        ft_sincos(0.5 * v, &sn, &cs);
        const MixComp<double> m(s[t], cs, sn);
        o0[t] = m.y();
        o1[t] = m.D;
        o2[t] = m.invD;
    }
}

// ---- the dual-number overloads of dual.h and the Dual instances of flow_transform.h.  Planes of n doubles: in[p * n + i] is input
// plane p of element i, out[q * n + i] output plane q; a dual operand takes two planes (value, tangent).  Operands a, b, c of the
// arithmetic ops: planes 0-1, 2-3, 4-5 (a scalar operand reads its value plane alone).
enum {
    D_MUL = 0, D_DIV_DD, D_DIV_SD, D_FMA_SDD, D_FMA_DDD, D_LOG, D_TANH, D_WRAP, D_WRAP_PM_PI, D_SINCOS, D_EXP, D_RCP, D_ATAN, D_ACT,
    D_MIXFWD, D_MIXBWD, D_NEW_PLAQ, D_ADJOINT, D_NOPS
};
__host__ __device__ constexpr int dual_nin(int op) {
    return op == D_MUL || op == D_DIV_DD || op == D_DIV_SD || op == D_MIXFWD || op == D_MIXBWD || op == D_NEW_PLAQ ? 4
         : op == D_FMA_SDD || op == D_FMA_DDD ? 6 : op == D_ADJOINT ? 14 : 2;
}
__host__ __device__ constexpr int dual_nout(int op) {
    return op == D_SINCOS || op == D_ACT ? 4 : op == D_LOG || op == D_TANH || op == D_NEW_PLAQ ? 3 : op == D_MIXFWD ? 9
         : op == D_MIXBWD ? 24 : op == D_ADJOINT ? 6 : 2;
}

// One mixture component as the kernels form it, (sn, cs) = ft_sincos(0.5 P) as they take them.  Forward (mix_forward of
// flow_generic.hip, the transform stage of flow_dual.hip; probe_math's composite on double): y, D, 1 / D.  Backward (the adjoint
// stages of the same files): sin P = 2.0 * sn * cs, then A, C, B and E as the tuned kernels stash them (Bn, En times invD2), B and
// E as these backwards form them ((. invD) invD), and the D, 1 / D they rest on.
template <typename T> struct CompOut { T v[8]; };
template <typename T> __device__ __forceinline__ CompOut<T> comp_fwd(T P, T s) {
    T sn, cs;
    ft_sincos(0.5 * P, &sn, &cs);
    const MixComp<T> m(s, cs, sn);
    CompOut<T> o;
    o.v[0] = m.y(); o.v[1] = m.D; o.v[2] = m.invD;
    return o;
}
template <typename T> __device__ __forceinline__ CompOut<T> comp_bwd(T P, T s, int K) {
    T sn, cs;
    ft_sincos(0.5 * P, &sn, &cs);
    const T sinP = 2.0 * sn * cs;
    const MixComp<T> m(s, cs, sn);
    CompOut<T> o;
    o.v[0] = m.A(sinP, K); o.v[1] = m.C(K); o.v[2] = m.B(m.invD2()); o.v[3] = m.E(sinP, m.invD2());
    o.v[4] = m.Bn() * m.invD * m.invD; o.v[5] = m.En(sinP) * m.invD * m.invD;
    o.v[6] = m.D; o.v[7] = m.invD;
    return o;
}

template <int OP>
__global__ void k_dual(const double* __restrict__ in, double* __restrict__ out, int n, int act, int K) {
    using fthmc::Dual;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t N = (size_t)n;
    auto dl = [&](int p) { return Dual(in[p * N + i], in[(p + 1) * N + i]); };
    auto put = [&](int q, Dual r) { out[q * N + i] = r.v; out[(q + 1) * N + i] = r.t; };
    const Dual a = dl(0);
    if (OP == D_MUL) put(0, a * dl(2));
    if (OP == D_DIV_DD) put(0, a / dl(2));
    if (OP == D_DIV_SD) put(0, a.v / dl(2));
    if (OP == D_FMA_SDD) put(0, fma(a.v, dl(2), dl(4)));
    if (OP == D_FMA_DDD) put(0, fma(a, dl(2), dl(4)));
    if (OP == D_LOG) { put(0, log(a)); out[2 * N + i] = ::log(a.v); }             // plane 2: the double function on the value
    if (OP == D_TANH) { put(0, tanh(a)); out[2 * N + i] = ::tanh(a.v); }
    if (OP == D_WRAP) put(0, ft_wrap(a));
    if (OP == D_WRAP_PM_PI) put(0, ft_wrap_pm_pi(a));
    if (OP == D_SINCOS) { Dual sn, cs; ft_sincos(a, &sn, &cs); put(0, sn); put(2, cs); }
    if (OP == D_EXP) put(0, ft_exp(a));
    if (OP == D_RCP) put(0, ft_rcp(a));
    if (OP == D_ATAN) put(0, ft_atan(a));
    if (OP == D_ACT) { Dual h, d; act_eval(a, act, h, d); put(0, h); put(2, d); }
    if (OP == D_MIXFWD) {
        // in: P, s; out planes 0-5: y, D, 1 / D of comp_fwd<Dual>, 6-8: the values of comp_fwd<double>
        const CompOut<Dual> o = comp_fwd<Dual>(a, dl(2));
        const CompOut<double> od = comp_fwd<double>(a.v, in[2 * N + i]);
        for (int q = 0; q < 3; ++q) { put(2 * q, o.v[q]); out[(6 + q) * N + i] = od.v[q]; }
    }
    if (OP == D_MIXBWD) {
        // in: P, s; out planes 0-15: the eight results of comp_bwd<Dual>, 16-23: the values of comp_bwd<double>
        const CompOut<Dual> o = comp_bwd<Dual>(a, dl(2), K);
        const CompOut<double> od = comp_bwd<double>(a.v, in[2 * N + i], K);
        for (int q = 0; q < 8; ++q) { put(2 * q, o.v[q]); out[(16 + q) * N + i] = od.v[q]; }
    }
    if (OP == D_NEW_PLAQ) {
        // in: ysum, t; plane 2: the double instance
        put(0, mix_new_plaq<Dual>(a, K, dl(2)));
        out[2 * N + i] = mix_new_plaq<double>(a.v, K, in[2 * N + i]);
    }
    if (OP == D_ADJOINT) {
        // in: gd, cbr, csum, esum, A_k, B_k, g; out: gs (0-1), dir_onto (2-3), the double instance's two values (4, 5)
        const MixAdjoint<Dual> adj(a, dl(2), dl(4), dl(6));
        put(0, adj.gs(dl(8), dl(10))); put(2, adj.dir_onto(dl(12)));
        const MixAdjoint<double> ad(a.v, in[2 * N + i], in[4 * N + i], in[6 * N + i]);
        out[4 * N + i] = ad.gs(in[8 * N + i], in[10 * N + i]); out[5 * N + i] = ad.dir_onto(in[12 * N + i]);
    }
}

template <int D> __global__ void k_fdiv(int* out, int n) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u < n) out[u] = fdiv<D>(u);
}

// blockIdx.y = lattice k: L = lstart + 4 k, v = -L .. -L + cnt(L) - 1 with cnt(L) = 3 L + extra, written at out + base(k)
template <bool FAST, bool POW2>
__global__ void k_wrap_line(int lstart, int extra, const long long* __restrict__ base, int* out) {
    const int L = lstart + 4 * (int)blockIdx.y, cnt = 3 * L + extra;
    const unsigned magic = POW2 ? (unsigned)(L - 1) : (FAST ? 0u : wrap_magic(L));
    int* o = out + base[blockIdx.y];
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < cnt; k += gridDim.x * blockDim.x)
        o[k] = wrap_line<FAST, POW2>(k - L, L, magic);
}

// every stash index map at the sites (rows[r], j) for all j, then (i, cols[c]) for all i; the host keeps the sites each map is for
__global__ void k_stash(int L, int mu, int off, const int* __restrict__ rows, int nrows, const int* __restrict__ cols, int ncols,
                        int* act, int* live, int* live2, int* frozen) {
    const long long nsite = (long long)(nrows + ncols) * L;
    for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x; k < nsite; k += (long long)gridDim.x * blockDim.x) {
        const int r = (int)(k / L), m = (int)(k % L);
        const int i = r < nrows ? rows[r] : m, j = r < nrows ? m : cols[r - nrows];
        act[k] = stash_active_idx(i, j, L, mu);
        live[k] = stash_live_idx<false>(i, j, L, mu, off);
        live2[k] = (L & (L - 1)) == 0 ? stash_live_idx<true>(i, j, L, mu, off) : -1;
        frozen[k] = stash_frozen_idx(i, j, L, mu, off);
    }
}

// the block at the far corner of a (1, gy, gz) grid reports in: whether a launch of that extent runs at all
__global__ void k_grid_corner(int* seen) {
    if (threadIdx.x == 0 && blockIdx.y == gridDim.y - 1 && blockIdx.z == gridDim.z - 1) seen[0] = (int)(blockIdx.y + 1) ^ (int)(blockIdx.z + 1);
}

// raw Philox blocks: out[k][0..4) = philox4x32_10(ctr[k][0..4), key[k][0..2))
__global__ void k_philox(const uint32_t* __restrict__ ctr, const uint32_t* __restrict__ key, uint32_t* __restrict__ out, int n) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const fthmc_rng::u4 r = fthmc_rng::philox4x32_10(fthmc_rng::u4{ctr[4 * k], ctr[4 * k + 1], ctr[4 * k + 2], ctr[4 * k + 3]},
                                                     key[2 * k], key[2 * k + 1]);
    out[4 * k] = r.x; out[4 * k + 1] = r.y; out[4 * k + 2] = r.z; out[4 * k + 3] = r.w;
}

// every draw of rng.hip from one block of words w[k][0..4): o[0] = u53(w0, w1), o[1] = u53(w2, w3), (o[2], o[3]) = normal_pair,
// o[4] = accept_uniform(w0, w1), o[5] = uniform_value(w0, w1, lo, wd), o[6] = uniform_value(w2, w3, lo, wd); o: 7 planes of n
__global__ void k_draws(const uint32_t* __restrict__ w, double lo, double wd, double* __restrict__ o, int n) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const fthmc_rng::u4 r{w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]};
    const size_t N = (size_t)n;
    o[k] = fthmc_rng::u53(r.x, r.y);
    o[N + k] = fthmc_rng::u53(r.z, r.w);
    const fthmc_rng::normal_pair g(r);
    o[2 * N + k] = g.first(); o[3 * N + k] = g.second();
    o[4 * N + k] = fthmc_rng::accept_uniform(r.x, r.y);
    o[5 * N + k] = fthmc_rng::uniform_value(r.x, r.y, lo, wd);
    o[6 * N + k] = fthmc_rng::uniform_value(r.z, r.w, lo, wd);
}

namespace {

struct Dev {                                   // device copies of the host arrays of one call, freed on every path
    void* p[8] = {};
    int np = 0;
    hipError_t err = hipSuccess;
    template <class T> T* in(const T* h, size_t n) {
        T* d = alloc<T>(n);
        if (d && h && err == hipSuccess) err = hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice);
        return d;
    }
    template <class T> T* alloc(size_t n) {
        void* d = nullptr;
        if (err == hipSuccess && n) err = hipMalloc(&d, n * sizeof(T));
        if (d) p[np++] = d;
        return static_cast<T*>(d);
    }
    template <class T> void out(T* h, const T* d, size_t n) {
        if (h && d && err == hipSuccess) err = hipMemcpy(h, d, n * sizeof(T), hipMemcpyDeviceToHost);
    }
    void launched() {
        if (err == hipSuccess) err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
    }
    ~Dev() { for (int k = 0; k < np; ++k) (void)hipFree(p[k]); }
};

template <int OP> void launch_math(int n, int act, const double* x, const double* s, double* o0, double* o1, double* o2) {
    const int per = (OP == P_SIGMOID4 || OP == P_EXPN4 || OP == P_ACT4 || OP == P_INVERSE) ? 4 : OP == P_ADJOINT ? 8 : OP == P_EXPN2 ? 2 : 1;
    const int nt = (n + per - 1) / per;
    hipLaunchKernelGGL(k_math<OP>, dim3((nt + 255) / 256), dim3(256), 0, 0, x, s, o0, o1, o2, n, act);
}

template <int... OPS>
void math_dispatch(int op, std::integer_sequence<int, OPS...>, int n, int act, const double* x, const double* s, double* o0, double* o1,
                   double* o2) {
    ((op == OPS ? launch_math<OPS>(n, act, x, s, o0, o1, o2) : void()), ...);
}

template <int OP> void launch_dual(const double* in, double* out, int n, int act, int K) {
    hipLaunchKernelGGL(k_dual<OP>, dim3((n + 255) / 256), dim3(256), 0, 0, in, out, n, act, K);
}
template <int... OPS>
void dual_dispatch(int op, std::integer_sequence<int, OPS...>, const double* in, double* out, int n, int act, int K) {
    ((op == OPS ? launch_dual<OPS>(in, out, n, act, K) : void()), ...);
}

template <int D> void launch_fdiv(int* out, int n) {
    hipLaunchKernelGGL(k_fdiv<D>, dim3((n + 255) / 256), dim3(256), 0, 0, out, n);
}
template <int... DS> void fdiv_dispatch(int d, std::integer_sequence<int, DS...>, int* out, int n) {
    ((d == DS + 2 ? launch_fdiv<DS + 2>(out, n) : void()), ...);
}

}  // namespace

extern "C" {

int probe_nops(void) { return P_NOPS; }

// n elements (a multiple of 4 for the four-wide forms and the inverse, of 8 for the adjoint, of 2 for ft_expN<2>); s: the
// composite's s_k, the inverse's tol and the adjoint's (gd, cb) at the head of each record, else unused (may be null);
// o1: the second output of act_eval / act_eval4 / ft_sincos / the composite (D_k), o2: the composite's ft_rcp(D_k)
int probe_math(int op, int act, const double* x, const double* s, double* o0, double* o1, double* o2, int n) {
    if (op < 0 || op >= P_NOPS || n <= 0 || !x || !o0) return (int)hipErrorInvalidValue;
    if ((op == P_SIGMOID4 || op == P_EXPN4 || op == P_ACT4 || op == P_INVERSE) && n % 4) return (int)hipErrorInvalidValue;
    if (op == P_ADJOINT && n % 8) return (int)hipErrorInvalidValue;
    if (op == P_EXPN2 && n % 2) return (int)hipErrorInvalidValue;
    if ((op == P_ACT || op == P_ACT4 || op == P_SINCOS || op == P_COMPOSITE) && !o1) return (int)hipErrorInvalidValue;
    if (op == P_COMPOSITE && (!s || !o2)) return (int)hipErrorInvalidValue;
    if ((op == P_INVERSE || op == P_ADJOINT) && !s) return (int)hipErrorInvalidValue;
    Dev d;
    const size_t N = (size_t)n;
    const double* dx = d.in(x, N);
    const double* ds = s ? d.in(s, N) : nullptr;
    double* d0 = d.alloc<double>(N);
    double* d1 = d.alloc<double>(N);
    double* d2 = d.alloc<double>(N);
    if (d.err != hipSuccess) return (int)d.err;
    math_dispatch(op, std::make_integer_sequence<int, P_NOPS>{}, n, act, dx, ds, d0, d1, d2);
    d.launched();
    d.out(o0, d0, N); d.out(o1, d1, N); d.out(o2, d2, N);
    return (int)d.err;
}

// The dual-number ops (k_dual): in holds dual_nin(op) planes of n doubles, out dual_nout(op) planes; nin / nout are checked against
// them.  act: the activation of D_ACT; K: the number of mixture components of D_MIXBWD / D_NEW_PLAQ (>= 1)
int probe_dual_nops(void) { return D_NOPS; }
int probe_dual(int op, int act, int K, const double* in, int nin, double* out, int nout, int n) {
    if (op < 0 || op >= D_NOPS || n <= 0 || !in || !out || K < 1 || act < 0 || act > 2) return (int)hipErrorInvalidValue;
    if (nin != dual_nin(op) || nout != dual_nout(op)) return (int)hipErrorInvalidValue;
    Dev d;
    const size_t N = (size_t)n;
    const double* di = d.in(in, nin * N);
    double* dout = d.alloc<double>(nout * N);
    if (d.err != hipSuccess) return (int)d.err;
    dual_dispatch(op, std::make_integer_sequence<int, D_NOPS>{}, di, dout, n, act, K);
    d.launched();
    d.out(out, dout, nout * N);
    return (int)d.err;
}

// out[u] = fdiv<D>(u), u < n, 2 <= D <= 32
int probe_fdiv(int D, int* out, int n) {
    if (D < 2 || D > 32 || n <= 0 || !out) return (int)hipErrorInvalidValue;
    Dev d;
    int* o = d.alloc<int>((size_t)n);
    if (d.err != hipSuccess) return (int)d.err;
    fdiv_dispatch(D, std::make_integer_sequence<int, 31>{}, o, n);
    d.launched();
    d.out(out, o, (size_t)n);
    return (int)d.err;
}

// form 0: general (wrap_magic), 1: FAST, 2: POW2 (FAST + POW2, as the EXACT kernel instances); lattices L = lstart + 4 k,
// k < nl; lattice k's results wrap_line(v) for v = -L .. 2 L + extra - 1 at out + base[k]
int probe_wrap_line(int form, int lstart, int nl, int extra, const long long* base, int* out, long long total) {
    if (form < 0 || form > 2 || lstart < 4 || lstart % 4 || nl <= 0 || nl > 65535 || extra < 0 || !base || !out || total <= 0)
        return (int)hipErrorInvalidValue;
    const int lmax = lstart + 4 * (nl - 1);
    for (int k = 0; k < nl; ++k)
        if (base[k] < 0 || base[k] + 3LL * (lstart + 4 * k) + extra > total) return (int)hipErrorInvalidValue;
    Dev d;
    const long long* db = d.in(base, (size_t)nl);
    int* o = d.alloc<int>((size_t)total);
    if (d.err != hipSuccess) return (int)d.err;
    const dim3 grid((3 * lmax + extra + 255) / 256, nl);
    if (form == 0) hipLaunchKernelGGL((k_wrap_line<false, false>), grid, dim3(256), 0, 0, lstart, extra, db, o);
    if (form == 1) hipLaunchKernelGGL((k_wrap_line<true, false>), grid, dim3(256), 0, 0, lstart, extra, db, o);
    if (form == 2) hipLaunchKernelGGL((k_wrap_line<true, true>), grid, dim3(256), 0, 0, lstart, extra, db, o);
    d.launched();
    d.out(out, o, (size_t)total);
    return (int)d.err;
}

// the four stash maps at (nrows + ncols) * L sites (k_stash); every output array holds that many ints
int probe_stash(int L, int mu, int off, const int* rows, int nrows, const int* cols, int ncols, int* act, int* live, int* live2,
                int* frozen) {
    if (L < 4 || L % 4 || mu < 0 || mu > 1 || off < 0 || off > 3 || nrows < 0 || ncols < 0 || nrows + ncols == 0) return (int)hipErrorInvalidValue;
    if ((nrows && !rows) || (ncols && !cols) || !act || !live || !live2 || !frozen) return (int)hipErrorInvalidValue;
    for (int r = 0; r < nrows; ++r) if (rows[r] < 0 || rows[r] >= L) return (int)hipErrorInvalidValue;
    for (int c = 0; c < ncols; ++c) if (cols[c] < 0 || cols[c] >= L) return (int)hipErrorInvalidValue;
    const size_t ns = (size_t)(nrows + ncols) * (size_t)L;
    Dev d;
    const int* dr = nrows ? d.in(rows, (size_t)nrows) : nullptr;
    const int* dc = ncols ? d.in(cols, (size_t)ncols) : nullptr;
    int* o[4];
    for (int k = 0; k < 4; ++k) o[k] = d.alloc<int>(ns);
    if (d.err != hipSuccess) return (int)d.err;
    const size_t blocks = (ns + 255) / 256;
    hipLaunchKernelGGL(k_stash, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, 0, L, mu, off, dr, nrows, dc, ncols,
                       o[0], o[1], o[2], o[3]);
    d.launched();
    d.out(act, o[0], ns); d.out(live, o[1], ns); d.out(live2, o[2], ns); d.out(frozen, o[3], ns);
    return (int)d.err;
}

// n Philox blocks: ctr [n][4], key [n][2] -> out [n][4]
int probe_philox(const uint32_t* ctr, const uint32_t* key, uint32_t* out, int n) {
    if (!ctr || !key || !out || n <= 0) return (int)hipErrorInvalidValue;
    Dev d;
    const size_t N = (size_t)n;
    const uint32_t* dc = d.in(ctr, 4 * N);
    const uint32_t* dk = d.in(key, 2 * N);
    uint32_t* o = d.alloc<uint32_t>(4 * N);
    if (d.err != hipSuccess) return (int)d.err;
    hipLaunchKernelGGL(k_philox, dim3((n + 255) / 256), dim3(256), 0, 0, dc, dk, o, n);
    d.launched();
    d.out(out, o, 4 * N);
    return (int)d.err;
}

// the draws of n word blocks (k_draws): words [n][4], out: 7 planes of n doubles; the prior on [lo, lo + w) with w = hi - lo
// formed here as k_random_uniform forms it
int probe_draws(const uint32_t* words, double lo, double hi, double* out, int n) {
    if (!words || !out || n <= 0) return (int)hipErrorInvalidValue;
    Dev d;
    const size_t N = (size_t)n;
    const uint32_t* dw = d.in(words, 4 * N);
    double* o = d.alloc<double>(7 * N);
    if (d.err != hipSuccess) return (int)d.err;
    const double w = hi - lo;
    hipLaunchKernelGGL(k_draws, dim3((n + 255) / 256), dim3(256), 0, 0, dw, lo, w, o, n);
    d.launched();
    d.out(out, o, 7 * N);
    return (int)d.err;
}

// the runtime's grid limits (hipDeviceProp_t::maxGridSize), and whether a (1, gy, gz) grid launches and reaches its last block:
// seen = gy ^ gz then; the launch error otherwise
int probe_grid_limits(int* xyz) {
    hipDeviceProp_t p;
    const hipError_t e = hipGetDeviceProperties(&p, 0);
    if (e == hipSuccess) for (int k = 0; k < 3; ++k) xyz[k] = p.maxGridSize[k];
    return (int)e;
}
int probe_grid_launch(unsigned gy, unsigned gz, int* seen) {
    if (!seen || gy == 0 || gz == 0) return (int)hipErrorInvalidValue;
    Dev d;
    int* o = d.in(seen, 1);
    if (d.err != hipSuccess) return (int)d.err;
    hipLaunchKernelGGL(k_grid_corner, dim3(1, gy, gz), dim3(64), 0, 0, o);
    d.launched();
    d.out(seen, o, 1);
    return (int)d.err;
}

}  // extern "C"
