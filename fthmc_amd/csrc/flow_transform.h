// The tan-mixture transform of the coupling layers (fthmc/utils/layers.py:66-90; its inverse :294-320, 373-396), stated once for
// flow_fwd.hip, flow_small.hip, flow_bwd_gather.hip, flow_bwd_train.hip, flow_generic.hip and tests/hip/device_probe.hip.  At an
// active site with plaquette P, (cs, sn) = (cos, sin)(P/2), and net outputs s_0 .. s_{K-1}, t:
//     y_k = wrap(2 atan(e^{s_k} sn / cs)),   D_k = e^{-s_k} cs^2 + e^{s_k} sn^2,   P' = wrap(mean_k y_k + t),
//     log J = log(sum_k 1/D_k) - log K   (= logsumexp_k(-log D_k) - log K)
// The pieces are values formed where the caller asks for them: a kernel keeps its own order of loads, stores and barriers.  K is a
// plain argument (NMIX in the tuned kernels, where it folds); T is double, or Dual (dual.h) in flow_generic.hip.  Results are
// pinned bit for bit: no expression may change its operand order or its helper.  That holds per caller, not from one caller to
// the next: which product of a sum becomes an FMA is the compiler's choice and follows what else the caller forms.  In
// tests/hip/device_probe.hip D_k is fma(e^-s, cs^2, round(e^s sn^2)) where Bn() is formed next to it, as a backward stage does, and
// differs in the last bit from the D_k of the forward form at one input in ten (tests/test_dual_math_gpu.py: 78 of 792, never more
// than 1 ulp; 2 ulp is the most two such forms can differ).  flow.hip, the VALU variant, deliberately keeps a second statement of
// the inverse (ocml's math, started at 0).
#pragma once
#include "flow_common.h"

namespace fthmc_flow {

// ---- one component.  e^{-s} = 1 / e^{s} and 1 / D by ft_rcp: |s| is O(1) for any usable flow and clamped to +-700 by ft_exp, so
// every denominator is far from the ends of the range; sn / cs by a TRUE division: |cs| can be tiny (P near +-pi).
// With it the adjoint's four coefficients (struct Stash, flow_mfma_common.h), sinP = sin P:
//     A_k = dy_k/ds_k / K = sin P / (K D_k)     C_k = 1 / (K D_k)   (sum_k C_k = dP'/dP)
//     B_k = d log(1/D_k)/ds_k / D_k             E_k = -d(1/D_k)/dP  (the log J terms, before their 1 / sum_k 1/D_k)
// flow_generic.hip recomputes them in its backward with roundings of its own: sinP = (2 sn) cs, and Bn, En times invD twice.
template <typename T> struct MixComp {
    T cs, sn, es, ems, cs2, sn2, D, invD;
    __device__ __forceinline__ MixComp(T s, T cs_, T sn_)
        : cs(cs_), sn(sn_), es(ft_exp(s)), ems(ft_rcp(es)), cs2(cs * cs), sn2(sn * sn), D(ems * cs2 + es * sn2), invD(ft_rcp(D)) {}
    __device__ __forceinline__ T y() const { return ft_wrap_pm_pi(2 * ft_atan(es * (sn / cs))); }
    __device__ __forceinline__ T sinP() const { return 2.0 * (sn * cs); }
    __device__ __forceinline__ T invD2() const { return invD * invD; }
    __device__ __forceinline__ T Bn() const { return ems * cs2 - es * sn2; }                  // B_k D_k^2
    __device__ __forceinline__ T En(T sinP) const { return sinP * 0.5 * (es - ems); }         // E_k D_k^2
    __device__ __forceinline__ T A(T sinP, int K) const { return sinP * invD / K; }
    __device__ __forceinline__ T B(T invD2) const { return Bn() * invD2; }
    __device__ __forceinline__ T C(int K) const { return invD / K; }
    __device__ __forceinline__ T E(T sinP, T invD2) const { return En(sinP) * invD2; }
};

// ---- combine: the new plaquette from ysum = sum_k y_k, the site's log J from si = sum_k 1 / D_k
template <typename T> __device__ __forceinline__ T mix_new_plaq(T ysum, int K, T t) { return ft_wrap(ysum / K + t); }
__device__ __forceinline__ double mix_logj(double si, int K) { return log(si) - log((double)K); }

// ---- adjoint at a site: gd = dL/dP' (the site's link gradient), cbr = dL/dlogJ / sum_k 1/D_k, csum = sum_k C_k, esum = sum_k E_k
template <typename T> struct MixAdjoint {
    T gd, cbr, csum, esum;
    __device__ __forceinline__ MixAdjoint(T gd_, T cbr_, T csum_, T esum_) : gd(gd_), cbr(cbr_), csum(csum_), esum(esum_) {}
    // the tuned kernels: from the stash record tc[4 k ..] = A_k B_k C_k E_k and cb = dL/dlogJ; 1 / (K csum) by v_rcp_f64 and two
    // correction steps (within an ulp of the quotient)
    __device__ __forceinline__ MixAdjoint(double gd_, double cb, const double* tc, int K) : gd(gd_) {
        csum = 0.0; esum = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) { csum += tc[4 * k + 2]; esum += tc[4 * k + 3]; }
        const double tsum = K * csum;                                    // sum_k 1 / D_k
        double rs = __builtin_amdgcn_rcp(tsum);
        rs = fma(fma(-tsum, rs, 1.0), rs, rs);
        rs = fma(fma(-tsum, rs, 1.0), rs, rs);
        cbr = cb * rs;
    }
    __device__ __forceinline__ T gs(T Ak, T Bk) const { return gd * Ak + cbr * Bk; }                 // dL/ds_k; dL/dt = gd
    // the site's own part of dL/dP, through the link and through log J; dir_onto: summed from the left, flow_generic.hip's order
    __device__ __forceinline__ T dir() const { return gd * (csum - 1.0) - cbr * esum; }
    __device__ __forceinline__ T dir_onto(T g) const { return g + gd * (csum - 1.0) - cbr * esum; }
};

// ---- inverse: solve mean_k y_k(x) = target on [-pi, pi] by safeguarded Newton from x = target (s ~ 0: identity).  The map is
// monotone with derivative mean_k 1 / D_k; a step that leaves the bracket becomes its midpoint; the loop ends at |error| <= tol
// or where the iterate no longer moves (the reference bisects to a global 1e-6).  es_of(k) hands over e^{+-s_k}, formed
// once or per iteration as the caller can afford.  Returns the root; fp = mean_k 1 / D_k there (log J of the inverse = -log fp).
// A component is ft_round_pm_pi(2 atan(.)) here: ft_wrap_pm_pi's rounding, so that the loop solves the map the forward rounds,
// without its move of pi to -pi.  Where e^{s} tan(x/2) is beyond ~1e16 the atan rounds to pi/2 exactly; read as -pi the error
// changes sign, the bracket closes on the wrong side and the root is lost (met with s = 10 at a target 2e-13 below pi: the
// start itself saturates, the loop ended at pi, 4.7e-9 off).  Unwrapped, the mean is monotone on [-pi, pi].
struct ExpPair { double es, ems; };
template <typename EsOf>
__device__ __forceinline__ double mix_inverse(double target, int K, double tol, EsOf es_of, double& fp) {
    double lo = -FT_PI, hi = FT_PI, xs = target;
    fp = 1.0;
    bool done = false;
    for (int it = 0; it < 200 && !done; ++it) {
        double sn, cs, f = 0.0;
        ft_sincos(xs / 2, &sn, &cs);
        const double th = sn / cs;
        fp = 0.0;
        for (int k = 0; k < K; ++k) {
            const ExpPair e = es_of(k);
            f += ft_round_pm_pi(2 * ft_atan(e.es * th));
            fp += 1.0 / (e.ems * cs * cs + e.es * sn * sn);
        }
        f /= K; fp /= K;
        const double err = target - f;
        if (fabs(err) <= tol) { done = true; break; }
        if (err > 0) lo = xs; else hi = xs;
        double xn = xs + err / fp;
        if (!(xn > lo && xn < hi)) xn = 0.5 * (lo + hi);
        if (xn == xs) done = true;
        xs = xn;
    }
    return xs;
}

}  // namespace fthmc_flow
