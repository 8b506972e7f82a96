// Dual numbers (value, tangent) for the second-order path: the plain kernels of flow_generic.hip instantiated on Dual run the
// first-order backward on x + eps g, and the eps parts of its outputs are the Hessian-vector product H g and the mixed
// derivative d/dw <g, F> (fthmc_ft_force_vjp, api.hip).  Every helper the plain kernels call has an overload here.  Value parts
// go through the double helpers themselves (common.h, flow_common.h), so they are the numbers of the double instance of the same
// expression in the same caller, bit for bit (from one caller to another a sum of products may round differently in its last
// bit, on double as on Dual: flow_transform.h); tangent parts are the analytic derivatives torch's autograd takes of the same
// functions: the remainders (ft_wrap, ft_wrap_pm_pi) pass the tangent through, relu'' = leaky_relu'' = 0,
// silu'' = sigma' (2 + z (1 - 2 sigma)), tanh'' = -2 t (1 - t^2).  tests/test_dual_math_gpu.py pins every overload: values against the
// double helpers bit for bit, tangents against the closed-form derivatives within bounds traced through the expressions below.
#pragma once
#include "flow_common.h"

namespace fthmc {

struct alignas(16) Dual {
    double v, t;
    Dual() = default;
    __host__ __device__ constexpr Dual(double v_) : v(v_), t(0.0) {}
    __host__ __device__ constexpr Dual(double v_, double t_) : v(v_), t(t_) {}
};

__device__ __forceinline__ Dual operator-(Dual a) { return Dual(-a.v, -a.t); }
__device__ __forceinline__ Dual operator+(Dual a, Dual b) { return Dual(a.v + b.v, a.t + b.t); }
__device__ __forceinline__ Dual operator+(Dual a, double b) { return Dual(a.v + b, a.t); }
__device__ __forceinline__ Dual operator+(double a, Dual b) { return Dual(a + b.v, b.t); }
__device__ __forceinline__ Dual operator-(Dual a, Dual b) { return Dual(a.v - b.v, a.t - b.t); }
__device__ __forceinline__ Dual operator-(Dual a, double b) { return Dual(a.v - b, a.t); }
__device__ __forceinline__ Dual operator-(double a, Dual b) { return Dual(a - b.v, -b.t); }
__device__ __forceinline__ Dual operator*(Dual a, Dual b) { return Dual(a.v * b.v, ::fma(a.t, b.v, a.v * b.t)); }
__device__ __forceinline__ Dual operator*(Dual a, double b) { return Dual(a.v * b, a.t * b); }
__device__ __forceinline__ Dual operator*(double a, Dual b) { return Dual(a * b.v, a * b.t); }
__device__ __forceinline__ Dual operator/(Dual a, Dual b) {
    const double q = a.v / b.v;
    return Dual(q, (a.t - q * b.t) / b.v);
}
__device__ __forceinline__ Dual operator/(Dual a, double b) { return Dual(a.v / b, a.t / b); }
__device__ __forceinline__ Dual operator/(double a, Dual b) {
    const double q = a / b.v;
    return Dual(q, -q * b.t / b.v);
}
__device__ __forceinline__ Dual& operator+=(Dual& a, Dual b) { a = a + b; return a; }
__device__ __forceinline__ Dual& operator*=(Dual& a, Dual b) { a = a * b; return a; }

// a b + c with a constant weight (the convolutions) and with two dual factors (the weight gradients)
__device__ __forceinline__ Dual fma(double a, Dual b, Dual c) { return Dual(::fma(a, b.v, c.v), ::fma(a, b.t, c.t)); }
__device__ __forceinline__ Dual fma(Dual a, Dual b, Dual c) { return Dual(::fma(a.v, b.v, c.v), ::fma(a.t, b.v, ::fma(a.v, b.t, c.t))); }

__device__ __forceinline__ Dual log(Dual a) { return Dual(::log(a.v), a.t / a.v); }
__device__ __forceinline__ Dual tanh(Dual a) { const double y = ::tanh(a.v); return Dual(y, (1.0 - y * y) * a.t); }

__device__ __forceinline__ Dual ft_wrap(Dual a) { return Dual(::ft_wrap(a.v), a.t); }
__device__ __forceinline__ Dual ft_wrap_pm_pi(Dual a) { return Dual(::ft_wrap_pm_pi(a.v), a.t); }
__device__ __forceinline__ void ft_sincos(Dual a, Dual* sn, Dual* cs) {
    double s, c;
    ::ft_sincos(a.v, &s, &c);
    *sn = Dual(s, c * a.t);
    *cs = Dual(c, -s * a.t);
}
__device__ __forceinline__ Dual ft_exp(Dual a) { const double e = fthmc_flow::ft_exp(a.v); return Dual(e, e * a.t); }
__device__ __forceinline__ Dual ft_rcp(Dual a) { const double r = fthmc_flow::ft_rcp(a.v); return Dual(r, -(r * r) * a.t); }
__device__ __forceinline__ Dual ft_atan(Dual a) { return Dual(::ft_atan(a.v), a.t / ::fma(a.v, a.v, 1.0)); }

// h = act(z) and d = act'(z), each with its tangent (act'(z) z', act''(z) z')
__device__ __forceinline__ void act_eval(Dual z, int act, Dual& h, Dual& d) {
    double hv, dv, d2 = 0.0;
    fthmc_flow::act_eval(z.v, act, hv, dv);
    if (act == FTHMC_ACT_SILU) {
        const double sg = fthmc_flow::ft_sigmoid(z.v);
        d2 = sg * (1.0 - sg) * ::fma(z.v, 1.0 - 2.0 * sg, 2.0);   // silu'' = sigma' (2 + z (1 - 2 sigma))
    }
    h = Dual(hv, dv * z.t);
    d = Dual(dv, d2 * z.t);
}

// the block sums of value and tangent, each in ft_block_sum's fixed order (the weight gradients, k_gen_conv_bwd_w)
__device__ __forceinline__ Dual ft_block_sum(Dual a, double* red) {
    const double v = ::ft_block_sum(a.v, red);
    return Dual(v, ::ft_block_sum(a.t, red));
}

}  // namespace fthmc
