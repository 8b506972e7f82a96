"""The dual-number overloads of csrc/dual.h and the Dual instances of the tan-mixture transform (csrc/flow_transform.h), pinned
one by one: the arithmetic under the second-order sweeps (fthmc_ft_force_vjp, fthmc_ft_action_vjp, fthmc_train_force_grad).

tests/hip/device_probe.hip (probe_dual) applies each overload as the headers define it, elementwise to arrays of (value, tangent)
pairs.  What is asserted:
  values     bit-equal to the double helper on the same inputs (probe_math of tests/test_device_math_gpu.py where it has the op,
             the double instance evaluated next to the Dual one otherwise): dual.h, "value parts go through the double helpers
             themselves";
  pass-throughs  ft_wrap / ft_wrap_pm_pi hand the tangent through bit for bit; relu'' = leaky_relu'' = 0 exactly and their h.t is
             the product act'(z) t bit for bit (z = +-0 and subnormal z included);
  every other tangent  against the true derivative in mpmath (40 digits), contracted with the input tangents, within a bound that is
             DERIVED per point and never read off the device.

The derivation, once for all tests (class E, class Du): the header's expression is traced in mpmath on pairs (v, e), v the
expression's value in exact arithmetic at the exact inputs and e a bound on |device - v|.  A correctly rounded +, -, *, /, fma adds
u (|v| + e) with u = 2^-53 (half an ulp; a contraction into an FMA only removes a rounding); a product propagates
|a| e_b + |b| e_a + e_a e_b, a quotient (e_a + |q| e_b) / (|b| - e_b); a helper propagates its argument's e through a bound on its
slope and adds its own stated error, in ulps <= 2^-52 |v|: ft_exp 1.5, ft_rcp 1, ft_atan 2, ft_sincos 2.5 of max(|v|, 2^-26),
ft_sigmoid 3 + 0.21 max(0, -z log2 e), silu' (3 + ...)(1 + |z|) + 2 of max(|silu'|, sigma) (flow_common.h / common.h, the bounds
tests/test_device_math_gpu.py enforces), ocml's log 3 and tanh 5 (the OpenCL limits it is built to).  Every amplification factor
is thereby evaluated in mpmath at the point: near P = +-pi the bound follows 1 / cs, and at a zero of a derivative (silu'' at
|z| = 2.3994, the sin P terms at P = 0, +-pi, 1 - tanh^2 at large |z|) it stays the sum of the cancelling terms' errors -- the
scale there is the terms', not the result's.  The trace's v is the derivative only if the header's formula is right, so the
reference is NOT the trace: it is the closed form written out in each test, and each test also asserts that trace and closed form
agree to 1e-30 of the terms' scale, which checks the trace itself.

Observed on an MI355X (pytest -s prints them), worst tangent error as a fraction of the derived bound: * 0.97, / 0.79,
double / Dual 0.76, the fmas 0.98 / 0.96, log 0.96, tanh 0.54, sincos 0.37, exp 0.73, rcp 0.53, atan 0.93, silu' 0.24, silu'' 0.43,
the component's y 0.21, D 0.17, 1 / D 0.12, A .. E 0.10 .. 0.12, the adjoint's gs 0.87, dir_onto 0.90: no tangent misses its bound,
and the arithmetic's bounds (1 .. 3 ulp of the result at most points) leave no room for more than the roundings counted.

One statement and the device disagreed, and the statement was corrected (csrc/flow_transform.h, csrc/dual.h): "value parts ... are
the numbers of the double instances", with flow_transform.h's "results are pinned bit for bit", holds for the double instance of
the same expression in the same caller -- the Dual values here equal the double ones formed next to them in every bit, and the
forward form (y, D, 1 / D alone) equals probe_math's composite -- but not from one caller to another: where the caller also forms
Bn = e^-s cs^2 - e^s sn^2, as a backward stage does, the compiler fuses the other product of D = e^-s cs^2 + e^s sn^2 into the
FMA, and D differs from the forward form's in the last bit at 78 of the 792 points here (1 ulp; the test allows the 2 ulp that two
such forms can differ by, derived there).  On double as on Dual, so nothing in dual.h causes it and no kernel was changed."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest
import torch  # noqa: F401  (before the probe: its libamdhip64 is the process's one HIP runtime)

import test_device_math_gpu as M
from gpu_support import module_defaults
from test_device_math_gpu import probe  # noqa: F401  (the module-scoped fixture that builds and loads the probe)

pytestmark = pytest.mark.gpu
_defaults = module_defaults()

mpmath = pytest.importorskip('mpmath')
mpmath.mp.dps = 40
mpf = mpmath.mpf

(D_MUL, D_DIV_DD, D_DIV_SD, D_FMA_SDD, D_FMA_DDD, D_LOG, D_TANH, D_WRAP, D_WRAP_PM_PI, D_SINCOS, D_EXP, D_RCP, D_ATAN, D_ACT,
 D_MIXFWD, D_MIXBWD, D_NEW_PLAQ, D_ADJOINT, D_NOPS) = range(19)
NIN = {D_MUL: 4, D_DIV_DD: 4, D_DIV_SD: 4, D_MIXFWD: 4, D_MIXBWD: 4, D_NEW_PLAQ: 4, D_FMA_SDD: 6, D_FMA_DDD: 6, D_ADJOINT: 14}
NOUT = {D_SINCOS: 4, D_ACT: 4, D_LOG: 3, D_TANH: 3, D_NEW_PLAQ: 3, D_MIXFWD: 9, D_MIXBWD: 24, D_ADJOINT: 6}
_D = ctypes.POINTER(ctypes.c_double)
S0 = (2.0, 5.0, 10.0, 20.0)                                # steep_fixture.S0: the |s| of the steep flows


@pytest.fixture(scope='module')
def dprobe(probe):  # noqa: F811
    probe.probe_dual.argtypes = [ctypes.c_int] * 3 + [_D, ctypes.c_int, _D, ctypes.c_int, ctypes.c_int]
    assert probe.probe_dual_nops() == D_NOPS
    return probe


def rund(lib, op, planes, act=M.SILU, K=2):
    """the output planes of one probe_dual op over the input planes (arrays of equal length)"""
    planes = [np.ascontiguousarray(p, dtype=np.float64) for p in planes]
    n = len(planes[0])
    assert len(planes) == NIN.get(op, 2) and all(len(p) == n for p in planes)
    inp = np.ascontiguousarray(np.stack(planes))
    out = np.full((NOUT.get(op, 2), n), np.nan)
    rc = lib.probe_dual(op, act, K, inp.ctypes.data_as(_D), len(planes), out.ctypes.data_as(_D), out.shape[0], n)
    assert rc == 0, f'probe_dual({op}): HIP error {rc}'
    return list(out)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def tangents(g, n, lo=-8.0, hi=8.0):
    """both signs, magnitudes 1e-8 .. 1e8"""
    return g.choice([-1.0, 1.0], n) * 10.0 ** g.uniform(lo, hi, n)


# ----------------------------------------------------------------------------------------------------------------- the derivation
U = mpf(2) ** -53
TINY = mpf(2) ** -1075                                      # half the smallest subnormal: the rounding of a result that underflows


def _pow2(x):
    return x != 0 and math.frexp(float(x))[0] in (0.5, -0.5)


class E:
    """a device quantity: v = its expression in exact arithmetic at the exact inputs, e >= |device - v|"""
    __slots__ = ('v', 'e')

    def __init__(self, v, e=0):
        self.v, self.e = mpf(v), mpf(e)

    @staticmethod
    def of(x):
        return x if isinstance(x, E) else E(x)

    @staticmethod
    def rnd(v, e, half_ulps=1):
        return E(v, e + half_ulps * U * (abs(v) + e) + TINY)

    def __neg__(self):
        return E(-self.v, self.e)

    def __add__(self, o):
        o = E.of(o)
        return E.rnd(self.v + o.v, self.e + o.e)
    __radd__ = __add__

    def __sub__(self, o):
        o = E.of(o)
        return E.rnd(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return E.of(o) - self

    def __mul__(self, o):
        if not isinstance(o, E) and _pow2(o):                                 # a scaling by a power of two: exact
            return E(self.v * o, self.e * abs(o))
        o = E.of(o)
        return E.rnd(self.v * o.v, abs(self.v) * o.e + abs(o.v) * self.e + self.e * o.e)
    __rmul__ = __mul__

    def __truediv__(self, o):
        if not isinstance(o, E) and _pow2(o):
            return E(self.v / o, self.e / abs(o))
        o = E.of(o)
        assert abs(o.v) > o.e
        q = self.v / o.v
        return E.rnd(q, (self.e + abs(q) * o.e) / (abs(o.v) - o.e))

    def __rtruediv__(self, o):
        return E.of(o) / self


def fma(a, b, c):
    a, b, c = E.of(a), E.of(b), E.of(c)
    return E.rnd(a.v * b.v + c.v, abs(a.v) * b.e + abs(b.v) * a.e + a.e * b.e + c.e)


def h_exp(a):                                               # ft_exp: 1.5 ulp
    v = mpmath.exp(a.v)
    return E.rnd(v, v * mpmath.expm1(a.e), 3)


def h_rcp(a):                                               # ft_rcp: 1 ulp
    assert abs(a.v) > a.e
    return E.rnd(1 / a.v, a.e / (abs(a.v) * (abs(a.v) - a.e)), 2)


def h_atan(a):                                              # ft_atan: 2 ulp; slope 1 / (1 + x^2) at the nearest point of the range
    lo = max(abs(a.v) - a.e, mpf(0))
    return E.rnd(mpmath.atan(a.v), a.e / (1 + lo * lo), 4)


def h_sincos(a):                                            # ft_sincos: 2.5 ulp of max(|result|, 2^-26); slopes <= 1
    out = []
    for f in (mpmath.sin, mpmath.cos):
        v = f(a.v)
        out.append(E(v, a.e + 5 * U * max(abs(v) + a.e, mpf(2) ** -26)))
    return out


def h_sigmoid(z):                                           # ft_sigmoid at an exact z: sigmoid_bound(z) ulp
    v = 1 / (1 + mpmath.exp(-mpf(z)))
    return E(v, 2 * U * float(M.sigmoid_bound(z)) * v)


def h_ocml(f, a, ulps):                                     # ::log, ::tanh at an exact argument
    v = f(a.v)
    return E(v, 2 * U * ulps * abs(v))


class Du:
    """csrc/dual.h over E, overload by overload"""
    __slots__ = ('v', 't')

    def __init__(self, v, t=0):
        self.v, self.t = E.of(v), E.of(t)

    def __neg__(self):
        return Du(-self.v, -self.t)

    def __add__(self, o):
        return Du(self.v + o.v, self.t + o.t) if isinstance(o, Du) else Du(self.v + o, self.t)

    def __radd__(self, o):
        return Du(o + self.v, self.t)

    def __sub__(self, o):
        return Du(self.v - o.v, self.t - o.t) if isinstance(o, Du) else Du(self.v - o, self.t)

    def __rsub__(self, o):
        return Du(o - self.v, -self.t)

    def __mul__(self, o):
        if isinstance(o, Du):
            return Du(self.v * o.v, fma(self.t, o.v, self.v * o.t))
        return Du(self.v * o, self.t * o)
    __rmul__ = __mul__                                      # double * Dual: (a b.v, a b.t)

    def __truediv__(self, o):
        if isinstance(o, Du):
            q = self.v / o.v
            return Du(q, (self.t - q * o.t) / o.v)
        return Du(self.v / o, self.t / o)

    def __rtruediv__(self, o):
        q = E.of(o) / self.v
        return Du(q, (-q) * self.t / self.v)


def du_fma(a, b, c):
    if isinstance(a, Du):
        return Du(fma(a.v, b.v, c.v), fma(a.t, b.v, fma(a.v, b.t, c.t)))
    return Du(fma(a, b.v, c.v), fma(a, b.t, c.t))


def du_sincos(a):
    s, c = h_sincos(a.v)
    return Du(s, c * a.t), Du(c, (-s) * a.t)


def du_exp(a):
    e = h_exp(a.v)
    return Du(e, e * a.t)


def du_rcp(a):
    r = h_rcp(a.v)
    return Du(r, (-(r * r)) * a.t)


def du_atan(a):
    return Du(h_atan(a.v), a.t / fma(a.v, a.v, 1))


def check(dev, ref, trace, what, x, floor=0.0):
    """|dev - ref| <= the trace's bound (times 1 + 2^-30: the reference's own 40 digits, with room), and the trace's value is the
    closed form; returns error / bound"""
    ref = mpf(ref)
    scale = abs(ref) + trace.e / U
    assert abs(trace.v - ref) <= mpf(10) ** -30 * scale, (what, x, 'the trace is not the closed form', trace.v, ref)
    bound = trace.e * (1 + mpf(2) ** -30) + floor
    err = abs(mpf(float(dev)) - ref)
    assert np.isfinite(dev) and err <= bound, (what, x, f'device {float(dev)!r}, reference {float(ref)!r}, error {float(err):.3e}, '
                                                        f'bound {float(bound):.3e} = {mpmath.nstr(bound / (2 * U * max(abs(ref), mpf(10) ** -300)), 4)} ulp')
    return float(err / bound) if bound else 0.0


def exact_fma(a, b, c):
    """the correctly rounded a b + c"""
    return np.array([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a, b, c)])


# ----------------------------------------------------------------------------------------------------------------- arithmetic
def test_products_quotients_and_fmas(dprobe):
    """operator*(Dual, Dual), operator/(Dual, Dual), operator/(double, Dual), fma(double, Dual, Dual), fma(Dual, Dual, Dual).

    Values: IEEE a b, a / b, fma, bit for bit.  Tangents, closed forms: (a b)' = a' b + a b'; (a / b)' = a' / b - a b' / b^2;
    (c / b)' = -c b' / b^2; (a b + c)' with a constant a: a b' + c', with a dual a: a' b + a b' + c'.  Bounds by the trace of the
    header: the product's tangent is one product and one fma (u |a b'| + u |t|); the quotient's (a.t - q b.t) / b.v carries q's
    rounding times |b'|, the product's, the difference's and the division's; divisors down to 1e-12 (cs at P near +-pi) and both
    signs of everything."""
    g = M.rng(31)
    n = 2000
    mag = lambda: g.choice([-1.0, 1.0], n) * 10.0 ** g.uniform(-3, 3, n)
    a, b, c = mag(), mag(), mag()
    b[:400] = g.choice([-1.0, 1.0], 400) * 10.0 ** g.uniform(-12, -6, 400)
    at, bt, ct = tangents(g, n), tangents(g, n), tangents(g, n)
    worst = {}
    for op, name in ((D_MUL, 'mul'), (D_DIV_DD, 'div'), (D_DIV_SD, 'sdiv'), (D_FMA_SDD, 'sfma'), (D_FMA_DDD, 'fma')):
        planes = [a, at, b, bt] + ([c, ct] if op in (D_FMA_SDD, D_FMA_DDD) else [])
        v, t = rund(dprobe, op, planes)
        want = {D_MUL: a * b, D_DIV_DD: a / b, D_DIV_SD: a / b}.get(op)
        assert same(v, exact_fma(a, b, c) if want is None else want), name
        w = 0.0
        for i in range(n):
            A, B, Cc = Du(a[i], at[i]), Du(b[i], bt[i]), Du(c[i], ct[i])
            ma, mb, mat, mbt, mct = mpf(a[i]), mpf(b[i]), mpf(at[i]), mpf(bt[i]), mpf(ct[i])
            if op == D_MUL:
                tr, ref = A * B, mat * mb + ma * mbt
            elif op == D_DIV_DD:
                tr, ref = A / B, mat / mb - ma * mbt / mb ** 2
            elif op == D_DIV_SD:
                tr, ref = a[i] / B, -ma * mbt / mb ** 2
            elif op == D_FMA_SDD:
                tr, ref = du_fma(E(a[i]), B, Cc), ma * mbt + mct
            else:
                tr, ref = du_fma(A, B, Cc), mat * mb + ma * mbt + mct
            w = max(w, check(t[i], ref, tr.t, name, (a[i], at[i], b[i], bt[i], c[i], ct[i])))
        worst[name] = round(w, 3)
    print('tangent error / derived bound:', worst)


def test_log_and_tanh(dprobe):
    """log(Dual) = (log a, a' / a): one division.  tanh(Dual) = (y, (1 - y y) a') with y = tanh(a) within ocml's 5 ulp: 1 - y^2
    carries 2 |y| e_y + u y^2 + u |1 - y^2| absolutely, which is all that is left of it where tanh saturates (|a| > 19: y = 1,
    tangent 0 against a true 4 e^-2|a| a', inside the bound).  Values: the double function next to it, bit for bit, and within
    ocml's 3 / 5 ulp of mpmath."""
    g = M.rng(32)
    n = 1500
    a = np.concatenate([10.0 ** g.uniform(-150, 150, n // 2), g.uniform(0.5, 2.0, n // 2), M.neighbours(1.0, 4)])
    at = tangents(g, len(a))
    v, t, vd = rund(dprobe, D_LOG, [a, at])
    assert same(v, vd)
    w = 0.0
    for i in range(len(a)):
        tr = Du(h_ocml(mpmath.log, E(a[i]), 3), E(at[i]) / E(a[i]))
        assert abs(mpf(float(v[i])) - tr.v.v) <= tr.v.e + 2 * U * 3 * mpf(2) ** -1022, ('log value', a[i])
        w = max(w, check(t[i], mpf(at[i]) / mpf(a[i]), tr.t, 'log', (a[i], at[i])))
    a = np.concatenate([np.linspace(-22.0, 22.0, 1001), g.normal(0, 2, 500), [0.0, -0.0, 1e-300, -1e-300, 1e-9, 40.0, -40.0, 700.0]])
    at = tangents(g, len(a))
    v, t, vd = rund(dprobe, D_TANH, [a, at])
    assert same(v, vd)
    w2 = 0.0
    for i in range(len(a)):
        y = h_ocml(mpmath.tanh, E(a[i]), 5)
        assert abs(mpf(float(v[i])) - y.v) <= y.e, ('tanh value', a[i])
        w2 = max(w2, check(t[i], (1 - mpmath.tanh(mpf(a[i])) ** 2) * mpf(at[i]), (1 - y * y) * E(at[i]), 'tanh', (a[i], at[i])))
    print(f'tangent error / derived bound: log {w:.3f}, tanh {w2:.3f}')


# ----------------------------------------------------------------------------------------------------------------- pass-throughs
def test_wraps_pass_the_tangent_through(dprobe):
    """ft_wrap(Dual), ft_wrap_pm_pi(Dual): the value of the double helper, the tangent handed through bit for bit (the remainder has
    slope 1 away from its jump), on the wrap's grids and at neighbours(+-pi)"""
    g = M.rng(33)
    x = M.wrap_inputs()
    x = x[np.isfinite(x)]
    t = tangents(g, len(x))
    v, tt = rund(dprobe, D_WRAP, [x, t])
    assert same(v, M.run(dprobe, M.P_WRAP, x)[0]) and same(tt, t)
    x = np.concatenate([g.uniform(-np.pi, np.pi, 3000), M.neighbours(M.FT_PI, 12), M.neighbours(-M.FT_PI, 12), [0.0, -0.0], M.SUBN,
                        g.uniform(-2 * np.pi, 2 * np.pi, 500)])
    t = tangents(g, len(x))
    v, tt = rund(dprobe, D_WRAP_PM_PI, [x, t])
    assert same(v, M.run(dprobe, M.P_WRAP_PM_PI, x)[0]) and same(tt, t)


def test_relu_and_leaky_relu_have_no_second_derivative(dprobe):
    """act_eval(Dual), relu and leaky_relu: h and d are the double act_eval's, d.t = 0 exactly, h.t = act'(z) t as one product, bit
    for bit -- at z = +-0 (act' = 0 / 0.01: the side z > 0 is false on) and at subnormal z too"""
    g = M.rng(34)
    z = np.concatenate([M.sigmoid_inputs()[::200], [0.0, -0.0], M.SUBN, M.neighbours(0.0, 4)])
    t = tangents(g, len(z))
    for act in (M.RELU, M.LEAKY):
        hv, ht, dv, dt = rund(dprobe, D_ACT, [z, t], act=act)
        h, d, _ = M.run(dprobe, M.P_ACT, z, act=act)
        assert same(hv, h) and same(dv, d), act
        assert np.all(dt == 0.0), (act, z[dt != 0.0][:4])
        assert same(ht, d * t), (act, z[bits(ht) != bits(d * t)][:4])
        assert np.all(d[z <= 0] == (0.0 if act == M.RELU else 0.01)) and np.all(d[z > 0] == 1.0)


# ----------------------------------------------------------------------------------------------------------------- helpers
def test_sincos_exp_rcp_atan_tangents(dprobe):
    """ft_sincos(Dual): (sin)' = cs a', (cos)' = -sn a', one product of a 2.5-ulp value (of max(|.|, 2^-26): at a zero of the
    derivative, a = k pi / 2, the scale is 2^-26 |a'|).  ft_exp(Dual): e a', 1.5 ulp and one product.  ft_rcp(Dual): -(r r) a'
    against -a' / a^2: r's 1 ulp twice, two products.  ft_atan(Dual): a' / fma(a, a, 1) against a' / (1 + a^2): an fma and a division.
    Values: probe_math's, bit for bit."""
    g = M.rng(35)
    ks = [float(mpf(k) * mpmath.pi / 2) for k in range(-4, 5)]
    a = np.concatenate([g.uniform(-2 * np.pi, 2 * np.pi, 1500), [0.0, -0.0], M.SUBN] + [M.neighbours(k, 3) for k in ks])
    at = tangents(g, len(a))
    sv, st, cv, ct = rund(dprobe, D_SINCOS, [a, at])
    s0, c0, _ = M.run(dprobe, M.P_SINCOS, a)
    assert same(sv, s0) and same(cv, c0)
    ws = 0.0
    for i in range(len(a)):
        sn, cs = du_sincos(Du(a[i], at[i]))
        ws = max(ws, check(st[i], mpmath.cos(mpf(a[i])) * mpf(at[i]), sn.t, 'sin', (a[i], at[i])),
                 check(ct[i], -mpmath.sin(mpf(a[i])) * mpf(at[i]), cs.t, 'cos', (a[i], at[i])))
    a = np.concatenate([np.linspace(-40.0, 40.0, 1001), g.uniform(-700, 600, 500), [0.0, -0.0, 1e-300], M.neighbours(20.0, 2)])
    at = tangents(g, len(a))
    v, t = rund(dprobe, D_EXP, [a, at])
    assert same(v, M.run(dprobe, M.P_EXP, a)[0])
    we = max(check(t[i], mpmath.exp(mpf(a[i])) * mpf(at[i]), du_exp(Du(a[i], at[i])).t, 'exp', (a[i], at[i])) for i in range(len(a)))
    a = np.concatenate([g.choice([-1.0, 1.0], 1200) * np.exp2(g.uniform(-100, 100, 1200)), g.uniform(0.5, 2.0, 300), M.neighbours(1.0, 4)])
    at = tangents(g, len(a))
    v, t = rund(dprobe, D_RCP, [a, at])
    assert same(v, M.run(dprobe, M.P_RCP, a)[0])
    wr = max(check(t[i], -mpf(at[i]) / mpf(a[i]) ** 2, du_rcp(Du(a[i], at[i])).t, 'rcp', (a[i], at[i])) for i in range(len(a)))
    a = np.concatenate([g.uniform(-4, 4, 1000), g.choice([-1.0, 1.0], 500) * np.exp(g.uniform(-30, 60, 500)), M.neighbours(1.0, 6),
                        M.neighbours(-1.0, 6), [0.0, -0.0, 1e-8, 1e8, -1e8, 1e100]])
    at = tangents(g, len(a))
    v, t = rund(dprobe, D_ATAN, [a, at])
    assert same(v, M.run(dprobe, M.P_ATAN, a)[0])
    wa = max(check(t[i], mpf(at[i]) / (1 + mpf(a[i]) ** 2), du_atan(Du(a[i], at[i])).t, 'atan', (a[i], at[i])) for i in range(len(a)))
    print(f'tangent error / derived bound: sincos {ws:.3f}, exp {we:.3f}, rcp {wr:.3f}, atan {wa:.3f}')


def test_silu_first_and_second_derivative(dprobe):
    """act_eval(Dual), silu: h.t = silu'(z) z' with the double act_eval's silu' -- within (b (1 + |z|) + 2) ulp of max(|silu'|, sg),
    b = sigmoid_bound(z), the bound test_activation_forms_agree_and_silu_is_accurate derives and enforces -- and one product.
    d.t = silu''(z) z', silu'' = sg (1 - sg) (2 + z (1 - 2 sg)) evaluated as (sg (1 - sg)) fma(z, 1 - 2 sg, 2): the trace carries sg's
    b ulp through 1 - sg (slope 1), 1 - 2 sg (slope 2, then |z|), the two products and the fma, so the bound is about
    (2 b + 3 + (2 b + 2) |z| / |2 + z (1 - 2 sg)|) ulp of silu'' -- at the zeros of silu'' (z tanh(z / 2) = 2, |z| = 2.3994) the
    bracket's terms cancel and the bound stays sg (1 - sg) (2 b |z| + 1) ulp(2): the scale there is 2 sigma', not silu''.  |z| <= 40
    and the subnormals; values h, d: the double act_eval's, bit for bit."""
    g = M.rng(36)
    z0 = float(mpmath.findroot(lambda z: z * mpmath.tanh(z / 2) - 2, 2.4))
    assert abs(z0 - 2.3994) < 1e-4
    z = np.concatenate([np.linspace(-40.0, 40.0, 1201), g.normal(0, 3, 600), [0.0, -0.0], M.SUBN, M.neighbours(z0, 6), M.neighbours(-z0, 6),
                        M.neighbours(-2.3993572805154676, 3)])
    z = z[np.abs(z) <= 40.0]
    t = tangents(g, len(z))
    hv, ht, dv, dt = rund(dprobe, D_ACT, [z, t], act=M.SILU)
    h, d, _ = M.run(dprobe, M.P_ACT, z, act=M.SILU)
    assert same(hv, h) and same(dv, d)
    w1 = w2 = 0.0
    for i in range(len(z)):
        zi, sg = mpf(z[i]), h_sigmoid(z[i])
        d1 = sg.v * (1 + zi * (1 - sg.v))
        b = float(M.sigmoid_bound(z[i]))
        d1e = E(d1, 2 * U * (b * (1 + abs(z[i])) + 2) * max(abs(d1), sg.v))
        w1 = max(w1, check(ht[i], d1 * mpf(t[i]), d1e * E(t[i]), "silu'", (z[i], t[i])))
        two_sg = E(2 * sg.v, 2 * sg.e)                                        # 2.0 * sg: exact
        d2 = (sg * (1 - sg)) * fma(E(z[i]), 1 - two_sg, 2)
        ref = sg.v * (1 - sg.v) * (2 + zi * (1 - 2 * sg.v)) * mpf(t[i])
        w2 = max(w2, check(dt[i], ref, d2 * E(t[i]), "silu''", (z[i], t[i])))
    print(f"tangent error / derived bound: silu' {w1:.3f}, silu'' {w2:.3f}")


# ----------------------------------------------------------------------------------------------------------------- the transform
def comp_trace(P, Pt, s, st, K):
    """tests/hip/device_probe.hip comp_fwd<Dual> and comp_bwd<Dual>, i.e. flow_transform.h MixComp<Dual> as flow_generic.hip and
    flow_dual.hip use it, statement by statement: (y, D, invD), (A, C, B, E in the stash forms, B, E in the generic backward's forms)"""
    Pd, sd = Du(P, Pt), Du(s, st)
    sn, cs = du_sincos(0.5 * Pd)                                              # 0.5 P: exact
    sinP = (2.0 * sn) * cs
    es = du_exp(sd)
    ems = du_rcp(es)
    cs2, sn2 = cs * cs, sn * sn
    Dd = ems * cs2 + es * sn2
    invD = du_rcp(Dd)
    y = 2 * du_atan(es * (sn / cs))                                           # the doubling and ft_wrap_pm_pi's tangent: exact
    invD2 = invD * invD
    Bn = ems * cs2 - es * sn2
    En = (sinP * 0.5) * (es - ems)
    return [y, Dd, invD], [sinP * invD / K, invD / K, Bn * invD2, En * invD2, Bn * invD * invD, En * invD * invD]


def comp_closed_forms(P, Pt, s, st, K):
    """d/dP and d/ds of y_k = 2 atan(e^s tan(P/2)), 1 / D_k, A = sin P / (K D), C = 1 / (K D), B = Bn / D^2, E = En / D^2 with
    D = e^-s c^2 + e^s n^2, Bn = e^-s c^2 - e^s n^2 = -dD/ds, En = sin P (e^s - e^-s) / 2 = dD/dP (c, n = cos, sin of P / 2):
        dy/dP = 1 / D, dy/ds = sin P / D;  dBn/dP = -sin P (e^s + e^-s) / 2, dBn/ds = -D;
        dEn/dP = cos P (e^s - e^-s) / 2, dEn/ds = sin P (e^s + e^-s) / 2,
    contracted with (P', s')"""
    P, Pt, s, st = mpf(P), mpf(Pt), mpf(s), mpf(st)
    c, n, e = mpmath.cos(P / 2), mpmath.sin(P / 2), mpmath.exp(s)
    sinP, cosP = mpmath.sin(P), mpmath.cos(P)
    Dv = c * c / e + e * n * n
    Bn, En = c * c / e - e * n * n, sinP * (e - 1 / e) / 2
    dD = En * Pt - Bn * st
    dBn = -sinP * (e + 1 / e) / 2 * Pt - Dv * st
    dEn = cosP * (e - 1 / e) / 2 * Pt + sinP * (e + 1 / e) / 2 * st
    dinv = -dD / Dv ** 2
    dB = dBn / Dv ** 2 - 2 * Bn * dD / Dv ** 3
    dE = dEn / Dv ** 2 - 2 * En * dD / Dv ** 3
    return [Pt / Dv + sinP / Dv * st, dD, dinv], [(cosP * Pt / Dv + sinP * dinv) / K, dinv / K, dB, dE, dB, dE]


FWD_NAMES = ('y', 'D', 'invD')
BWD_NAMES = ('A', 'C', 'B', 'E', 'B (generic)', 'E (generic)')


def test_mixture_component_on_dual_near_the_cut(dprobe):
    """MixComp<Dual> with s in +-{2, 5, 10, 20} and P at +-pi -+ {0, 1e-9, 1e-6}, their nextafter neighbours, +-pi/2, 0 and a few
    random plaquettes; tangents of P and of s of both signs, 1e-8 .. 1e8, and each alone.

    Values: every result bit-equal to MixComp<double> evaluated next to it, and the forward form's y, D, 1 / D bit-equal to
    probe_math's composite.
    Tangents against comp_closed_forms within the bound of comp_trace, the header traced statement by statement.  What the bound
    follows: sn / cs is a dual division by cs = cos(P / 2), 6e-17 at P = fl(pi) and 5e-10 at pi - 1e-9, known to 2.5 ulp of 2^-26
    = 8e-24 absolutely, i.e. to 1.3e-7 / 1.6e-14 relatively: q = tan(P / 2) inherits that, its tangent (sn' - q cs') / cs twice
    that, and atan's 1 / (1 + w^2), w = e^s q, gives both back, so y's tangent ends within about 4 e_cs / |cs| of P' / D + ...,
    not within ulps; the coefficients A .. E do not divide by cs and stay within tens of ulps of their terms (the sin P terms at
    P = 0, +-pi in ulps of their cancelling parts)."""
    g = M.rng(37)
    K = 2
    Ps = []
    for sign in (1.0, -1.0):
        for dlt in (0.0, 1e-9, 1e-6):
            Ps += M.neighbours(sign * (M.FT_PI - dlt), 1 if dlt else 2)
        Ps.append(sign * np.pi / 2)
    Ps += [0.0, 1e-9, -1e-7] + list(g.uniform(-np.pi, np.pi, 6))
    Ps = np.clip(np.array(Ps), -M.FT_PI, M.FT_PI)
    Ss = np.array([sg * s for s in S0 for sg in (1.0, -1.0)])
    PP, SS = (a.ravel() for a in np.meshgrid(Ps, Ss))
    reps = 3
    PP, SS = np.tile(PP, reps), np.tile(SS, reps)
    n = len(PP)
    Pt, St = tangents(g, n), tangents(g, n)
    Pt[n // 3:2 * n // 3:2] = 0.0                                             # d/ds alone
    St[n // 3 + 1:2 * n // 3:2] = 0.0                                         # d/dP alone
    fwd = rund(dprobe, D_MIXFWD, [PP, Pt, SS, St], K=K)
    bwd = rund(dprobe, D_MIXBWD, [PP, Pt, SS, St], K=K)
    for q in range(3):
        assert same(fwd[2 * q], fwd[6 + q]), (FWD_NAMES[q], 'value differs from MixComp<double>', int(np.sum(bits(fwd[2 * q]) != bits(fwd[6 + q]))))
    for q in range(8):
        assert same(bwd[2 * q], bwd[16 + q]), (q, 'value differs from MixComp<double>', int(np.sum(bits(bwd[2 * q]) != bits(bwd[16 + q]))))
    y0, D0, i0 = M.run(dprobe, M.P_COMPOSITE, PP, SS)
    assert same(fwd[0], y0) and same(fwd[2], D0) and same(fwd[4], i0)
    # D where the caller also forms Bn (see the module docstring): the same expression, but which of its two positive products
    # e^-s cs^2, e^s sn^2 is rounded before the sum is the compiler's choice of FMA: u p_1 + u p_2 <= u D <= 1 ulp apart before the
    # final rounding, at most 2 ulp after it
    dD = np.abs(bwd[12] - D0) / np.spacing(D0)
    print(f'D of the backward form against the forward form: {int(np.sum(dD != 0))} of {n} differ, by at most {dD.max():.2f} ulp')
    assert dD.max() <= 2.0, (dD.max(), PP[np.argmax(dD)], SS[np.argmax(dD)])
    wf, wb = [0.0] * 3, [0.0] * 6
    for i in range(n):
        trf, trb = comp_trace(PP[i], Pt[i], SS[i], St[i], K)
        rf, rb = comp_closed_forms(PP[i], Pt[i], SS[i], St[i], K)
        x = (PP[i], Pt[i], SS[i], St[i])
        for q in range(3):
            wf[q] = max(wf[q], check(fwd[2 * q + 1][i], rf[q], trf[q].t, FWD_NAMES[q], x))
        for q in range(6):
            wb[q] = max(wb[q], check(bwd[2 * q + 1][i], rb[q], trb[q].t, BWD_NAMES[q], x))
        for q, k in ((12, 1), (14, 2)):                                       # the backward form's own D', (1 / D)'
            check(bwd[q + 1][i], rf[k], trf[k].t, 'backward ' + FWD_NAMES[k], x)
    print(f'{n} points; tangent error / derived bound:', dict(zip(FWD_NAMES + BWD_NAMES, (round(w, 3) for w in wf + wb))))


def test_new_plaquette_on_dual(dprobe):
    """mix_new_plaq<Dual>(ysum, K, t) = ft_wrap(ysum / K + t): the value of the double instance, the tangent ysum' / K + t' -- a
    correctly rounded division and sum, bit for bit; K = 2 and K = 3"""
    g = M.rng(38)
    n = 3000
    ys = np.concatenate([g.uniform(-3 * np.pi, 3 * np.pi, n - 34), M.neighbours(2 * M.FT_PI, 8), M.neighbours(-2 * M.FT_PI, 8)])
    t = g.uniform(-4, 4, n)
    yt, tt = tangents(g, n), tangents(g, n)
    for K in (2, 3):
        v, tg, vd = rund(dprobe, D_NEW_PLAQ, [ys, yt, t, tt], K=K)
        assert same(v, vd) and same(v, M.run(dprobe, M.P_WRAP, ys / K + t)[0]), K
        assert same(tg, yt / K + tt), K


def test_adjoint_on_dual(dprobe):
    """MixAdjoint<Dual>: gs = gd A_k + cbr B_k and dir_onto(g) = g + gd (csum - 1) - cbr esum, with the inputs of
    test_transform_adjoint_from_stash_coefficients (sum C near 1 in a quarter of the records) and a tangent on every operand.
    Values: MixAdjoint<double> next to it, bit for bit.  Tangents, closed forms: gs' = gd' A + gd A' + cbr' B + cbr B',
    dir' = g' + gd' (csum - 1) + gd csum' - cbr' esum - cbr esum'; bound by the trace: two dual products and a sum for gs; for dir
    the rounding of csum - 1 (u |csum - 1|, times |gd'|), the two dual products and the two sums from the left -- in units of the
    terms, so that the cancellation in csum - 1 is not held against the helper."""
    g = M.rng(39)
    n = 1500
    csum = np.exp(g.uniform(-9.0, 3.0, n))
    near1 = g.random(n) < 0.25
    csum[near1] = 1.0 + g.normal(0, 1e-9, near1.sum())
    wide = lambda: g.normal(0, 1, n) * np.exp(g.uniform(-6, 6, n))
    gd, cbr, esum, Ak, Bk, gg = (wide() for _ in range(6))
    vals = [gd, cbr, csum, esum, Ak, Bk, gg]
    tans = [tangents(g, n) for _ in vals]
    planes = [p for pair in zip(vals, tans) for p in pair]
    gv, gt, dv, dt, gdbl, ddbl = rund(dprobe, D_ADJOINT, planes)
    assert same(gv, gdbl) and same(dv, ddbl)
    wg = wd = 0.0
    for i in range(n):
        d_ = [Du(v[i], t[i]) for v, t in zip(vals, tans)]
        m = [(mpf(v[i]), mpf(t[i])) for v, t in zip(vals, tans)]
        (gd_, gdt), (cb_, cbt), (cs_, cst), (es_, est), (A_, At), (B_, Bt), (_, g_t) = m
        gs = d_[0] * d_[4] + d_[1] * d_[5]
        dr = d_[6] + d_[0] * (d_[2] - 1.0) - d_[1] * d_[3]
        x = tuple(float(v[i]) for v in vals)
        wg = max(wg, check(gt[i], gdt * A_ + gd_ * At + cbt * B_ + cb_ * Bt, gs.t, 'gs', x))
        wd = max(wd, check(dt[i], g_t + gdt * (cs_ - 1) + gd_ * cst - cbt * es_ - cb_ * est, dr.t, 'dir_onto', x))
    print(f'tangent error / derived bound: gs {wg:.3f}, dir_onto {wd:.3f}')
