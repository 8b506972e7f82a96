"""The kernels' hand-written fp64 math (common.h, flow_common.h), the tan-mixture transform they share (flow_transform.h) and
integer index helpers (flow_mfma_common.h), pinned one by one.

Every other GPU test checks whole kernels on random fields, where the inputs at which such code breaks (P near +-pi, the atan fold at
|x| = 1, the exp clamps, large |z| in the sigmoid, reduction boundaries) are rare.  tests/hip/device_probe.hip applies each helper
as the headers define it -- compiled with the kernels' CXXFLAGS -- elementwise to arrays, and this file compares the results with
references of higher precision: numpy.longdouble (x87 80-bit, 64-bit significand) on dense grids, mpmath at 40 digits on the edge
sets.  Errors are in ulps of the correctly rounded result, except near zeros of a result, where the scale is stated per helper.

The bounds are the ones the source comments state; where a comment and the device disagreed the comment (or the helper) was fixed
in the same change, with the reason next to it.
"""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the probe: its libamdhip64 is the process's one HIP runtime, as fthmc_amd/_lib.py does)

from conftest import ROOT
from gpu_support import module_defaults

pytestmark = pytest.mark.gpu
_defaults = module_defaults()

mpmath = pytest.importorskip('mpmath')
mpmath.mp.dps = 40

CSRC = os.path.join(ROOT, 'fthmc_amd', 'csrc')
PROBE = os.path.join(ROOT, 'tests', 'hip', 'libdevice_probe.so')
(P_SIGMOID, P_SIGMOID4, P_EXP, P_EXPN4, P_EXPN2, P_ACT, P_ACT4, P_SINCOS, P_ATAN, P_RCP, P_WRAP, P_WRAP_PM_PI,
 P_REGULARIZE, P_COMPOSITE, P_INVERSE, P_ADJOINT, P_NOPS) = range(17)
SILU, RELU, LEAKY = 0, 1, 2
FT_PI, FT_TWO_PI = 3.14159265358979323846, 6.28318530717958647692
LD = np.longdouble
_I = ctypes.POINTER(ctypes.c_int)
_D = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope='module')
def probe():
    r = subprocess.run(['make', '-C', CSRC, 'probe'], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'warning' not in (r.stdout + r.stderr).lower(), r.stdout[-3000:] + r.stderr[-3000:]
    lib = ctypes.CDLL(PROBE)
    lib.probe_math.argtypes = [ctypes.c_int, ctypes.c_int, _D, _D, _D, _D, _D, ctypes.c_int]
    lib.probe_fdiv.argtypes = [ctypes.c_int, _I, ctypes.c_int]
    lib.probe_wrap_line.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_longlong), _I,
                                    ctypes.c_longlong]
    lib.probe_stash.argtypes = [ctypes.c_int] * 3 + [_I, ctypes.c_int, _I, ctypes.c_int, _I, _I, _I, _I]
    lib.probe_grid_launch.argtypes = [ctypes.c_uint, ctypes.c_uint, _I]
    assert lib.probe_nops() == P_NOPS
    return lib


def _p(a, t=_D):
    return None if a is None else a.ctypes.data_as(t)


def run(lib, op, x, s=None, act=SILU):
    """(o0, o1, o2) of one probe op over x (and s for the composite)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n = len(x)
    pad = (-n) % 4
    xp = np.concatenate([x, np.zeros(pad)]) if pad else x
    sp = None if s is None else np.ascontiguousarray(np.concatenate([s, np.zeros(pad)]) if pad else s, dtype=np.float64)
    o = [np.full(len(xp), np.nan) for _ in range(3)]
    rc = lib.probe_math(op, act, _p(xp), _p(sp), _p(o[0]), _p(o[1]), _p(o[2]), len(xp))
    assert rc == 0, f'probe_math({op}): HIP error {rc}'
    return tuple(a[:n] for a in o)


def ulp(ref):
    """ulp of the fp64 value nearest to ref (longdouble or float), >= the smallest subnormal"""
    return np.abs(np.spacing(np.abs(np.asarray(ref, dtype=np.float64))))


def ulp_err(dev, ref, scale=None):
    """|dev - ref| in ulps of the correctly rounded ref (or of `scale` where given: the scale of a result near its zeros)"""
    d = np.abs(np.asarray(dev, dtype=LD) - np.asarray(ref, dtype=LD))
    u = ulp(ref if scale is None else scale)
    return np.asarray(d / u.astype(LD), dtype=np.float64)


def worst(e, x):
    k = int(np.nanargmax(e))
    return f'max {e[k]:.3f} ulp at x = {x[k]!r}'


def neighbours(c, k=8):
    """c and its k nextafter neighbours on either side"""
    out = [float(c)]
    lo = hi = float(c)
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return out


SUBN = [5e-324, -5e-324, 1e-310, -1e-310, 2.2250738585072009e-308, -2.2250738585072009e-308, 2.2250738585072014e-308]


def rng(seed):
    return np.random.default_rng(seed)


def test_reference_is_extended_precision():
    """the bulk references need a wider significand than fp64"""
    assert np.finfo(np.longdouble).nmant == 63


# ----------------------------------------------------------------------------------------------------------------- sigmoid
def sigmoid_ref(z):
    z = np.asarray(z, dtype=LD)
    return LD(1) / (LD(1) + np.exp(-z))


def sigmoid_bound(z):
    """flow_common.h (FT_SIG_RATIONAL, FT_SIG_LN2_ONE): 3 ulp, plus |n| 2.3e-17 relative where sigma is small (z < 0,
    n = round(-z log2 e)) from the single correctly rounded ln 2 of the reduction -- 0.21 ulp per unit of n (6.6 measured at
    n = 18, where 2.8 + 0.21 n would be 6.58: the base term is taken as 3)"""
    return 3.0 + 0.21 * np.maximum(0.0, -np.asarray(z, dtype=np.float64)) * 1.4426950408889634


def sigmoid_inputs():
    g = rng(1)
    z = np.concatenate([np.linspace(-40.0, 40.0, 400001), g.uniform(-40, 40, 200000), g.normal(0, 3, 100000),
                        np.array([0.0, -0.0] + SUBN)])
    return z


def test_sigmoid_within_its_stated_bound(probe):
    """flow_common.h: ft_sigmoid within sigmoid_bound(z) of the correctly rounded sigmoid over |z| <= 40 (2.8 ulp on z >= 0)"""
    z = sigmoid_inputs()
    sg = run(probe, P_SIGMOID, z)[0]
    e = ulp_err(sg, sigmoid_ref(z))
    assert np.all(e <= sigmoid_bound(z)), worst(e - sigmoid_bound(z), z)
    assert e[z >= 0].max() <= 2.8, worst(e[z >= 0], z[z >= 0])


def test_sigmoid_tails_and_the_magic_rounding_limit(probe):
    """Beyond |z| = 40: -z is clamped at 700 (sigmoid(z < -700) is e^-700-scaled, the correctly rounded tiny number of the clamp);
    large positive z underflows e^-z and gives 1 within the bound -- up to the documented domain of the magic-number rounding
    (FT_SIG_MAGIC: |a log2 e| < 2^31, a = -z, i.e. z < 2^31 ln 2 = 1.4885e9).

    Beyond that limit the exponent in the low dword of t wraps and the result is wrong; no arithmetic is added to the hot path
    for it: the network's pre-activations are z = b + sum w h over 18 (conv1: cos / sin inputs, |.| <= 1) or 72 (conv2: |h1| <=
    |z1|) taps, so |z| < 2^31 ln 2 unless the weights reach ~1e3 -- a flow that far off is unusable long before (its sigmoids of
    |z| > 40 are already saturated at 0 / 1)."""
    zmax = 2.0 ** 31 * math.log(2.0)
    big = np.array([40.5, 100.0, 700.0, 745.0, 750.0, 1e4, 1e6, 1e9, np.nextafter(zmax * 0.999999, 0)])
    neg = np.array([-40.5, -100.0, -699.0] + neighbours(-700.0, 4) + [-745.0, -1e4, -1e9])
    sg = run(probe, P_SIGMOID, np.concatenate([big, neg]))[0]
    eb = ulp_err(sg[:len(big)], np.array([float(1 / (1 + mpmath.exp(-mpmath.mpf(v)))) for v in big]))
    assert eb.max() <= 2.8, worst(eb, big)
    sn = sg[len(big):]
    ref = np.array([float(1 / (1 + mpmath.exp(mpmath.mpf(min(-v, 700.0))))) for v in neg])
    e = ulp_err(sn, ref)
    bound = sigmoid_bound(np.maximum(neg, -700.0))
    assert np.all(e <= bound), worst(e - bound, neg)
    # below -700 the clamp holds the value of sigmoid(-700)
    assert np.all(sn[neg < -700.0] == run(probe, P_SIGMOID, np.array([-700.0]))[0][0])


def test_sigmoid4_is_the_scalar_sigmoid_lane_for_lane(probe):
    z = np.concatenate([sigmoid_inputs(), [700.0, -700.0, -1e4, 1e9, 745.0]])
    z = np.concatenate([z, np.zeros((-len(z)) % 4)])
    a = run(probe, P_SIGMOID, z)[0]
    b = run(probe, P_SIGMOID4, z)[0]
    assert np.array_equal(a.view(np.int64), b.view(np.int64)), int(np.sum(a != b))


# ----------------------------------------------------------------------------------------------------------------- activations
def test_activation_forms_agree_and_silu_is_accurate(probe):
    """act_eval4 = act_eval bit for bit for the three activations; relu / leaky relu exact; silu h = z sigmoid(z) and

    silu'(z) = sg (1 + z (1 - sg)), evaluated as fma(h, 1 - sg, sg).  Bound derived from the sigmoid's, b(z) = sigmoid_bound:
    d/dsg of sg + z sg (1 - sg) is 1 + z (1 - 2 sg), |.| <= 1 + |z|, so b(z) ulp(sg) become at most b(z) (1 + |z|) ulp(sg) in
    silu', plus the roundings of h, 1 - sg and the fma (each below one ulp of the scale): |error| <= (b(z) (1 + |z|) + 2) ulp of
    max(|silu'|, sg); h = z sg within b(z) + 1 ulp.  The scale is sg because silu' has a zero (z = -2.3994) where its two terms cancel."""
    z = np.concatenate([sigmoid_inputs(), neighbours(-2.3993572805154676, 8)])
    z = np.concatenate([z, np.zeros((-len(z)) % 4)])
    for act in (SILU, RELU, LEAKY):
        h, d, _ = run(probe, P_ACT, z, act=act)
        h4, d4, _ = run(probe, P_ACT4, z, act=act)
        assert np.array_equal(h.view(np.int64), h4.view(np.int64)) and np.array_equal(d.view(np.int64), d4.view(np.int64)), act
        if act == RELU:
            assert np.array_equal(h, np.where(z > 0, z, 0.0)) and np.array_equal(d, np.where(z > 0, 1.0, 0.0))
        elif act == LEAKY:
            assert np.array_equal(h, np.where(z > 0, z, 0.01 * z)) and np.array_equal(d, np.where(z > 0, 1.0, 0.01))
        else:
            zl = z.astype(LD)
            sg = sigmoid_ref(zl)
            eh = ulp_err(h, zl * sg, scale=np.maximum(np.abs(zl * sg), 1e-300))
            assert np.all(eh <= sigmoid_bound(z) + 1), worst(eh - sigmoid_bound(z) - 1, z)
            dref = sg * (1 + zl * (1 - sg))
            ed = ulp_err(d, dref, scale=np.maximum(np.abs(dref), sg))
            bound = sigmoid_bound(z) * (1 + np.abs(z)) + 2
            assert np.all(ed <= bound), worst(ed - bound, z)


# ----------------------------------------------------------------------------------------------------------------- exp
def exp_inputs():
    g = rng(2)
    return np.concatenate([np.linspace(-745.0, 709.0, 500001), g.uniform(-50, 50, 200000), g.uniform(-1, 1, 50000),
                           np.array([0.0, -0.0] + SUBN), neighbours(-745.0, 6), neighbours(709.0, 6), neighbours(700.0, 6),
                           neighbours(-708.3964185322641, 6), [-744.44007192138126, -1e4, 1e4, -1e300, 1e300]])


def test_exp_within_its_stated_bound_and_clamps(probe):
    """flow_common.h: ft_exp < 1.5 ulp on [-745, 709] (subnormal results included: the ulp there is 2^-1074); beyond, the clamp
    holds exp(-745) / exp(709)"""
    x = exp_inputs()
    e = run(probe, P_EXP, x)[0]
    inside = (x >= -745.0) & (x <= 709.0)
    ref = np.exp(np.clip(x, -745.0, 709.0).astype(LD))
    err = ulp_err(e[inside], ref[inside])
    assert err.max() <= 1.5, worst(err, x[inside])
    lo, hi = run(probe, P_EXP, np.array([-745.0, 709.0]))[0]
    assert np.all(e[x < -745.0] == lo) and np.all(e[x > 709.0] == hi)
    assert lo == 5e-324 and abs(hi - float(mpmath.exp(709))) <= 1.5 * float(ulp(hi))


def test_expN_is_ft_exp(probe):
    """ft_expN<4> (flow_fwd.hip) and ft_expN<2>: the same arithmetic as ft_exp, bit for bit"""
    x = exp_inputs()
    x = np.concatenate([x, np.zeros((-len(x)) % 4)])
    a = run(probe, P_EXP, x)[0]
    for op in (P_EXPN4, P_EXPN2):
        b = run(probe, op, x)[0]
        assert np.array_equal(a.view(np.int64), b.view(np.int64)), (op, int(np.sum(a != b)))


# ----------------------------------------------------------------------------------------------------------------- rcp
def test_rcp_within_one_ulp(probe):
    """ft_rcp (v_rcp_f64 + one third-order step) within 1 ulp for |t| in [2^-1000, 2^1000], both signs"""
    g = rng(3)
    t = np.exp2(g.uniform(-1000, 1000, 300000)) * g.choice([-1.0, 1.0], 300000)
    t = np.concatenate([t, g.uniform(0.5, 2.0, 200000), np.linspace(1e-3, 1e3, 100000), neighbours(1.0, 8), neighbours(2.0, 8),
                        neighbours(-1.0, 8), [3.0, 7.0, 0.1, 1e300, -1e-300]])
    y = run(probe, P_RCP, t)[0]
    err = ulp_err(y, LD(1) / t.astype(LD))
    assert err.max() <= 1.0, worst(err, t)


# ----------------------------------------------------------------------------------------------------------------- sincos
def test_sincos_within_its_stated_bound(probe):
    """ft_sincos: within 2.5 ulp for |x| up to 1e5 (common.h: the one-double reduced argument adds its rounding to the fdlibm
    polynomials' < 1 ulp; 2.16 measured).  Scale: ulp of max(|result|, 2^-26) -- within ~1.5e-8 of a zero of sin or cos the
    reduced argument r = x - k pi/2 carries an absolute error of about an ulp of the largest partial remainder (~2^-80 at
    |x| = 1e5) that no result of that size can hide, so there the error is counted in ulps of 2^-26 (absolute 3.3e-24)."""
    g = rng(4)
    x = np.concatenate([g.uniform(-1e5, 1e5, 400000), g.uniform(-2 * np.pi, 2 * np.pi, 400000), np.linspace(-10, 10, 100001),
                        np.array([0.0, -0.0] + SUBN)])
    ks = np.concatenate([np.arange(-16, 17), g.integers(-63000, 63000, 60), [63661, -63661]])
    edges = []
    for k in ks:
        edges += neighbours(float(mpmath.mpf(int(k)) * mpmath.pi / 2), 6)
        edges += neighbours(float((mpmath.mpf(int(k)) + 0.5) * mpmath.pi / 2), 2)   # the rint() tie points of x * 2 / pi
    edges += neighbours(np.pi, 6) + neighbours(-np.pi, 6) + neighbours(1e5, 4) + neighbours(-1e5, 4)
    x = np.concatenate([x, np.array(edges)])
    sn, cs, _ = run(probe, P_SINCOS, x)
    xl = x.astype(LD)
    bulk = len(x) - len(edges)
    for dev, f, name in ((sn, np.sin, 'sin'), (cs, np.cos, 'cos')):
        ref = f(xl)
        err = ulp_err(dev[:bulk], ref[:bulk], scale=np.maximum(np.abs(ref[:bulk]), 2.0 ** -26))
        assert err.max() <= 2.5, name + ': ' + worst(err, x[:bulk])
    xe = np.array(edges)
    rs = np.array([float(mpmath.sin(mpmath.mpf(v))) for v in xe])
    rc = np.array([float(mpmath.cos(mpmath.mpf(v))) for v in xe])
    for dev, ref, name in ((sn[bulk:], rs, 'sin'), (cs[bulk:], rc, 'cos')):
        err = ulp_err(dev, ref, scale=np.maximum(np.abs(ref), 2.0 ** -26))
        assert err.max() <= 2.5, name + ' (edges): ' + worst(err, xe)
    # tiny arguments are returned as they are (sin) / as 1 (cos); sin(-0) comes back as +0 (the reduction's fma adds -0 to
    # +0), which nothing downstream can tell apart: the values feed products and squares
    tiny = np.array([0.0, -0.0] + SUBN)
    s_, c_, _ = run(probe, P_SINCOS, tiny)
    assert np.array_equal(s_[2:].view(np.int64), tiny[2:].view(np.int64)) and np.all(s_[:2] == 0.0) and np.all(c_ == 1.0)


# ----------------------------------------------------------------------------------------------------------------- atan
def test_atan_within_two_ulp_and_its_special_values(probe):
    """ft_atan: 2 ulp over the line (the fold at |x| = 1 from both sides, tiny to huge); atan(+-inf) = +-pi/2 (the correctly
    rounded fp64 value); NaN gives NaN; +-0 and subnormals come back unchanged"""
    g = rng(5)
    x = np.concatenate([g.uniform(-1, 1, 300000), g.uniform(-4, 4, 200000), np.exp(g.uniform(-700, 700, 200000)) * g.choice([-1.0, 1.0], 200000),
                        np.linspace(-2, 2, 100001)])
    edges = neighbours(1.0, 12) + neighbours(-1.0, 12) + neighbours(1e300, 3) + neighbours(-1e300, 3) + [1.7976931348623157e308, -1.7976931348623157e308, 1e-8, 1e8]
    x = np.concatenate([x, np.array(edges)])
    y = run(probe, P_ATAN, x)[0]
    err = ulp_err(y, np.arctan(x.astype(LD)))
    assert err.max() <= 2.0, worst(err, x)
    xe = np.array(edges)
    re = np.array([float(mpmath.atan(mpmath.mpf(v))) for v in xe])
    err = ulp_err(y[-len(edges):], re)
    assert err.max() <= 2.0, worst(err, xe)
    sp = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0] + SUBN)
    ys = run(probe, P_ATAN, sp)[0]
    assert ys[0] == 1.5707963267948966 and ys[1] == -1.5707963267948966 and np.isnan(ys[2])
    assert np.array_equal(ys[3:].view(np.int64), sp[3:].view(np.int64)), ys[3:]


# ----------------------------------------------------------------------------------------------------------------- wrap, regularize
def wrap_inputs():
    g = rng(6)
    x = [g.uniform(-4 * np.pi, 4 * np.pi, 300000), g.uniform(-30, 30, 100000), g.uniform(-1e6, 1e6, 50000), np.linspace(-20, 20, 40001)]
    edges = [0.0, -0.0, np.inf, -np.inf, np.nan] + SUBN
    # the short path's limits: x + pi in {-2 pi, 0, 2 pi, 4 pi} as the device forms r = x + FT_PI
    for c in (-FT_TWO_PI, 0.0, FT_TWO_PI, 2.0 * FT_TWO_PI):
        edges += neighbours(c - FT_PI, 12)
    for k in range(-5, 6):
        edges += neighbours(k * FT_PI, 6)
    return np.concatenate(x + [np.array(edges)])


def _same(a, b):
    """bit-identical, any NaN equal to any NaN"""
    nan = np.isnan(a) & np.isnan(b)
    return np.all(nan | (a.view(np.int64) == b.view(np.int64)))


def test_wrap_is_torch_remainder_bit_for_bit(probe):
    """ft_wrap = oracle.ref_cpu.wrap (CPU fp64 torch.remainder(x + pi, 2 pi) - pi) on both of its paths"""
    from oracle import ref_cpu as R
    x = wrap_inputs()
    y = run(probe, P_WRAP, x)[0]
    ref = R.wrap(torch.from_numpy(x)).numpy()
    bad = ~(np.isnan(y) & np.isnan(ref)) & (y.view(np.int64) != ref.view(np.int64))
    assert not bad.any(), (x[bad][:8], y[bad][:8], ref[bad][:8])
    short = np.abs(x + FT_PI) < 2 * FT_TWO_PI
    assert short.sum() > 100000 and (~short & np.isfinite(x)).sum() > 10000     # both paths exercised


def test_wrap_pm_pi_is_wrap_on_the_principal_range(probe):
    g = rng(7)
    x = np.concatenate([g.uniform(-np.pi, np.pi, 300000), np.array(neighbours(FT_PI, 12) + neighbours(-FT_PI, 12) + [0.0, -0.0] + SUBN)])
    x = x[(x >= -FT_PI) & (x <= FT_PI)]
    a = run(probe, P_WRAP_PM_PI, x)[0]
    b = run(probe, P_WRAP, x)[0]
    assert _same(a, b)
    assert a[x == FT_PI][0] == -FT_PI


def test_regularize_is_the_oracle_bit_for_bit(probe):
    from oracle import ref_cpu as R
    x = wrap_inputs()
    y = run(probe, P_REGULARIZE, x)[0]
    ref = R.regularize(torch.from_numpy(x)).numpy()
    assert _same(y, ref), int(np.sum(y != ref))


# ----------------------------------------------------------------------------------------------------------------- the composite
def test_tan_mixture_component_near_p_pm_pi(probe):
    """One mixture component as flow_fwd.hip evaluates it: y = wrap(2 atan(e^s sn / cs)), (sn, cs) = ft_sincos(P / 2), and
    D = e^-s cos^2(P/2) + e^s sin^2(P/2) (through ft_rcp(e^s)), 1 / D through ft_rcp.

    Bounds, from the helpers': the atan argument carries sincos (2.5 + 2.5 ulp), the division (0.5), exp (1.5) and the product
    (0.5): 7.5 ulp relative, which atan turns into at most 7.5 / 2 ulp of pi / 2 absolute (|w / (1 + w^2)| <= 1/2); with atan's own
    2 ulp and the exact doubling, y is within 5.75 ulp(pi) (circular distance): 6 ulp(pi).  D is a sum of two positive terms, each
    within 1.5 + 1 (exp, rcp) + 5.5 (the square of a 2.5-ulp value) + 1 (two roundings) ulp: D within 9 ulp relative, 1 / D
    within 10.  |s| up to 700, the clamp of the sigmoid; ft_exp's own clamp is 709, where e^-s = 1.2e-308 leaves the normal
    range that ft_rcp is stated for."""
    g = rng(8)
    P = []
    for c in (FT_PI, -FT_PI):
        P += neighbours(c, 40)
    P += list(FT_PI - np.exp2(-np.arange(1, 50.0))) + list(-FT_PI + np.exp2(-np.arange(1, 50.0)))
    # not below |P| ~ 1e-150: sin^2(P/2) underflows there and e^s sin^2 is lost next to e^-s cos^2 at s ~ 700 (plaquettes are sums
    # of four link angles; an exact 0 is fine)
    P += list(g.uniform(-np.pi, np.pi, 200)) + [0.0, -0.0, 1e-140, np.pi / 2, -np.pi / 2]
    P = np.array(P)
    S = np.array([0.0, 1.0, -1.0, 0.3, -2.5, 5.0, -5.0, 20.0, -20.0, 100.0, -100.0, 700.0, -700.0])
    PP, SS = np.meshgrid(P, S)
    PP, SS = PP.ravel(), SS.ravel()
    y, D, invD = run(probe, P_COMPOSITE, PP, SS)
    pi = mpmath.pi
    ey, eD, eI = [], [], []
    for p, s, yd, dd, idd in zip(PP, SS, y, D, invD):
        p, s = mpmath.mpf(p), mpmath.mpf(s)
        t = mpmath.sin(p / 2) / mpmath.cos(p / 2)
        yr = 2 * mpmath.atan(mpmath.exp(s) * t)
        dist = abs(((mpmath.mpf(yd) - yr + pi) % (2 * pi)) - pi)
        Dr = mpmath.exp(-s) * mpmath.cos(p / 2) ** 2 + mpmath.exp(s) * mpmath.sin(p / 2) ** 2
        ey.append(float(dist))
        eD.append(float(abs(mpmath.mpf(dd) / Dr - 1)))
        eI.append(float(abs(mpmath.mpf(idd) * Dr - 1)))
    ey, eD, eI = np.array(ey), np.array(eD), np.array(eI)
    u = 2.0 ** -52
    assert np.all(np.isfinite(y)) and np.all((y >= -FT_PI) & (y < FT_PI)), y[~((y >= -FT_PI) & (y < FT_PI))][:4]
    k = int(np.argmax(ey)); assert ey[k] <= 6 * float(ulp(np.pi)), (ey[k], PP[k], SS[k])
    k = int(np.argmax(eD)); assert eD[k] <= 9 * u, (eD[k] / u, PP[k], SS[k])
    k = int(np.argmax(eI)); assert eI[k] <= 10 * u, (eI[k] / u, PP[k], SS[k])


# ----------------------------------------------------------------------------------------------------------------- the inverse, the adjoint
@pytest.mark.parametrize('tol', [1e-13, 0.0])
def test_transform_inverse_on_the_steep_fixture(probe, tol):
    """flow_transform.h mix_inverse, called as flow_fwd.hip's REV instances call it (e^{+-s_k} by one ft_expN<4>, target =
    ft_wrap(P' - t)), on the 20 x 2 x 64 active sites of tests/golden/steep_inverse.npz at L = 16: s, t of the oracle, P' = the
    mpmath forward of the true P.  Per site the bound of test_steep_inverse_gpu.py for the plaquette-level kernels,
    (tol + 8 delta_ref) / fp + 4 ulp(pi); test_steep_reference.py's numpy port of the loop reaches 0.93 of it on these inputs.  At
    tol = 0 the loop has to end through xn == xs or an error of exactly 0."""
    import steep_fixture as SF
    g = SF.load()
    worst_q = 0.0
    for r, ci, si, mu, off in SF.plaq_combos(g, 16):
        P = g['P_L16'][si][:, SF.active_mask(16, mu, off)].ravel()
        s = g['s_L16'][r]                                                   # [B, K, na]
        assert s.shape[1] == 2 and s.shape[0] * s.shape[2] == len(P) == 128
        rec = np.stack([g['fP_L16'][r].ravel(), g['t_L16'][r].ravel(), s[:, 0].ravel(), s[:, 1].ravel()], axis=1).ravel()
        o = run(probe, P_INVERSE, rec, np.full(len(rec), tol))[0].reshape(-1, 4)
        x, fpd = o[:, 0], o[:, 1]
        fp = g['fp_L16'][r].astype(np.float64).ravel()
        bound = (tol + 8 * g['delta_ref'][si]) / fp + 4 * SF.ULP_PI
        dx = np.abs(SF.wrapdiff(x, P))
        q = float(np.max(dx / bound))
        worst_q = max(worst_q, q)
        assert np.all(np.isfinite(x)) and np.all(np.isfinite(fpd)) and np.all(fpd > 0), (r, ci, mu, off)
        assert q <= 1.0, (r, ci, mu, off, q, float(dx.max()))
    print(f'mix_inverse, tol = {tol}: worst |dx| / bound {worst_q:.3f}')


def test_transform_adjoint_from_stash_coefficients(probe):
    """flow_transform.h MixAdjoint from a stash record (A_k B_k C_k E_k, K = 2), as the three backward kernels build it:
        gs_k = gd A_k + cb B_k / (K sum C),    dir = gd (sum C - 1) - cb sum E / (K sum C)
    against mpmath on the same doubles.  Roundings of the helper, u = 2^-53 (half an ulp, relative) each unless stated; a
    contraction into an FMA only removes one:
      csum = (0 + C_0) + C_1: 1 (C_k > 0: no cancellation); esum = E_0 + E_1: 1, relative to |E_0| + |E_1|; K csum: exact;
      1 / (K csum) by v_rcp_f64 and two correction steps: within 1 ulp = 2 u; cbr = cb rs: 1   -> cbr within 4 u of cb / (K sum C);
      gs_k = gd A_k + cbr B_k: two products and the sum -> |error| <= (2 T1 + 6 T2) u, T1 = |gd A_k|, T2 = |cb B_k| / (K sum C);
      dir: csum - 1 carries csum's rounding (u sum C) and its own (u |sum C - 1|), the product one more, cbr esum 4 + 1 + 1, the
      last subtraction u (|gd| |sum C - 1| + TE) -> |error| <= (4 G + 7 TE) u, G = |gd| (sum C + 1), TE = |cb| (|E_0| + |E_1|) / (K sum C):
      in units of the terms' magnitudes, so that the cancellation in sum C - 1 (sum C = dP'/dP is 1 for the identity map) is not
      held against the helper.
    Second-order terms are below 2^-45 of these (at most 11 factors 1 + u): the bounds are asserted with a factor 1 + 2^-40."""
    g = rng(9)
    n = 4096
    C = np.exp(g.uniform(-9.0, 3.0, (n, 2)))                                # 1 / (K D_k): e^{-|s|} .. e^{|s|} / K
    near1 = g.random(n) < 0.25                                               # sum C near 1: the near-identity flows
    C[near1, 0] = g.uniform(0.01, 0.99, near1.sum())
    C[near1, 1] = 1.0 - C[near1, 0] + g.normal(0, 1e-9, near1.sum())
    A, Bc, E = (g.normal(0, 1, (n, 2)) * np.exp(g.uniform(-6, 6, (n, 2))) for _ in range(3))
    gd = g.normal(0, 1, n) * np.exp(g.uniform(-8, 8, n))
    cb = g.normal(0, 1, n) * np.exp(g.uniform(-8, 8, n))
    assert np.all(C > 0) and (gd > 0).any() and (gd < 0).any() and (cb > 0).any() and (cb < 0).any()
    rec = np.stack([A[:, 0], Bc[:, 0], C[:, 0], E[:, 0], A[:, 1], Bc[:, 1], C[:, 1], E[:, 1]], axis=1).ravel()
    sv = np.zeros((n, 8))
    sv[:, 0], sv[:, 1] = gd, cb
    o = run(probe, P_ADJOINT, rec, sv.ravel())[0].reshape(n, 8)
    u = 2.0 ** -53 * (1 + 2.0 ** -40)
    m = mpmath.mpf
    worst_gs = worst_dir = 0.0
    for i in range(n):
        sc, se = m(C[i, 0]) + m(C[i, 1]), m(E[i, 0]) + m(E[i, 1])
        cbr = m(cb[i]) / (2 * sc)
        for k in range(2):
            ref = m(gd[i]) * m(A[i, k]) + cbr * m(Bc[i, k])
            bound = (2 * abs(m(gd[i]) * m(A[i, k])) + 6 * abs(cbr * m(Bc[i, k]))) * u
            q = float(abs(m(o[i, k]) - ref) / bound)
            worst_gs = max(worst_gs, q)
            assert q <= 1.0, ('gs', i, k, q)
        ref = m(gd[i]) * (sc - 1) - cbr * se
        bound = (4 * abs(m(gd[i])) * (sc + 1) + 7 * abs(cbr) * (abs(m(E[i, 0])) + abs(m(E[i, 1])))) * u
        q = float(abs(m(o[i, 2]) - ref) / bound)
        worst_dir = max(worst_dir, q)
        assert q <= 1.0, ('dir', i, q)
    print(f'MixAdjoint: worst error / bound: gs {worst_gs:.3f}, dir {worst_dir:.3f}')


# ----------------------------------------------------------------------------------------------------------------- index helpers
def test_fdiv_exact_for_every_small_divisor(probe):
    """fdiv<D>(u) = u / D for every D in 2..32 and every u in [0, 32768)"""
    n = 32768
    u = np.arange(n)
    for D in range(2, 33):
        out = np.empty(n, dtype=np.int32)
        assert probe.probe_fdiv(D, _p(out, _I), n) == 0
        bad = out != u // D
        assert not bad.any(), (D, u[bad][:4], out[bad][:4])


def _wrap_line(probe, form, Ls, extra):
    lstart, nl = int(Ls[0]), len(Ls)
    cnt = 3 * Ls + extra
    base = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)
    total = int(cnt.sum())
    out = np.empty(total, dtype=np.int32)
    assert probe.probe_wrap_line(form, lstart, nl, extra, _p(base, ctypes.POINTER(ctypes.c_longlong)), _p(out, _I), total) == 0
    return out, base


def test_wrap_line_all_forms_on_their_domains(probe):
    """wrap_line = v mod L: the general form (wrap_magic: n M >> 32 = n / L for n, L < 2^16) for every L = 0 mod 4 in 4..8192 and
    v from -L up to the window reach of a 16 x 16 tile on the smallest lattices (2 L + 24); the FAST form on -L <= v < 2 L for
    every L (the launchers take it where wrap_fast_ok, L >= 24); POW2 (EXACT instances: L a power of two, 32..8192) on the same v"""
    Ls = np.arange(4, 8193, 4)
    extra = 24
    gen, base = _wrap_line(probe, 0, Ls, extra)
    fast, _ = _wrap_line(probe, 1, Ls, extra)
    for k, L in enumerate(Ls):
        L = int(L)
        v = np.arange(-L, 2 * L + extra)
        seg = slice(int(base[k]), int(base[k]) + len(v))
        assert np.array_equal(gen[seg], v % L), ('general', L)
        assert np.array_equal(fast[seg][:3 * L], (v % L)[:3 * L]), ('fast', L)
    P2 = np.array([1 << e for e in range(2, 14)])
    for L in P2:
        pw, b2 = _wrap_line(probe, 2, np.array([L]), extra)
        v = np.arange(-L, 2 * L + extra)
        assert np.array_equal(pw, v % L), ('pow2', L)


def _stash_model(L, mu, off):
    """compact indices, restated from the layout (flow_mfma_common.h struct Stash): rank of a site's stripe line among the
    stored lines in their storage order, times the sites per line, plus the position along the line"""
    x = np.arange(L)
    act_lines = x[(x - off) % 4 == 0]                               # in lattice order
    live_lines = sorted([v for v in x if (v - off) % 4 != 2], key=lambda v: (v - off - 3) % L)
    froz_lines = sorted([v for v in x if (v - off) % 4 in (1, 2)], key=lambda v: (v - off - 1) % L)
    maps = {}
    for name, lines in (('act', act_lines), ('live', live_lines), ('frozen', froz_lines)):
        rank = np.full(L, -1)
        rank[np.array(lines)] = np.arange(len(lines))
        maps[name] = (rank, len(lines))
    return maps


def _check_stash(probe, L, rows, cols):
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    ns = (len(rows) + len(cols)) * L
    ii = np.concatenate([np.repeat(rows, L), np.tile(np.arange(L), len(cols))])
    jj = np.concatenate([np.tile(np.arange(L), len(rows)), np.repeat(cols, L)])
    full = len(rows) == L and len(cols) == 0
    for mu in (0, 1):
        for off in range(4):
            outs = [np.empty(ns, dtype=np.int32) for _ in range(4)]
            rc = probe.probe_stash(L, mu, off, _p(rows, _I), len(rows), _p(cols, _I) if len(cols) else None, len(cols),
                                   *[_p(o, _I) for o in outs])
            assert rc == 0
            line, along = (jj, ii) if mu == 0 else (ii, jj)
            model = _stash_model(L, mu, off)
            for name, got in (('act', outs[0]), ('live', outs[1]), ('live_pow2', outs[2]), ('frozen', outs[3])):
                if name == 'live_pow2' and L & (L - 1):
                    continue
                rank, nlines = model['live' if name == 'live_pow2' else name]
                on = rank[line] >= 0
                # storage order: mu = 0 planes are [i][compact column], mu = 1 planes [compact row][j]
                want = along[on] * nlines + rank[line[on]] if mu == 0 else rank[line[on]] * L + along[on]
                assert np.array_equal(got[on], want), (name, L, mu, off)
                count = nlines * L
                assert got[on].min() >= 0 and got[on].max() < count, (name, L, mu, off)
                if full:                                             # a bijection onto [0, count)
                    assert np.array_equal(np.sort(got[on]), np.arange(count)), (name, L, mu, off)
            if L & (L - 1) == 0:
                assert np.array_equal(outs[1], outs[2]), ('pow2 vs general', L, mu, off)


def test_stash_maps_are_bijections_on_every_small_lattice(probe):
    """stash_active_idx, stash_live_idx<false / true>, stash_frozen_idx on every site of every L = 0 mod 4 up to 256, every
    (mu, off): each equals the layout's rank model and is a bijection onto [0, count) on its sites"""
    for L in range(4, 257, 4):
        _check_stash(probe, L, np.arange(L), [])


@pytest.mark.parametrize('L', [1020, 1024, 4096, 8188, 8192])
def test_stash_maps_on_sampled_lines_of_large_lattices(probe, L):
    """the same on whole rows and whole columns through sampled lines (first and last included) of the large lattices: along
    the sampled rows / columns every stripe line of either direction is met"""
    g = rng(L)
    sel = np.unique(np.concatenate([np.arange(8), np.arange(L - 8, L), g.integers(0, L, 16)]))
    _check_stash(probe, L, sel, sel)


# ----------------------------------------------------------------------------------------------------------------- grid extents
def test_grid_extent_of_the_chain_dimension(probe):
    """The plain-lattice and flow launchers put the chain index in blockIdx.y / blockIdx.z (k_plaq, k_force, k_random_momenta,
    the flow kernels' chain groups): extents past 65536 launch and reach their last block, so the chain limit of
    include/fthmc_hip.h comes from the x extents (one workgroup of up to 1024 threads per chain), not from y / z."""
    lim = (ctypes.c_int * 3)()
    assert probe.probe_grid_limits(lim) == 0
    # the runtime reports its maxGridSize (65536 for y and z on the machines this was written on) but does not enforce it: the
    # dispatch packet's extents are 32-bit work-item counts.  Up to FTHMC_MAX_B, the largest chain extent the launchers form
    print('maxGridSize', list(lim))
    hdr = open(os.path.join(ROOT, 'include', 'fthmc_hip.h')).read()
    bmax = int(re.search(r'#define FTHMC_MAX_B (\d+)', hdr).group(1))
    for gy, gz in ((65536, 1), (1, 65536), (65537, 1), (1, 65537), (bmax, 1), (1, bmax)):
        seen = np.zeros(1, dtype=np.int32)
        assert probe.probe_grid_launch(gy, gz, _p(seen, _I)) == 0, (gy, gz)
        assert int(seen[0]) == gy ^ gz, (gy, gz, int(seen[0]))
