"""The coupling layer and its inverse on STEEP flows (|s| = 2 .. 20) against tests/golden/steep_inverse.npz: mpmath at 40 digits
on the oracle's s, t (tests/golden/make_golden_steep.py).  Every other inverse test draws default-init weights, |s| < 0.3, where
the tan-mixture map is almost the identity and the safeguarded Newton loop needs 4 plain steps; here it needs its bracket, its
bisection fallback, its xn == xs stop, and log J at ill-conditioned roots.  Both statements of the loop run, through every
caller: csrc/flow_transform.h mix_inverse from csrc/flow_fwd.hip (REV instances: exact tiles at L = 32, ragged at L = 20, L = 16
with the fused small path off) and from csrc/flow_generic.hip (n_mix 1 and 3), and csrc/flow.hip's own (VALU variant, link level).

Tolerances follow the conditioning, never a kernel's output.  delta_ref = max |oracle fp64 forward - mpmath forward| over the
active sites is the reference's own noise floor, measured by the generator per s0 and stored in the fixture:

    s0 = 2: 1.332e-15    s0 = 5: 1.332e-15    s0 = 10: 1.332e-15    s0 = 20: 8.882e-16

The factor 8 on it is margin for the kernels' own exp / atan / sincos (< 1.5 ulp each, test_device_math_gpu.py) over libm.
  forward fP            8 delta_ref, as an angle
  forward log J         1e-12 sum |local log J|
  inverse, per site     (tol + 8 delta_ref) / fp + 4 ulp(pi), tol = 1e-13, fp = dfP/dP at the site (1 / fp = dx/dy reaches e^{|s|})
  inverse log J         (tol + 8 delta_ref) sum |d log fp/dP| / fp + 1e-12 sum |local log J|
  frozen, passive       bit-equal to the input
The link-level entries add roundings of their own, at the magnitude of a plaquette of wrapped links (|P| < 4 pi, ulp = 4 ulp(pi)):
forward links 8 delta_ref + 4 ulp(pi) (d = fP - P, then wrap(d + x)); inverse: the kernel's plaquette of y carries up to
E = 8 ulp(pi) of summation rounding, which moves the target (y-space: tol + 8 delta_ref + E) and enters the link update directly,
with the roundings of d and of the wrap: 16 ulp(pi) in place of 4.

Found by these inputs: inside the loop a component 2 atan(.) that rounds to exactly pi was wrapped to -pi as in the forward map;
at s0 = 10, (+,+), P = pi - d the loop then ended at pi, 4.7e-9 from the root (2.06 times the per-site bound; 21 times at tol = 0)
in every copy the loop then had.  The loop keeps the component monotone now (flow_transform.h mix_inverse, common.h ft_round_pm_pi).

No site is left out of any check.  The test prints the observed maxima as fractions of their bounds (pytest -s)."""
import math

import numpy as np
import pytest
import torch

import steep_fixture as SF
from steep_fixture import TOL, ULP_PI

from gpu_support import D, H, module_defaults, ops, switches

pytestmark = pytest.mark.gpu
_defaults = module_defaults()


@pytest.fixture(scope='module')
def g():
    return SF.load()


def W(ws):
    return ops.pack_weights([tuple(torch.from_numpy(np.asarray(a)) for a in ws)], device='cuda')


class Worst:
    """largest observed error / bound per quantity"""

    def __init__(self):
        self.r = {}

    def check(self, key, err, bound, where):
        err, bound = np.asarray(err), np.asarray(bound)
        q = float(np.max(err / bound))
        self.r[key] = max(self.r.get(key, 0.0), q)
        assert np.all(np.isfinite(err)) and q <= 1.0, (key, where, q, float(np.max(err)))

    def show(self, title):
        print(title + ': ' + ', '.join(f'{k} {v:.3f}' for k, v in self.r.items()) + '  (error / bound)')


def check_plaq_level(wst, w, P, act, e, delta, where, arch=None, tol=TOL, sanity=False):
    """forward and inverse of one plaquette-level case; e: the fixture's fP, fp [B, na], logJ, labs, sens [B]"""
    Pd = D(P)
    fPg, ljg = ops.plaq_coupling_fwd(Pd, w, *where[-2:], arch=arch)
    fPg, ljg = H(fPg), H(ljg)
    wst.check('fwd fP', np.abs(SF.wrapdiff(fPg[:, act], e['fP'])), 8 * delta, where)
    wst.check('fwd logJ', np.abs(ljg - e['logJ']), 1e-12 * e['labs'], where)
    assert np.array_equal(fPg[:, ~act], P[:, ~act]), where
    fP = P.copy()
    fP[:, act] = e['fP']
    Pr, ljr = ops.plaq_coupling_rev(D(fP), w, *where[-2:], tol=tol, arch=arch)
    Pr, ljr = H(Pr), H(ljr)
    fp = e['fp'].astype(np.float64)
    wst.check('rev x', np.abs(SF.wrapdiff(Pr[:, act], P[:, act])), (tol + 8 * delta) / fp + 4 * ULP_PI, where)
    wst.check('rev logJ', np.abs(ljr + e['logJ']), (tol + 8 * delta) * e['sens'] + 1e-12 * e['labs'], where)
    assert np.array_equal(Pr[:, ~act], fP[:, ~act]), where
    if sanity:
        for a in (fPg, Pr):
            assert np.all(np.isfinite(a)) and a.min() >= -math.pi and a.max() < math.pi, where
        assert np.all(np.isfinite(ljg)) and np.all(np.isfinite(ljr))


@pytest.mark.parametrize('L', [32, 20, 16])
def test_mfma_plaquette_level(g, L):
    """k_flow_fwd<.., REV>: exact two-by-two tiles at L = 32 (all eight (mu, off)), ragged tiles at L = 20, and L = 16 on the tiled
    kernels (the fused small-lattice path switched off)."""
    wst = Worst()
    try:
        with switches(variant=1, small=(L != 16)):
            for r, ci, si, mu, off in SF.plaq_combos(g, L):
                e = {k: g[f'{k}_L{L}'][r] for k in ('fP', 'fp', 'logJ', 'labs', 'sens')}
                check_plaq_level(wst, W(SF.case_weights(g, ci)), g[f'P_L{L}'][si], SF.active_mask(L, mu, off), e, g['delta_ref'][si],
                                 (L, ci, mu, off), sanity=(si == 3))
    finally:
        wst.show(f'mfma L={L}')


def test_generic_net_plaquette_level(g):
    """k_gen_transform<double, REV>: one and three mixture components, hidden [4]."""
    wst = Worst()
    for gi in range(4):
        K, si, mu, off = (int(v) for v in g[f'gen{gi}_meta'])
        w = W([g[f'gen{gi}_w{pi}'] for pi in range(4)])
        assert ops.arch_of(w) == ((4,), 3, K)
        e = {k: g[f'gen{gi}_{k}'] for k in ('fP', 'fp', 'logJ', 'labs', 'sens')}
        check_plaq_level(wst, w, g['P_L16'][si], SF.active_mask(16, mu, off), e, g['delta_ref'][si], ('gen', gi, mu, off))
    wst.show('generic')


def check_link_level(wst, g, ci, tol=TOL):
    _, L, mu, off = (int(v) for v in g[f'link{ci}_meta'])
    si = SF.si_of(g, ci)
    delta = g['delta_ref'][si]
    w = W(SF.case_weights(g, ci))
    act = SF.active_mask(L, mu, off)
    x = g[f'link{ci}_x']
    e = {k: g[f'link{ci}_{k}'] for k in ('yl', 'fp', 'logJ', 'labs', 'sens')}
    where = ('link', ci, L, mu, off)
    yg, ljg = ops.flow_layer_fwd(D(x), w, mu, off)
    yg, ljg = H(yg), H(ljg)
    wst.check('fwd y', np.abs(SF.wrapdiff(yg[:, mu][:, act], e['yl'])), 8 * delta + 4 * ULP_PI, where)
    wst.check('fwd logJ', np.abs(ljg - e['logJ']), 1e-12 * e['labs'], where)
    y = x.copy()
    y[:, mu][:, act] = e['yl']
    same = np.ones(x.shape, bool)
    same[:, mu][:, act] = False
    assert np.array_equal(yg[same], x[same]), where
    xr, ljr = ops.flow_layer_rev(D(y), w, mu, off, tol=tol)
    xr, ljr = H(xr), H(ljr)
    ytol = tol + 8 * delta + 8 * ULP_PI
    wst.check('rev x', np.abs(SF.wrapdiff(xr[:, mu][:, act], x[:, mu][:, act])), ytol / e['fp'] + 16 * ULP_PI, where)
    wst.check('rev logJ', np.abs(ljr + e['logJ']), ytol * e['sens'] + 1e-12 * e['labs'], where)
    assert np.array_equal(xr[same], y[same]), where
    if si == 3:
        assert np.all(np.isfinite(yg)) and np.all(np.isfinite(xr)) and xr.min() >= -math.pi and xr.max() < math.pi


@pytest.mark.parametrize('variant', [0, 1], ids=['valu', 'mfma'])
def test_link_level(g, variant):
    """k_flow_layer<MODE 0 / 3> (the VALU variant has no plaquette-level entry) and the MFMA kernels' link output, on link fields
    whose plaquettes are exact sums (links are multiples of 2^-40) with |P| < pi."""
    wst = Worst()
    try:
        with switches(variant=variant, small=False):
            for ci in range(len(g['case_s0'])):
                check_link_level(wst, g, ci)
    finally:
        wst.show('link level, variant %d' % variant)


def test_loop_ends_without_a_tolerance(g):
    """tol = 0.0 is met only by an error of exactly 0.0: otherwise the loop has to end through xn == xs in each of its callers
    (test_steep_reference.py shows the plain port ending in at most 60 of its 200 iterations), at (8 delta_ref) / fp + 4 ulp(pi) per
    site.  Once per caller, at L = 16, on the steepest regular case (s0 = 10, (+,+): at the planted pi - d the target lies 2e-13
    below pi and the start of the iteration itself saturates the atan)."""
    wst = Worst()
    try:
        with switches(small=False):
            r, ci, si, mu, off = [c for c in SF.plaq_combos(g, 16)
                                  if g['case_s0'][c[1]] == 10.0 and tuple(g['case_sign'][c[1]]) == (1, 1)][0]
            e = {k: g[f'{k}_L16'][r] for k in ('fP', 'fp', 'logJ', 'labs', 'sens')}
            check_plaq_level(wst, W(SF.case_weights(g, ci)), g['P_L16'][si], SF.active_mask(16, mu, off), e, g['delta_ref'][si],
                             ('tol0', ci, mu, off), tol=0.0)
            K, si, mu, off = (int(v) for v in g['gen3_meta'])
            e = {k: g[f'gen3_{k}'] for k in ('fP', 'fp', 'logJ', 'labs', 'sens')}
            check_plaq_level(wst, W([g[f'gen3_w{pi}'] for pi in range(4)]), g['P_L16'][si], SF.active_mask(16, mu, off), e,
                             g['delta_ref'][si], ('tol0 gen', 3, mu, off), tol=0.0)
            with switches(variant=0):
                check_link_level(wst, g, 6, tol=0.0)                    # s0 = 10, (+,+), L = 16
    finally:
        wst.show('tol = 0')
