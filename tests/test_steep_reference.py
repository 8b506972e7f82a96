"""CPU checks behind tests/test_steep_inverse_gpu.py: the steep-flow fixture regenerates, its mpmath forward agrees with the
oracle where the oracle is trustworthy, and a plain fp64 port of the kernels' safeguarded Newton loop (csrc/flow_transform.h
mix_inverse, which csrc/flow_fwd.hip REV and flow_generic.hip k_gen_transform<REV> call, and flow.hip MODE 3, the VALU variant's
own statement of it) meets, on the fixture's own inputs, the bounds the GPU tests ask of the kernels -- so the inputs are fair
to a correct kernel.

Measured with the port (tol = 1e-13): at most 15 / 20 / 22 / 35 iterations at s0 = 2 / 5 / 10 / 20, worst |dx| = 0.93 of its
bound, worst log J error 0.14 of its bound; at tol = 0 (L = 16) at most 60 iterations, ending through xn == xs or through an
error of exactly 0.0 (the loop's f is rounded like the forward's wrap, so it meets its target exactly more often than not).

The port is the loop as it stands since this test exists: with the component 2 atan(.) wrapped to [-pi, pi) as in the forward
map, the port (and every kernel) missed the per-site bound twice over at the planted pi - d of s0 = 10, signs (+,+) -- see
flow_transform.h mix_inverse (common.h ft_round_pm_pi)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import steep_fixture as SF
from conftest import GOLDEN
from oracle import ref_cpu as R

sys.path.insert(0, GOLDEN)


def round_pm_pi(x):
    """common.h ft_round_pm_pi: the rounding of the forward's wrap, without its move of pi to -pi (the loop's f is monotone)"""
    return (x + math.pi) - math.pi


def newton_port(target, s, tol):
    """The documented loop, vectorised over sites: start at the target, bracket lo / hi, bisection when a step leaves the bracket,
    stop on |err| <= tol or xn == xs, 200 iterations at the most.  target [n], s [K, n] -> (x, fp at the last iterate, iterations,
    ended [n] bool, ended through xn == xs [n] bool)"""
    es, ems = np.exp(s), np.exp(-s)
    lo, hi = np.full_like(target, -math.pi), np.full_like(target, math.pi)
    xs, fp = target.copy(), np.ones_like(target)
    done, same = np.zeros(target.shape, bool), np.zeros(target.shape, bool)
    iters = np.zeros(target.shape, np.int64)
    for _ in range(200):
        live = ~done
        if not live.any():
            break
        sn, cs = np.sin(xs / 2), np.cos(xs / 2)
        with np.errstate(over='ignore', divide='ignore'):
            f = round_pm_pi(2 * np.arctan(es * (sn / cs))).mean(0)
            fpn = (1.0 / (ems * cs * cs + es * sn * sn)).mean(0)
        fp = np.where(live, fpn, fp)
        iters += live
        err = target - f
        done |= live & (np.abs(err) <= tol)
        upd = ~done
        lo = np.where(upd & (err > 0), xs, lo)
        hi = np.where(upd & ~(err > 0), xs, hi)
        xn = xs + err / fp
        xn = np.where((xn > lo) & (xn < hi), xn, 0.5 * (lo + hi))
        stop = upd & (xn == xs)
        same |= stop
        done |= stop
        xs = np.where(upd, xn, xs)
    return xs, fp, iters, done, same


@pytest.fixture(scope='module')
def g():
    return SF.load()


def test_fixture_is_small_and_states_its_noise_floor(g):
    assert os.path.getsize(os.path.join(GOLDEN, 'steep_inverse.npz')) < 1000 * 1000
    assert g['delta_ref'].shape == (4,) and 0 < g['delta_ref'].max() < 8 * SF.ULP_PI    # a few roundings of an angle
    assert g['cond_max'].max() <= 1e13
    assert len(g['combo_L32']) == 80 and len(g['combo_L20']) == len(g['combo_L16']) == 20
    for L in (16, 20, 32):                                       # the planted values sit on active sites of every (mu, off)
        for r, ci, si, mu, off in SF.plaq_combos(g, L):
            Pa = g[f'P_L{L}'][si][:, SF.active_mask(L, mu, off)]
            small = np.sort(np.abs(Pa).ravel())[:5]
            assert small[0] == 0.0 and small[1] == small[2] == 1e-12 and small[3] == small[4] == 1e-6
            assert np.sum(math.pi - np.abs(Pa) < 2e-4) >= 2


def test_fixture_regenerates_bit_for_bit(g):
    pytest.importorskip('mpmath')
    import make_golden_steep
    new = make_golden_steep.generate()
    assert sorted(new) == sorted(g)
    for k in sorted(g):
        a, b = np.asarray(new[k]), g[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def test_mpmath_forward_is_the_oracle_near_the_identity():
    """At s0 = 0.3 (the range the default init gives) the oracle's fp64 forward has no cancellation to lose: the high-precision
    forward of the generator must reproduce it to 1e-14."""
    mp = pytest.importorskip('mpmath')
    import make_golden_steep as M
    mp.mp.dps = 40
    gen = torch.Generator().manual_seed(303)
    L, mu, off = 16, 1, 2
    w = M.case_weights(R.default_flow(1, gen)[0], 0.3, (1, -1))
    P = (torch.rand(2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi
    s, t, act = M.net_st(R, P, w, mu, off)
    r = M.mp_forward(mp, P[:, act].numpy(), s, t)
    fx, logJ = R.plaq_coupling_forward(P, w, mu, off)
    assert np.abs(SF.wrapdiff(fx[:, act].numpy(), r['fP'])).max() <= 1e-14
    assert np.abs(logJ.numpy() - r['logJ']).max() <= 1e-14 * max(1.0, r['labs'].max())
    assert np.array_equal(fx[:, ~act].numpy(), P[:, ~act].numpy())


def _inputs(g, L):
    """per plaquette-level combo: (si, true P, target, s, fp) at the active sites, chains flattened, and the per-chain sums; s, t from
    the oracle"""
    for r, ci, si, mu, off in SF.plaq_combos(g, L):
        P = torch.from_numpy(g[f'P_L{L}'][si])
        w = [torch.from_numpy(a) for a in SF.case_weights(g, ci)]
        mA, mF, _, _ = R.stripe_masks(L, mu, off)
        x2 = mF * P
        out = R.conv_net(torch.stack((torch.cos(x2), torch.sin(x2)), dim=1), w)
        act = mA.bool()
        s = out[:, :-1][:, :, act].numpy()                       # [B, K, na]
        t = out[:, -1][:, act].numpy()
        if L == 16:
            assert np.abs(s - g['s_L16'][r]).max() < 1e-13 and np.abs(t - g['t_L16'][r]).max() < 1e-13
            s, t = g['s_L16'][r], g['t_L16'][r]
        target = R.wrap(torch.from_numpy(g[f'fP_L{L}'][r] - t)).numpy()
        yield si, P[:, act].numpy().ravel(), target.ravel(), s.transpose(1, 0, 2).reshape(s.shape[1], -1), \
            g[f'fp_L{L}'][r].astype(np.float64).ravel(), {k: g[f'{k}_L{L}'][r] for k in ('logJ', 'labs', 'sens')}


def test_newton_port_meets_the_bounds_on_the_fixture_inputs(g):
    """The bounds are the GPU test's: per site (tol + 8 delta_ref) / fp, plus 4 ulp(pi) because x itself is a double in [-pi, pi)
    (where the map is steep, fp ~ e^{|s|}, the first term is far below the spacing of the doubles around x); log J per chain."""
    worst, worst_lj, most = 0.0, 0.0, {si: 0 for si in range(4)}
    for L in (32, 20, 16):
        for si, P, target, s, fp, e in _inputs(g, L):
            x, fpl, iters, done, _ = newton_port(target, s, SF.TOL)
            assert done.all() and iters.max() < 200
            bound = (SF.TOL + 8 * g['delta_ref'][si]) / fp + 4 * SF.ULP_PI
            dx = np.abs(SF.wrapdiff(x, P))
            assert (dx <= bound).all(), (L, si, float((dx / bound).max()))
            worst = max(worst, float((dx / bound).max()))
            most[si] = max(most[si], int(iters.max()))
            dlj = np.abs(-np.log(fpl).reshape(2, -1).sum(1) + e['logJ'])  # log J of the inverse, taken at the last iterate
            blj = (SF.TOL + 8 * g['delta_ref'][si]) * e['sens'] + 1e-12 * e['labs']
            assert (dlj <= blj).all(), (L, si, dlj, blj)
            worst_lj = max(worst_lj, float((dlj / blj).max()))
    print(f'port: most iterations per s0 {most}, worst |dx| / bound {worst:.3f}, worst log J error / bound {worst_lj:.3f}')
    assert max(most[si] for si in range(3)) > 10                          # steep enough to leave the near-identity regime


def test_newton_port_ends_without_a_tolerance(g):
    """tol = 0.0 is met only by an error of exactly 0.0: otherwise the loop has to end through xn == xs, well inside its 200
    iterations."""
    most = n_same = 0
    for si, P, target, s, fp, _e in _inputs(g, 16):
        x, _, iters, done, same = newton_port(target, s, 0.0)
        assert done.all() and iters.max() < 200                          # through xn == xs, or an error of exactly 0.0
        n_same += int(same.sum())
        bound = 8 * g['delta_ref'][si] / fp + 4 * SF.ULP_PI
        dx = np.abs(SF.wrapdiff(x, P))
        assert (dx <= bound).all(), (si, float((dx / bound).max()))
        most = max(most, int(iters.max()))
    print(f'port at tol = 0: most iterations {most}, {n_same} sites ended through xn == xs')
    assert n_same > 0
