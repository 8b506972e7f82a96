"""GPU tests of boundary-condition tempering through the flow at the launch edges of the defect kernels it shares with the
plain sampler, against the torch float64 twin of tests/ft_defect_cases.py (FD.force, FD.action, FD.trajectory) on two shapes that are
not in FD.CASES:

  (B 258, L 8, one default-init layer x 3), run two ways: with the small path off the sequenced path -- launch_defect_sums into the
      workspace rows and launch_defect_energy on `rows + 2 B`, 258 chains: past one workgroup of 256 and into its guard --, with it on
      k_ft_small's DEFECT instance.  Defects wrap (nstep 1, leapfrog, amplitude pi, beta 2) and end (nstep 2, omelyan, amplitude 0.3,
      beta 6: a line that starts on the last row); couplings mixed out of {0, beta / 3, beta}, three different on chains 255 .. 257.
  (B 2, L 132, one layer): the defect across the pass edge of launch_defect_gp's grid-stride loop (sites 16373 and 16505 either side
      of 16384) and the one that starts behind the edge and wraps to the front; a one-step leapfrog trajectory, i.e. the second pass
      of launch_defect_gp as the seed of the flowed force.

Bounds: those of tests/test_z_ft_defect_gpu.py, quoted at each check; the two settings against each other within the sum of the two
paths' bounds against the twin (tests/test_z_ft_meta_gpu.py's path-to-path rule).  No bound is widened: the reference side -- the
float64 twin's C and Dsum against a long double evaluation (defect_cases.sums) of the twin's own flowed field -- uses less than 1/8 of
its bound on either shape, which test_the_reference_side_does_not_widen_a_bound computes on the CPU and prints.  Accept flags are
compared on every chain: the twin leaves none out on these seeds.

Observed on an MI355X (worst |device - twin| over the chains; the reference side: C within 5.6e-14 relative and Dsum within 1.6e-15 of
the long double evaluation on every shape):
  force and action            force / its scale   S relative   Dsum          (bounds: 1e-8 rel + 1e-10 of the scale, 1e-11, 1e-11)
  B258-L8 wrap, off = small   3.3e-15             4.0e-13      7.1e-15
  B258-L8 end, off = small    1.5e-15             3.8e-16      4.4e-15
  B2-L132 straddle            2.1e-15             8.9e-16      2.2e-16
  B2-L132 wrapback            1.1e-15             3.0e-16      0
  trajectories                dH        H0        H1        plaq      Q         Dsum      (bounds: 1e-6, 1e-10 rel, 1e-7 rel, 1e-6 rel, 1e-6, 1e-8)
  B258-L8 wrap   off          7.1e-14   4.3e-14   4.3e-14   1.9e-16   1.3e-15   9.1e-15
                 small        5.7e-14   4.3e-14   4.3e-14   2.0e-16   1.3e-15   6.7e-15
  B258-L8 end    off          1.7e-13   1.4e-13   1.7e-13   3.3e-16   5.7e-16   5.3e-15
                 small        2.0e-13   1.4e-13   1.1e-13   3.3e-16   5.7e-16   4.4e-15
  B2-L132 straddle            0         0         0         2.2e-18   1.4e-14   4.4e-16
  B2-L132 wrapback            2.9e-11   2.9e-11   2.9e-11   2.2e-16   1.8e-15   8.9e-16   (H about 2e4: 8 ulp)
every accept flag equal to the twin's."""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401

import defect_cases as DC
import defect_hard_cases as DH
import ft_defect_cases as FD
import meta_cases as MC
from oracle import ref_cpu as R

from gpu_support import D, H, angle_close, module_defaults, ops, switches

pytestmark = pytest.mark.gpu
_defaults = module_defaults()

# (path label of the flow, B, L, n_layers, amp, beta, nstep, integrator, defect kind, weight scale): ft_defect_cases' case tuple
BATCH = (('one', 258, 8, 1, math.pi, 2.0, 1, 'leapfrog', 'wrap', 3.0), ('one', 258, 8, 1, 0.3, 6.0, 2, 'omelyan', 'end', 3.0))
L132 = (('tiled', 2, 132, 1, math.pi, 2.0, 1, 'leapfrog', 'straddle', 1.0), ('tiled', 2, 132, 1, 0.3, 6.0, 1, 'leapfrog', 'wrapback', 1.0))
SETTINGS = ('off', 'small')
KEYS = ('x_new', 'dH', 'acc', 'H0', 'H1', 'plaq', 'Q')
ALL = KEYS + ('dsum', 'state')


def case_id(c):
    path, B, L, nl, amp, beta, nstep, integ, dk, sc = c
    return f'B{B}-L{L}-n{nl}-a{amp:.1f}-b{beta:g}-s{nstep}-{integ}-{dk}-w{sc:g}'


def bits(a, b):
    a, b = np.ascontiguousarray(H(a)), np.ascontiguousarray(H(b))
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@functools.lru_cache(maxsize=None)
def inputs(c):
    """FD.inputs with defect_hard_cases' defects and couplings -> (x, v, u, g [B] numpy, defect, flow); shared, read-only"""
    path, B, L, nl, amp, beta, nstep, integ, dk, sc = c
    seed = 7700 + 97 * L + 13 * B + 5 * DH.KINDS.index(dk)
    x = torch.from_numpy(MC.links(B, L, seed, amp))
    v, u = MC.draws(B, L, seed + 1)
    if L == 132:
        u[0] = 0.0                       # one step of this size at L = 132 gains dH of a few units: chain 0 is accepted whatever dH < 700,
                                         # so that x_new is the MD's end point on one chain and the start field on the other
    return x, torch.from_numpy(v), u, DC.couplings(B, beta, DH.KINDS.index(dk)), DH.defect_of(dk, L), FD.flow_of(path, nl, sc)


@functools.lru_cache(maxsize=None)
def twin(c):
    """-> (the twin's force, its action tuple (S, logdet, C, Dsum, Q), its trajectory), computed once"""
    path, B, L, nl, amp, beta, nstep, integ, dk, sc = c
    x, v, u, g, df, flow = inputs(c)
    gt = torch.from_numpy(g)
    with torch.no_grad():
        A = FD.action(x, flow, beta, gt, df)
    return FD.force(x, flow, beta, gt, df), A, FD.trajectory(x, v, u, flow, beta, g, df, FD.DT, nstep, integ)


def dev(c, nl=None):
    path, B, L, n, amp, beta, nstep, integ, dk, sc = c
    x, v, u, g, df, flow = inputs(c)
    nl = n if nl is None else nl
    return D(x), D(v), D(u), (ops.pack_weights(flow, device='cuda') if nl else None), D(g), df


def setting(s):
    return switches(variant=1, small=s == 'small')


def run(c, s, sl=slice(None), g=None, defect=None):
    path, B, L, nl, amp, beta, nstep, integ, dk, sc = c
    x, v, u, w, gd, df = dev(c)
    with setting(s):
        return ops.ft_defect_trajectory(x[sl].clone(), v[sl].clone(), u[sl].clone(), w, nl, beta, (gd if g is None else g)[sl].clone(),
                                        df if defect is None else defect, FD.DT, nstep, integrator=integ)


# ---------------------------------------------------------------- the reference side, on the CPU
def test_the_reference_side_does_not_widen_a_bound():
    """the float64 twin's C and Dsum against defect_cases.sums in long double of the twin's own flowed field: 8 x the figure stays
    inside the bounds used below (C rtol 1e-11, Dsum atol 1e-11), so no bound widens for these shapes; the shapes reach what they
    claim"""
    for c in BATCH + L132:
        path, B, L, nl, amp, beta, nstep, integ, dk, sc = c
        x, v, u, g, df, flow = inputs(c)
        _, (S, ld, C, Dm, Q), tr = twin(c)
        with torch.no_grad():
            y = R.flow_forward(x, flow, 'silu')[0].numpy()
        Cl, Dl, Ql = DC.sums(y, df, np.longdouble)
        fc = float(np.abs((H(C).astype(np.longdouble) - Cl) / Cl).max())
        fd = float(np.abs(H(Dm).astype(np.longdouble) - Dl).max())
        print(f'REFERENCE SIDE {case_id(c)}: C {fc:.2e} relative (bound 1e-11), Dsum {fd:.2e} (bound 1e-11); left out {int(tr["left_out"].sum())}; '
              f'accepted {int(tr["acc"].sum())} of {B}')
        assert 8 * fc <= 1e-11 and 8 * fd <= 1e-11
        assert np.array_equal(np.rint(H(Q)), Ql)
        assert not tr['left_out'].any()
    assert -(-258 // DH.ENERGY_BLOCK) == 2 and 258 % DH.ENERGY_BLOCK == 2
    for c in BATCH:
        assert sorted(inputs(c)[3][255:258]) == [0.0, c[5] / 3.0, c[5]]
    assert 132 * 132 - DH.STRIDE_SITES == 1040


# ---------------------------------------------------------------- force and action against the twin
@pytest.mark.parametrize('c', BATCH + L132, ids=case_id)
def test_force_and_action_against_the_twin(c):
    path, B, L, nl, amp, beta, nstep, integ, dk, sc = c
    x, v, u, w, g, df = dev(c)
    Ft, (St, ldt, ct, dt_, Qt), _ = twin(c)
    for s in (SETTINGS if B > 2 else SETTINGS[:1]):
        with setting(s):
            F = ops.ft_defect_force(x, w, nl, beta, g, df)
            S, ld, cs, ds, Q = ops.ft_defect_action(x, w, nl, beta, g, df)
        fmax = max(1.0, float(Ft.abs().max()))
        print(f'OBSERVED {case_id(c)} {s}: force {np.abs(H(F) - H(Ft)).max() / fmax:.2e} of its scale, S {np.abs((H(S) - H(St)) / H(St)).max():.2e} relative, '
              f'dsum {np.abs(H(ds) - H(dt_)).max():.2e}')
        # tests/test_z_ft_defect_gpu.py: force rtol 1e-8 + 1e-10 of its scale; S, logdet, C rtol 1e-11; Dsum 1e-11; Q 1e-6
        np.testing.assert_allclose(H(F), H(Ft), rtol=1e-8, atol=1e-10 * fmax)
        np.testing.assert_allclose(H(S), H(St), rtol=1e-11)
        np.testing.assert_allclose(H(ld), H(ldt), rtol=1e-11, atol=1e-11)
        np.testing.assert_allclose(H(cs), H(ct), rtol=1e-11)
        np.testing.assert_allclose(H(ds), H(dt_), rtol=0, atol=1e-11)
        np.testing.assert_allclose(H(Q), np.rint(H(Qt)), rtol=0, atol=1e-6)
        for b in ((255, 256, 257) if B > 2 else ()):                          # a chain alone: the same bits
            with setting(s):
                one = ops.ft_defect_action(x[b:b + 1].clone(), w, nl, beta, g[b:b + 1].clone(), df)
                assert bits(ops.ft_defect_force(x[b:b + 1].clone(), w, nl, beta, g[b:b + 1].clone(), df), F[b:b + 1]), (s, b)
            assert all(bits(one[k], (S, ld, cs, ds, Q)[k][b:b + 1]) for k in range(5)), (s, b)


# ---------------------------------------------------------------- whole trajectories against the twin
def check_trajectory(r, ref):
    """tests/test_z_ft_defect_gpu.py's bounds: every accept; x_new 1e-6 as an angle; dH 1e-6 + 1e-6 |dH|; H0 rtol 1e-10; H1 rtol 1e-7; plaq
    rtol 1e-6; Q 1e-6; Dsum 1e-8; the state rows are the outputs"""
    assert np.array_equal(H(r['acc']) > 0.5, ref['acc'])
    angle_close(r['x_new'], ref['x_new'], 1e-6)
    np.testing.assert_allclose(H(r['dH']), ref['dH'], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(H(r['H0']), ref['H0'], rtol=1e-10)
    np.testing.assert_allclose(H(r['H1']), ref['H1'], rtol=1e-7)
    np.testing.assert_allclose(H(r['plaq']), ref['plaq'], rtol=1e-6)
    np.testing.assert_allclose(H(r['Q']), ref['Q'], rtol=0, atol=1e-6)
    np.testing.assert_allclose(H(r['dsum']), ref['dsum'], rtol=0, atol=1e-8)
    st = H(r['state'])
    assert bits(st[1], r['plaq']) and bits(st[2], r['Q']) and bits(st[3], r['dsum'])


@pytest.mark.parametrize('c', BATCH, ids=case_id)
def test_trajectory_of_258_chains_on_the_sequenced_path_and_in_the_one_launch_kernel(c):
    path, B, L, nl, amp, beta, nstep, integ, dk, sc = c
    ref = twin(c)[2]
    assert not ref['left_out'].any() and ref['acc'].any() and not ref['acc'].all()
    res = {}
    for s in SETTINGS:
        r = res[s] = run(c, s)
        print(f'OBSERVED {case_id(c)} {s}: ' + ' '.join(f'{k} {np.abs(H(r[k]) - ref[k]).max():.2e}' for k in ('dH', 'H0', 'H1', 'plaq', 'Q', 'dsum')))
        check_trajectory(r, ref)
        assert all(bits(run(c, s)[k], r[k]) for k in ALL), s                  # two calls, the same bits
        for b in (0, 255, 256, 257):                                          # either side of the edge of launch_defect_energy's workgroup
            one = run(c, s, sl=slice(b, b + 1))
            assert all(bits(H(r[k])[b:b + 1] if k != 'state' else H(r[k])[:, b:b + 1], one[k]) for k in ALL), (s, b)
    # the two settings: the same accepts, and fields within the sum of the two paths' bounds against the twin (tests/test_z_ft_meta_gpu.py)
    a, b = res['small'], res['off']
    assert np.array_equal(H(a['acc']), H(b['acc']))
    angle_close(a['x_new'], b['x_new'], 2e-6)
    np.testing.assert_allclose(H(a['dH']), H(b['dH']), rtol=2e-6, atol=2e-6)
    np.testing.assert_allclose(H(a['H0']), H(b['H0']), rtol=2e-10)
    np.testing.assert_allclose(H(a['dsum']), H(b['dsum']), rtol=0, atol=2e-8)


@pytest.mark.parametrize('c', L132, ids=case_id)
def test_one_leapfrog_step_with_the_defect_across_the_pass_edge_of_the_seed(c):
    ref = twin(c)[2]
    assert not ref['left_out'].any() and ref['acc'].tolist() == [True, False]
    r = run(c, 'off')
    print(f'OBSERVED {case_id(c)}: ' + ' '.join(f'{k} {np.abs(H(r[k]) - ref[k]).max():.2e}' for k in ('dH', 'H0', 'H1', 'plaq', 'Q', 'dsum')))
    check_trajectory(r, ref)
    assert all(bits(run(c, 'off')[k], r[k]) for k in ALL)


# ---------------------------------------------------------------- what the defect must not change, and what no layers reduce to
@pytest.mark.parametrize('c', BATCH + L132, ids=case_id)
def test_g_equal_to_beta_and_an_empty_defect_give_the_bits_of_ft_trajectory(c):
    path, B, L, nl, amp, beta, nstep, integ, dk, sc = c
    x, v, u, w, g, df = dev(c)
    for s in (SETTINGS if B > 2 else SETTINGS[:1]):
        with setting(s):
            p = ops.ft_trajectory(x, v, u, w, nl, beta, FD.DT, nstep, integrator=integ)
        r = run(c, s, g=torch.full_like(g, beta))
        e = run(c, s, defect=(df[0], df[1], 0))
        for k in KEYS:
            assert bits(r[k], p[k]) and bits(e[k], p[k]), (s, k)
        assert bits(r['state'][:3], p['state']) and bits(e['state'][:3], p['state']) and not H(e['dsum']).any()


@pytest.mark.parametrize('c', BATCH + L132, ids=case_id)
def test_no_layers_gives_the_bits_of_the_plain_trajectory_with_a_defect(c):
    """n_layers = 0: ops.defect_trajectory's sequenced path bit for bit, except Q (the flowed call hands out the sum of
    the wrapped plaquettes over 2 pi as it comes, the plain call the integer)"""
    path, B, L, nl, amp, beta, nstep, integ, dk, sc = c
    x, v, u, w, g, df = dev(c, nl=0)
    r = ops.ft_defect_trajectory(x, v, u, None, 0, beta, g, df, FD.DT, nstep, integrator=integ)
    p = ops.defect_trajectory(x, v, u, beta, g, df, FD.DT, nstep, integrator=integ, path=2)
    for k in ('x_new', 'dH', 'acc', 'H0', 'H1', 'dsum'):
        assert bits(r[k], p[k]), k
    assert np.array_equal(np.rint(H(r['Q'])), H(p['Q'])) and np.abs(H(r['Q']) - H(p['Q'])).max() <= 1e-12
    np.testing.assert_allclose(H(r['plaq']) * (L * L), H(p['csum']), rtol=1e-14)
