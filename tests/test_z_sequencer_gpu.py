"""GPU tests of the two host sequencers of csrc/api.hip -- hmc_trajectory_call (plain) and ft_trajectory_call (flowed), each with
its optional bias -- on the branches at the smallest shape with two table rows of two chains each: B = 4, L = 8, G = 2, where a
row offset or a 3 B / 4 B / 5 B row stride can still go wrong, and L = 20 for the tuned branch (16 x 16 tiles do not divide it).

Which of these branches the other GPU files reach (read from their case tables):
  plain, biased, path 2: {leapfrog, force_gradient} x {fresh x_new, x itself} -- all reached (test_z_meta_gpu.py runs every biased
    case of meta_cases.CASES on path 2 with both outputs), none with more than one chain per table row and more than one row;
  flowed, biased, tuned branch: reached without a carried state by every integrator (ft_meta_cases 'off', 'tiled'); carried with the
    leapfrog ('off', B = 3, G = 1) and force_gradient ('tiled', L = 20, B = G = 2); NOT carried x force_gradient with the small path off at L <= 16;
  flowed, biased, generic net: leapfrog and omelyan, fresh and carried; NOT force_gradient (either state);
  flowed, biased, 0 layers: force_gradient (G = 1) and leapfrog (G = B = 2), fresh and carried -- all reached, one chain per row;
  flowed, unbiased, per-chain beta, 0 layers: the leapfrog at L = 128, B = 2 (tempering_cases 'plain-ft-L128'); NOT force_gradient, NOT carried.
The whole grid is run here at the one shape, so that every branch meets the two-chains-per-row layout.

What is asserted is what those files assert, with their bounds: with a zero table (nb = 11) and wall = 0 the bits of the unbiased twin
call; with the rough table of meta_cases.table (G = 2; that table has nb = 41) the numpy / torch twin within test_z_meta_gpu.py's
and test_z_ft_meta_gpu.py's bounds; state[k] bit-equal to the plaq / Q / qm vectors handed out beside it; a carried state gives the
bits of the stateless call."""
import math

import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401

import ft_meta_cases as FC
import meta_cases as MC
import tempering_cases as TC

from gpu_support import D, H, angle_close, module_defaults, ops, switches

pytestmark = pytest.mark.gpu
_defaults = module_defaults()

B, G, NB0 = 4, 2, 11
INTEGS = ('leapfrog', 'force_gradient')
KEYS = ('x_new', 'dH', 'acc', 'H0', 'H1', 'plaq', 'Q')
ALL = KEYS + ('qm', 'vbias', 'state')


def bits(a, b):
    a, b = np.ascontiguousarray(H(a)), np.ascontiguousarray(H(b))
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def zero_table():
    return torch.zeros(G, NB0, dtype=torch.float64, device='cuda'), 3.0, 0.0


# ---------------------------------------------------------------- plain, biased, sequenced
# field amplitudes at which the twin accepts some chains of the batch and rejects others, so that the Metropolis kernel selects old
# rows and new ones (read off the twin alone); at L = 20 the leapfrog's batch is all accepted
AMP = 1.5
AMP_L20 = {'leapfrog': 0.3, 'force_gradient': math.pi}
PLAIN = [(B, 8, AMP, 2.0, 2, integ, 'rough', G) for integ in INTEGS]             # meta_cases' case tuple


def plain_in_place(x, v, u, beta, dt, nstep, integ):
    """the unbiased sequenced trajectory at any L: fthmc_hmc_trajectory_int with x_new aliasing x (C ABI directly: ops.hmc_trajectory
    refuses the alias) -> dict as ops.hmc_trajectory"""
    from fthmc_amd import _lib
    n, _, L, _ = x.shape
    xd = x.clone()
    o = {k: torch.empty(n, dtype=torch.float64, device='cuda') for k in ('dH', 'acc', 'H0', 'H1')}
    ws, nb = ops._ws(xd, n, L, 0)
    rc = _lib.load().fthmc_hmc_trajectory_int(ops._p(xd), ops._p(v), ops._p(u), n, L, beta, dt, nstep, _lib.INTEGRATORS[integ], ops._p(xd),
                                              ops._p(o['dH']), ops._p(o['acc']), ops._p(o['H0']), ops._p(o['H1']), ws, nb, ops._stream(xd))
    assert rc == 0
    o['x_new'] = xd
    return o


def plain_call(x, v, u, c, V, qmax, wall, alias):
    _, L, amp, beta, nstep, integ, tk, _ = c
    xa = x.clone()
    out = {'x_new': xa} if alias else None
    r = ops.meta_trajectory(xa, v, u, beta, MC.DT, nstep, V, qmax, wall, integrator=integ, path=2, out=out)
    assert (r['x_new'].data_ptr() == xa.data_ptr()) == alias
    return r


@pytest.mark.parametrize('alias', (False, True), ids=('fresh', 'alias'))
@pytest.mark.parametrize('c', PLAIN, ids=MC.case_id)
def test_plain_zero_table_gives_the_bits_of_the_unbiased_sequence(c, alias):
    _, L, amp, beta, nstep, integ, tk, _ = c
    x, v, u = (D(a) for a in MC.case(c)[:3])
    r = plain_call(x, v, u, c, *zero_table(), alias)
    p = plain_in_place(x, v, u, beta, MC.DT, nstep, integ)
    for k in ('x_new', 'dH', 'acc', 'H0', 'H1'):
        assert bits(r[k], p[k]), k
    assert not H(r['vbias']).any()
    np.testing.assert_allclose(H(r['qm']), MC.f64(MC.charge_m(H(r['x_new']), MC.LD)), rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize('alias', (False, True), ids=('fresh', 'alias'))
@pytest.mark.parametrize('c', PLAIN, ids=MC.case_id)
def test_plain_rough_table_against_the_twin(c, alias):
    """test_z_meta_gpu.check_traj's bounds"""
    x, v, u, tab, ref = MC.case(c)
    assert tab.G == G and not ref['left_out'].any()
    r = plain_call(D(x), D(v), D(u), c, D(tab.V), tab.qmax, tab.wall, alias)
    for k in ('x_new', 'dH', 'H0', 'H1', 'qm', 'vbias'):
        print(k, float(np.abs(H(r[k]).astype(MC.LD) - ref[k]).max()))
    close = lambda a, b, rtol=1e-10, atol=1e-10: np.testing.assert_allclose(H(a), MC.f64(b), rtol=rtol, atol=atol)
    assert np.array_equal(H(r['acc']) > 0.5, ref['acc'])
    close(r['H0'], ref['H0'], rtol=1e-10)
    close(r['H1'], ref['H1'], rtol=1e-8)
    close(r['dH'], ref['dH'], rtol=1e-8, atol=1e-9)
    close(r['x_new'], ref['x_new'], atol=1e-9)
    close(r['qm'], ref['qm'], rtol=1e-9, atol=1e-10)
    close(r['vbias'], ref['vbias'], rtol=1e-8, atol=1e-9)


# ---------------------------------------------------------------- flowed, biased
# ft_meta_cases' case tuple; 'off': the small path off -- the tuned branch at L = 8 and, ragged, at L = 20
FLOWED = [(path, B, L, nl, AMP_L20[integ] if L == 20 else AMP, 2.0, 2, integ, 'rough', G, 1.0)
          for path, L, nl in (('off', 8, 2), ('off', 20, 2), ('gen', 8, 2), ('nolayers', 8, 0)) for integ in INTEGS]
CARRIED = (False, True)


def flowed_inputs(c, table, carried):
    """-> (x, v, u, w, flow): the case's inputs, or -- carried -- the end of a first trajectory under `table` from them: its x_new,
    fresh draws and its state [4, B] as a fifth element"""
    path, _, L, nl, amp, beta, nstep, integ, tk, _, sc = c
    x, v, u, _, flow = FC.inputs(c)
    w = ops.pack_weights(flow, device='cuda') if nl else None
    x, v, u = D(x), D(v), D(u)
    if not carried:
        return x, v, u, w, flow, None
    a = ops.ft_meta_trajectory(x, v, u, w, nl, beta, FC.DT, nstep, *table, integrator=integ)
    v2, u2 = MC.draws(B, L, FC.case_seed(c) + 2)
    return a['x_new'].clone(), D(v2), D(u2), w, flow, a['state'].clone()


@pytest.mark.parametrize('carried', CARRIED, ids=('fresh', 'carried'))
@pytest.mark.parametrize('c', FLOWED, ids=FC.case_id)
def test_flowed_zero_table_gives_the_bits_of_ft_trajectory(c, carried):
    path, _, L, nl, amp, beta, nstep, integ, tk, _, sc = c
    Z = zero_table()
    with switches(small=False):
        x, v, u, w, flow, st = flowed_inputs(c, Z, carried)
        r = ops.ft_meta_trajectory(x, v, u, w, nl, beta, FC.DT, nstep, *Z, integrator=integ, state_in=st)
        p = ops.ft_trajectory(x, v, u, w, nl, beta, FC.DT, nstep, integrator=integ, state_in=None if st is None else st[:3].contiguous())
    for k in KEYS:
        assert bits(r[k], p[k]), k
    assert bits(r['state'][:3], p['state']) and not H(r['vbias']).any()
    s = H(r['state'])
    assert bits(s[1], r['plaq']) and bits(s[2], r['Q']) and bits(s[3], r['qm'])


@pytest.mark.parametrize('carried', CARRIED, ids=('fresh', 'carried'))
@pytest.mark.parametrize('c', FLOWED, ids=FC.case_id)
def test_flowed_rough_table_against_the_twin(c, carried):
    """test_z_ft_meta_gpu.test_biased_trajectory_against_the_twin's bounds; the carried call gives the stateless call's bits"""
    path, _, L, nl, amp, beta, nstep, integ, tk, _, sc = c
    tab = FC.inputs(c)[3]
    assert tab.G == G
    T = (D(tab.V), tab.qmax, tab.wall)
    with switches(small=False):
        x, v, u, w, flow, st = flowed_inputs(c, T, carried)
        r = ops.ft_meta_trajectory(x, v, u, w, nl, beta, FC.DT, nstep, *T, integrator=integ, state_in=st)
        if carried:
            s0 = ops.ft_meta_trajectory(x, v, u, w, nl, beta, FC.DT, nstep, *T, integrator=integ)
            assert all(bits(r[k], s0[k]) for k in ALL)
    ref = FC.trajectory(x.cpu(), v.cpu(), H(u), flow, beta, FC.DT, nstep, integ, tab)
    assert not ref['left_out'].any()
    for k in ('dH', 'H0', 'H1', 'plaq', 'Q', 'qm', 'vbias'):
        print(k, np.abs(H(r[k]) - ref[k]).max())
    assert np.array_equal(H(r['acc']) > 0.5, ref['acc'])
    angle_close(r['x_new'], ref['x_new'], 1e-6)
    np.testing.assert_allclose(H(r['dH']), ref['dH'], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(H(r['H0']), ref['H0'], rtol=1e-10)
    np.testing.assert_allclose(H(r['H1']), ref['H1'], rtol=1e-7)
    np.testing.assert_allclose(H(r['plaq']), ref['plaq'], rtol=1e-6)
    np.testing.assert_allclose(H(r['Q']), ref['Q'], rtol=0, atol=1e-6)
    slope = max(1.0, float(np.abs(np.diff(tab.V, axis=1)).max() / ((2 * tab.qmax) / (tab.nb - 1))), tab.wall)
    np.testing.assert_allclose(H(r['qm']), ref['qm'], rtol=0, atol=1e-9)
    np.testing.assert_allclose(H(r['vbias']), ref['vbias'], rtol=0, atol=1e-9 * slope)
    s = H(r['state'])
    assert bits(s[1], r['plaq']) and bits(s[2], r['Q']) and bits(s[3], r['qm'])


# ---------------------------------------------------------------- flowed, unbiased, per-chain beta, no layers (pb_eval beside the rows)
@pytest.mark.parametrize('carried', CARRIED, ids=('fresh', 'carried'))
@pytest.mark.parametrize('integ', INTEGS)
def test_per_chain_beta_without_layers_is_the_scalar_call(integ, carried):
    """test_tempering_gpu.py's statement A: a constant beta_b gives the scalar call's bits, the beta-free state its state"""
    L, beta, nstep = 8, 2.3, 2
    c = ('nolayers', B, L, 0, AMP, beta, nstep, integ, 'rough', G, 1.0)
    x, v, u = (D(a) for a in FC.inputs(c)[:3])
    bb = torch.full((B,), beta, dtype=torch.float64, device='cuda')
    st_pb = st = None
    if carried:
        a = ops.ft_trajectory(x, v, u, None, 0, bb, FC.DT, nstep, integrator=integ)
        a0 = ops.ft_trajectory(x, v, u, None, 0, beta, FC.DT, nstep, integrator=integ)
        assert bits(a['x_new'], a0['x_new'])
        v2, u2 = MC.draws(B, L, FC.case_seed(c) + 2)
        x, v, u, st_pb, st = a['x_new'].clone(), D(v2), D(u2), a['state'].clone(), a0['state'].clone()
    r = ops.ft_trajectory(x, v, u, None, 0, bb, FC.DT, nstep, integrator=integ, state_in=st_pb)
    p = ops.ft_trajectory(x, v, u, None, 0, beta, FC.DT, nstep, integrator=integ, state_in=st)
    for k in KEYS:
        assert bits(r[k], p[k]), k
    assert TC.state_matches(H(r['state']), np.full(B, beta), L, H(p['state']))
    assert np.array_equal(TC.state_to_scalar(H(r['state']), np.full(B, beta), L)[2], H(r['plaq'])) and bits(r['state'][2], r['Q'])
