"""GPU tests of metadynamics HMC (csrc/meta.hip) against the numpy twin of tests/meta_cases.py.  (Named to be collected behind every other
GPU test file; nothing here or there depends on the order: the module sets the library's default variant and small path, as the
other GPU modules do, and keeps its scratch in a cache family of its own.)

Cases (meta_cases.CASES): (B, L) in {(3, 4), (2, 8), (5, 12), (2, 20), (3, 32), (2, 64)} on the one-launch and the sequenced path,
(2, 68) and (1, 128) on the sequenced path; field amplitudes pi and 0.3, beta 2 and 6, nstep 1 and 3, the three integrators; a zero
table, a smooth quadratic one and a rough one drawn once (node-to-node steps up to 3, nb = 41 on |q| <= 2, wall 10: chains of the
rough fields sit on the wall); one shared row and one row per chain.

Bounds: the project's figures for the plain kernels (tests/test_integrators_gpu.py: H0 rtol 1e-10, forces 1e-11 of their scale,
x_new atol 1e-9, dH rtol 1e-8 / atol 1e-9, H1 rtol 1e-8).  The float64 twin against the long double twin on these cases
(tests/test_meta.py, measured): force 2.4e-15 of its scale, S_b 5.2e-14 relative, x_new 2.1e-15, H1 1.4e-14 relative, dH 5.7e-7 of
its bound -- 8 x each is far inside the figures above, so no table widens a bound.  Accept flags are compared on every chain: the
twin leaves none out on these inputs (min |t - round(t)| >= 1e-9 at every lookup, |u - exp(-dH)| >= 1e-6 exp(-dH))."""
import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401

import meta_cases as MC

import gpu_support
from gpu_support import D, H, module_defaults, ops, switches

pytestmark = pytest.mark.gpu
_defaults = module_defaults()

LD = np.longdouble
Q2_EXACT_L16_B6 = 1.1947014482


def close(a, b, rtol=1e-10, atol=1e-10):
    """against the twin's longdouble figures, rounded to fp64 first"""
    gpu_support.close(a, MC.f64(b), rtol=rtol, atol=atol)


def bits(a, b):
    a, b = H(a), H(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def paths_of(L):
    return (1, 2) if L <= 64 else (2,)


def dev_case(c):
    x, v, u, tab, ref = MC.case(c)
    return D(x), D(v), D(u), D(tab.V), tab, ref


def run(c, path, out=None, integrator=None):
    B, L, amp, beta, nstep, integ, tk, G = c
    x, v, u, V, tab, ref = dev_case(c)
    return ops.meta_trajectory(x, v, u, beta, MC.DT, nstep, V, tab.qmax, tab.wall, integrator=integrator or integ, path=path, out=out)


def parent_in_place(x, v, u, beta, dt, nstep, integ):
    """the parent's sequenced trajectory at any L: fthmc_hmc_trajectory_int with x_new aliasing x (C ABI directly: ops.hmc_trajectory
    refuses the alias) -> dict as ops.hmc_trajectory"""
    from fthmc_amd import _lib
    B, _, L, _ = x.shape
    xd = x.clone()
    o = {k: torch.empty(B, dtype=torch.float64, device='cuda') for k in ('dH', 'acc', 'H0', 'H1')}
    ws, nb = ops._ws(xd, B, L, 0)
    rc = _lib.load().fthmc_hmc_trajectory_int(ops._p(xd), ops._p(v), ops._p(u), B, L, beta, dt, nstep, _lib.INTEGRATORS[integ], ops._p(xd),
                                              ops._p(o['dH']), ops._p(o['acc']), ops._p(o['H0']), ops._p(o['H1']), ws, nb, ops._stream(xd))
    assert rc == 0
    o['x_new'] = xd
    return o


ZERO = [c for c in MC.CASES if c[6] == 'zero']
BIASED = [c for c in MC.CASES if c[6] != 'zero']


# ---------------------------------------------------------------- zero table: the plain kernels' bits
@pytest.mark.parametrize('c', ZERO, ids=MC.case_id)
def test_zero_table_gives_the_plain_trajectory_bit_for_bit(c):
    B, L, amp, beta, nstep, integ, tk, G = c
    x, v, u, V, tab, ref = dev_case(c)
    assert tab.wall == 0.0 and not tab.V.any()
    for path in paths_of(L):
        r = run(c, path)
        if path == 1:
            p = ops.hmc_trajectory(x, v, u, beta, MC.DT, nstep, integrator=integ)          # L <= 64: the one-launch kernels
        else:
            p = parent_in_place(x, v, u, beta, MC.DT, nstep, integ)                         # the sequenced form
        for k in ('x_new', 'dH', 'acc', 'H0', 'H1'):
            assert bits(r[k], p[k]), (path, k, float(np.abs(H(r[k]) - H(p[k])).max()))
        assert not H(r['vbias']).any()
        close(r['qm'], ref['qm'], rtol=1e-11, atol=1e-12)
    if L > 64:                                                                              # there ops.hmc_trajectory is the sequenced form too
        p = ops.hmc_trajectory(x, v, u, beta, MC.DT, nstep, integrator=integ)
        assert all(bits(r[k], p[k]) for k in ('x_new', 'dH', 'acc', 'H0', 'H1'))


# ---------------------------------------------------------------- the bias on its own
@pytest.mark.parametrize('c', MC.CASES, ids=MC.case_id)
def test_force_and_action_against_the_long_double_twin(c):
    B, L, amp, beta, nstep, integ, tk, G = c
    x, v, u, V, tab, ref = dev_case(c)
    xh = MC.case(c)[0]
    Fr, margin = MC.force(xh, beta, tab, LD)
    assert margin.min() >= MC.T_MARGIN
    F = ops.meta_force(x, beta, V, tab.qmax, tab.wall)
    scale = float(np.abs(Fr).max())
    err = float(np.abs(H(F).astype(LD) - Fr).max())
    Sr, qr, vr, _ = MC.biased_action(xh, beta, tab, LD)
    S, qm, vb = ops.meta_action(x, beta, V, tab.qmax, tab.wall)
    print(f'force: {err / scale:.2e} of its scale {scale:.2e}; S_b {float(np.abs((H(S) - Sr) / Sr).max()):.2e} relative')
    assert err <= 1e-11 * scale
    close(S, Sr, rtol=1e-10); close(qm, qr, rtol=1e-11, atol=1e-12); close(vb, vr, rtol=1e-10)
    # the same field through ops.wilson_force where there is no bias
    if tk == 'zero':
        close(F, H(ops.wilson_force(x, beta)), rtol=0, atol=1e-13 * scale)
    # each output is optional
    only = ops.meta_action(x, beta, V, tab.qmax, tab.wall, out={'qm': torch.empty(B, dtype=torch.float64, device='cuda')})
    assert bits(only[1], qm) and bits(only[0], S)


# ---------------------------------------------------------------- the biased trajectory against the twin
def check_traj(r, ref):
    assert not ref['left_out'].any()
    assert np.array_equal(H(r['acc']) > 0.5, ref['acc'])
    close(r['H0'], ref['H0'], rtol=1e-10)
    close(r['H1'], ref['H1'], rtol=1e-8)
    close(r['dH'], ref['dH'], rtol=1e-8, atol=1e-9)
    close(r['x_new'], ref['x_new'], atol=1e-9)
    close(r['qm'], ref['qm'], rtol=1e-9, atol=1e-10)                     # of the selected end
    close(r['vbias'], ref['vbias'], rtol=1e-8, atol=1e-9)


@pytest.mark.parametrize('c', BIASED, ids=MC.case_id)
def test_biased_trajectory_against_the_twin_on_every_path(c):
    B, L, amp, beta, nstep, integ, tk, G = c
    x, v, u, V, tab, ref = dev_case(c)
    res = {}
    for path in paths_of(L):
        r = res[path] = run(c, path)
        print(f'path {path}: x_new {float(np.abs(H(r["x_new"]).astype(LD) - ref["x_new"]).max()):.2e}, dH '
              f'{float(np.abs(H(r["dH"]).astype(LD) - ref["dH"]).max()):.2e} (|dH| up to {float(np.abs(ref["dH"]).max()):.2e}), '
              f'accepted {int(ref["acc"].sum())} of {B}')
        check_traj(r, ref)
        # qm / vbias belong to the field x_new holds
        S, qm, vb = ops.meta_action(r['x_new'], beta, V, tab.qmax, tab.wall)
        close(r['qm'], H(qm), rtol=1e-9, atol=1e-10); close(r['vbias'], H(vb), rtol=1e-8, atol=1e-9)
        assert all(bits(run(c, path)[k], r[k]) for k in r)                                  # two calls, the same bits
    if len(res) == 2:                                                                       # path against path: the sum of their bounds
        a, b = res[1], res[2]
        assert bits(a['acc'], b['acc'])
        close(a['x_new'], H(b['x_new']), rtol=2e-10, atol=2e-9); close(a['dH'], H(b['dH']), rtol=2e-8, atol=2e-9)
        close(a['H1'], H(b['H1']), rtol=2e-8); close(a['H0'], H(b['H0']), rtol=2e-10, atol=2e-10)
        assert all(bits(run(c, 0)[k], a[k]) for k in a)                                     # path 0 is path 1 where it is served
    else:
        assert all(bits(run(c, 0)[k], res[2][k]) for k in res[2])
    # aliased output on the sequenced path equals separate output
    xa = x.clone()
    ra = ops.meta_trajectory(xa, v, u, beta, MC.DT, nstep, V, tab.qmax, tab.wall, integrator=integ, path=2, out={'x_new': xa})
    assert ra['x_new'].data_ptr() == xa.data_ptr() and all(bits(ra[k], res[2][k]) for k in ra)
    ra0 = ops.meta_trajectory(xa.copy_(x), v, u, beta, MC.DT, nstep, V, tab.qmax, tab.wall, integrator=integ, path=0, out={'x_new': xa})
    assert all(bits(ra0[k], res[2][k]) for k in ra0)                                        # and path 0 takes it there


@pytest.mark.parametrize('c', [c for c in BIASED if c[7] == c[0] and c[0] > 1], ids=MC.case_id)
def test_a_chain_of_a_batch_equals_the_chain_alone(c):
    B, L, amp, beta, nstep, integ, tk, G = c
    x, v, u, V, tab, ref = dev_case(c)
    for path in paths_of(L):
        r = run(c, path)
        for b in (0, B - 1):
            one = ops.meta_trajectory(x[b:b + 1].clone(), v[b:b + 1].clone(), u[b:b + 1].clone(), beta, MC.DT, nstep, V[b:b + 1].clone(),
                                      tab.qmax, tab.wall, integrator=integ, path=path)
            assert all(bits(one[k], r[k][b:b + 1]) for k in r), (path, b)
    Fb = ops.meta_force(x, beta, V, tab.qmax, tab.wall)
    assert bits(ops.meta_force(x[1:2].clone(), beta, V[1:2].clone(), tab.qmax, tab.wall), Fb[1:2])


def test_scratch_is_asked_for_only_on_the_sequenced_path():
    c = next(c for c in BIASED if c[1] == 8)
    B, L, amp, beta, nstep, integ, tk, G = c
    x, v, u, V, tab, ref = dev_case(c)
    meta_keys = lambda: [k for k in ops._WS if k[-1] == 'meta']
    ops.release_workspaces()
    r0 = run(c, 0); r1 = run(c, 1)
    assert not meta_keys()                                               # one launch: no workspace
    run(c, 2)
    assert len(meta_keys()) == 1 and ops._WS[meta_keys()[0]].numel() * 8 >= ops.meta_ws_bytes(B, L, 2) > 0
    ops.release_workspaces()
    xa = x.clone()
    ops.meta_trajectory(xa, v, u, beta, MC.DT, nstep, V, tab.qmax, tab.wall, integrator=integ, path=0, out={'x_new': xa})
    assert len(meta_keys()) == 1                                         # path 0 with aliased output: the sequenced path
    ops.release_workspaces()
    with switches(variant=0):                                            # ... and with the VALU variant set, as fthmc_hmc_trajectory_int chooses
        rv = run(c, 0)
        assert len(meta_keys()) == 1 and all(bits(rv[k], run(c, 2)[k]) for k in rv)
    assert all(bits(r0[k], r1[k]) for k in r0)
    # more chains than the sequenced path's launch shapes serve: refused, nothing launched
    from fthmc_amd._lib import FthmcError
    big = torch.zeros(65536, 2, 4, 4, dtype=torch.float64, device='cuda')
    with pytest.raises(FthmcError):
        ops.meta_trajectory(big, big, torch.zeros(65536, dtype=torch.float64, device='cuda'), 2.0, 0.1, 1, V[:1].clone(), tab.qmax, path=2)
    ops.release_workspaces()


def test_refusals_through_the_wrappers():
    x = torch.zeros(4, 2, 8, 8, dtype=torch.float64, device='cuda')
    u = torch.zeros(4, dtype=torch.float64, device='cuda')
    V = torch.zeros(2, 11, dtype=torch.float64, device='cuda')
    with pytest.raises(ValueError):
        ops.meta_trajectory(x, x, u, 2.0, 0.1, 1, V, 2.0, path=1, out={'x_new': x})
    with pytest.raises(ValueError):
        ops.meta_trajectory(x, x, u, 2.0, 0.1, 1, torch.zeros(3, 11, dtype=torch.float64, device='cuda'), 2.0)
    with pytest.raises(ValueError):
        ops.meta_trajectory(x, x, u, 2.0, 0.1, 1, V, 2.0, integrator='rk4')
    with pytest.raises(ValueError):
        ops.meta_deposit(u, V, 2.0, -1.0)


# ---------------------------------------------------------------- deposit
def test_deposit_is_the_twins_statement_in_chain_order():
    rng = np.random.default_rng(41)
    # one shared row, 257 walkers: several per node, some outside, the edges themselves
    q = rng.uniform(-2.4, 2.4, 257)
    q[:6] = (2.0, -2.0, 2.0000001, -2.0000001, 0.0, np.nextafter(2.0, 0))
    V0 = rng.normal(size=(1, 81))
    tab = MC.Table(V0, 2.0, 0.0).deposit(q, 0.0025)
    Vd = D(V0)
    assert ops.meta_deposit(D(q), Vd, 2.0, 0.0025) is Vd
    assert bits(Vd, tab.V)
    assert float(np.abs(tab.V - V0).sum()) > 0.0025 * 150
    # a second deposit on top of the first (the table is read in place)
    q2 = rng.uniform(-2.0, 2.0, 257)
    ops.meta_deposit(D(q2), Vd, 2.0, 0.01)
    assert bits(Vd, tab.deposit(q2, 0.01).V)
    # one row per chain: walkers outside add nothing, the other rows are untouched
    qb = np.array([0.3, 5.0, -1.99, np.nan, -7.0])
    Vb0 = rng.normal(size=(5, 41))
    tb = MC.Table(Vb0, 2.0, 0.0).deposit(qb, 0.5)
    Vb = D(Vb0)
    ops.meta_deposit(D(qb), Vb, 2.0, 0.5)
    assert bits(Vb, tb.V)
    assert bits(Vb[[1, 3, 4]], Vb0[[1, 3, 4]]) and not bits(Vb[0], Vb0[0]) and int((H(Vb) != Vb0).sum()) == 4
    # two rows of several walkers, a table of the largest and the smallest size
    for G, nb in ((2, 65536), (4, 2)):
        qg = rng.uniform(-1.2, 1.2, 64)
        Vg0 = np.zeros((G, nb))
        Vg = D(Vg0)
        ops.meta_deposit(D(qg), Vg, 1.0, 0.125)
        assert bits(Vg, MC.Table(Vg0, 1.0, 0.0).deposit(qg, 0.125).V)
    # w = 0 leaves the bits
    ops.meta_deposit(D(q), Vd, 2.0, 0.0)
    assert bits(Vd, tab.V)


# ---------------------------------------------------------------- the driver
def _param(**kw):
    from fthmc_amd.config import Param
    return Param(**kw)


def test_run_meta_captured_equals_eager():
    from fthmc_amd.meta import MetaPotential, run_meta
    x0 = D(MC.links(6, 8, 77, 1.0))
    out = []
    for use_graph in (True, False):
        pot = MetaPotential(41, 2.0, 10.0, groups=2)
        f, h, p = run_meta(_param(beta=3.0, L=8, tau=0.6, nstep=3, ntraj=7, nrun=2, seed=5), x=x0, potential=pot, n_build=9, w=0.05,
                           integrator='omelyan', use_graph=use_graph)
        assert p is pot
        out.append((f, h, pot.numpy()))
    (fa, ha, ta), (fb, hb, tb) = out
    assert bits(ta, tb) and ta.any() and all(bits(a, b) for a, b in zip(fa, fb))
    for n in (0, 1):
        assert ha[n]['build'] == hb[n]['build'] == [n * 7 + i < 9 for i in range(7)]
        assert ha[n]['traj'] == [n * 7 + i + 1 for i in range(7)]
        for k in ('acc', 'dH', 'plaq', 'q', 'dq', 'qm', 'vbias'):
            assert len(ha[n][k]) == 7 and all(bits(a, b) for a, b in zip(ha[n][k], hb[n][k])), k
    # the deposits are the twin's: the table is the sum of the hills at the recorded Q_m, in trajectory and chain order
    tw = MC.Table(np.zeros((2, 41)), 2.0, 10.0)
    for n in (0, 1):
        for i in range(7):
            if ha[n]['build'][i]:
                tw.deposit(H(ha[n]['qm'][i]), 0.05)
    assert bits(ta, tw.V)
    # and the static trajectories' weights are the frozen table's
    from fthmc_amd.meta import MetaPotential as MP
    frozen = MP(41, 2.0, 10.0, groups=2).load_state_dict(pot.state_dict())
    for g in (0, 1):
        np.testing.assert_allclose(H(ha[1]['vbias'][-1])[3 * g:3 * g + 3], frozen.value(H(ha[1]['qm'][-1])[3 * g:3 * g + 3], g), rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize('integ', ['leapfrog', 'force_gradient'])
def test_run_meta_without_a_bias_is_the_plain_hmc_loop(integ):
    from fthmc_amd.meta import run_meta
    par = _param(beta=4.0, L=8, tau=0.5, nstep=5, ntraj=6, nrun=1, seed=17)
    x0 = D(MC.links(4, 8, 78, 0.5))
    f, h, pot = run_meta(par, x=x0, integrator=integ)
    assert not pot.numpy().any() and pot.wall == 0.0
    x = x0.clone()
    for t in range(par.ntraj):
        seeds = ops.chain_seeds(par.seed, 0, 4, t, device=x.device)
        v, u = ops.random_momenta(seeds, x.shape)
        r = ops.hmc_trajectory(x, v, u, par.beta, par.dt, par.nstep, integrator=integ)
        x = r['x_new']
        S, Q, plaq = ops.wilson_action_charge(x, par.beta)
        assert bits(h[0]['dH'][t], r['dH']) and bits(h[0]['acc'][t], r['acc']) and bits(h[0]['plaq'][t], plaq) and bits(h[0]['q'][t], Q), t
        assert not H(h[0]['vbias'][t]).any()
    assert bits(f[0], x)


# ---------------------------------------------------------------- physics: what the feature is for
def test_metadynamics_unfreezes_the_charge_and_reweights_to_the_exact_moment():
    """L = 16, beta = 6, 256 chains cold, one shared table (nb = 81, qmax = 4, wall = 50), w = 0.0025, 300 build + 400 static leapfrog
    trajectories (tau = 1, 10 steps): the reweighted <Q^2> (jackknife over the chains) within |z| <= 4 of the exact 1.1947014482, and
    more tunnelling per static trajectory than the same 700 trajectories under a zero table with w = 0."""
    from fthmc_amd.meta import MetaPotential, run_meta
    from fthmc_amd.utils.observables import reweighted_mean
    par = _param(beta=6.0, L=16, tau=1.0, nstep=10, ntraj=700, nrun=1, seed=23)
    x0 = torch.zeros(256, 2, 16, 16, dtype=torch.float64, device='cuda')
    res = {}
    for name, w in (('biased', 0.0025), ('plain', 0.0)):
        f, h, pot = run_meta(par, x=x0, potential=MetaPotential(81, 4.0, 50.0), n_build=300, w=w)
        h = h[0]
        q = np.rint(np.stack([H(t) for t in h['q'][300:]]))
        vb = np.stack([H(t) for t in h['vbias'][300:]])
        q2, err = reweighted_mean(q ** 2, vb, n_block=256)
        tab = pot.numpy()
        res[name] = {'q2': q2, 'err': err, 'z': (q2 - Q2_EXACT_L16_B6) / err, 'dq': float(np.mean([H(t).mean() for t in h['dq'][300:]])),
                     'acc': float(np.mean([H(t).mean() for t in h['acc'][300:]])), 'range': float(tab.max() - tab.min())}
        print(name, {k: f'{val:.4f}' for k, val in res[name].items()})
    assert res['plain']['range'] == 0.0 and res['biased']['range'] > 1.0
    assert abs(res['biased']['z']) <= 4.0, res
    assert res['biased']['dq'] > res['plain']['dq'], res
