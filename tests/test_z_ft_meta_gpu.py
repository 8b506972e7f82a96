"""GPU tests of metadynamics ftHMC (the bias in the charge through the flow) against the torch float64 twin of
tests/ft_meta_cases.py.  (Named to be collected behind the other GPU files; nothing depends on the order: the module sets the
library's default variant and small path, and every test that changes them puts them back.)

Cases (ft_meta_cases.CASES): one launch (3, 8, 2), (2, 12, 3), (4, 16, 4); the same sizes with the small path off (3, 8, 2),
(4, 16, 4); tiled (2, 20, 2) ragged, (2, 32, 2), (2, 64, 2); the VALU variant (2, 16, 2); the generic net [4, 6, 5] / k = 5 / 3
components (2, 8, 2); no layers (2, 8, 0).  Default-init flows times 1 and times 3, beta 2 and 6, nstep 1 and 3, the three
integrators, the zero / quadratic / rough tables of meta_cases.table, field amplitudes pi and 0.3, G in {1, B}.

Bounds: the figures tests/test_hip_parity.py holds the unbiased flowed force, action and trajectories to (stated at each check).
Accept flags are compared on every chain: the twin leaves none out on these inputs (tests/test_ft_meta.py)."""
import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401

import ft_meta_cases as FC
import meta_cases as MC

from gpu_support import D, H, angle_close, module_defaults, ops, switches

pytestmark = pytest.mark.gpu
_defaults = module_defaults()

Q2_EXACT_L16_B6 = 1.1947014482


def bits(a, b):
    a, b = np.ascontiguousarray(H(a)), np.ascontiguousarray(H(b))
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def setting(path):
    """the library's switches for a path of the case table: 'off' the small path off, 'valu' the VALU variant"""
    return switches(variant=0 if path == 'valu' else 1, small=path != 'off')


def dev(c):
    path, B, L, nl, amp, beta, nstep, integ, tk, G, sc = c
    x, v, u, tab, flow = FC.inputs(c)
    w = ops.pack_weights(flow, device='cuda') if nl else None
    return D(x), D(v), D(u), w, D(tab.V), tab


def run(c, table=None, path=None, **kw):
    p, B, L, nl, amp, beta, nstep, integ, tk, G, sc = c
    x, v, u, w, V, tab = dev(c)
    with setting(path or p):
        return ops.ft_meta_trajectory(x, v, u, w, nl, beta, FC.DT, nstep, V if table is None else table, tab.qmax, tab.wall,
                                      integrator=integ, **kw)


ZERO = [c for c in FC.CASES if c[8] == 'zero']
BIASED = [c for c in FC.CASES if c[8] != 'zero']
KEYS = ('x_new', 'dH', 'acc', 'H0', 'H1', 'plaq', 'Q')


# ---------------------------------------------------------------- zero table: the unbiased trajectory, bit for bit
@pytest.mark.parametrize('c', ZERO, ids=FC.case_id)
def test_zero_table_gives_the_bits_of_ft_trajectory(c):
    path, B, L, nl, amp, beta, nstep, integ, tk, G, sc = c
    x, v, u, w, V, tab = dev(c)
    assert tab.wall == 0.0 and not tab.V.any()
    with setting(path):
        r = ops.ft_meta_trajectory(x, v, u, w, nl, beta, FC.DT, nstep, V, tab.qmax, tab.wall, integrator=integ)
        p = ops.ft_trajectory(x, v, u, w, nl, beta, FC.DT, nstep, integrator=integ)
    for k in KEYS:
        assert bits(r[k], p[k]), k
    assert bits(r['state'][:3], p['state']) and not H(r['vbias']).any()


# ---------------------------------------------------------------- force and action against the twin and against each other
@pytest.mark.parametrize('c', BIASED, ids=FC.case_id)
def test_force_and_action_against_the_twin(c):
    path, B, L, nl, amp, beta, nstep, integ, tk, G, sc = c
    x, v, u, w, V, tab = dev(c)
    xt, _, _, _, flow = FC.inputs(c)
    with setting(path):
        F = ops.ft_meta_force(x, w, nl, beta, V, tab.qmax, tab.wall)
        S, ld, qm, vb = ops.ft_meta_action(x, w, nl, beta, V, tab.qmax, tab.wall)
    Ft, margin = FC.force(xt, flow, beta, tab)
    with torch.no_grad():
        St, ldt, qmt, vbt, m2 = FC.biased_action(xt, flow, beta, tab)
    assert min(margin.min(), m2.min()) >= FC.T_MARGIN
    fmax = max(1.0, float(Ft.abs().max()))
    print('force', np.abs(H(F) - H(Ft)).max() / fmax, 'S_b', np.abs(H(S) - H(St)).max(), 'qm', np.abs(H(qm) - H(qmt)).max())
    np.testing.assert_allclose(H(F), H(Ft), rtol=1e-8, atol=1e-10 * fmax)                # test_hip_parity.py: the flowed force
    np.testing.assert_allclose(H(S), H(St), rtol=1e-11, atol=1e-11 * max(1.0, float(vbt.abs().max())))
    np.testing.assert_allclose(H(qm), H(qmt), rtol=0, atol=1e-12)
    np.testing.assert_allclose(H(vb), H(vbt), rtol=1e-11, atol=1e-11 * max(1.0, float(vbt.abs().max())))
    np.testing.assert_allclose(H(ld), H(ldt), rtol=1e-11, atol=1e-11)


@pytest.mark.parametrize('c', [c for c in BIASED if c[8] == 'quad'], ids=FC.case_id)
def test_force_is_the_gradient_of_the_devices_own_action(c):
    """central differences of ft_meta_action at 8 links per chain on the smooth table: relative 1e-6"""
    path, B, L, nl, amp, beta, nstep, integ, tk, G, sc = c
    x, v, u, w, V, tab = dev(c)
    h = 1e-5
    rng = np.random.default_rng(3)
    sites = [tuple(rng.integers(0, n) for n in (2, L, L)) for _ in range(8)]
    with setting(path):
        F = H(ops.ft_meta_force(x, w, nl, beta, V, tab.qmax, tab.wall))
        xs = x.repeat(16, 1, 1, 1).reshape(16, B, 2, L, L)                              # every chain moves the same link: one call per sign
        for k, (mu, i, j) in enumerate(sites):
            xs[2 * k, :, mu, i, j] += h
            xs[2 * k + 1, :, mu, i, j] -= h
        Vrep = V if G == 1 else V.repeat(16, 1)
        S = H(ops.ft_meta_action(xs.reshape(16 * B, 2, L, L), w, nl, beta, Vrep, tab.qmax, tab.wall)[0]).reshape(16, B)
    fd = np.stack([(S[2 * k] - S[2 * k + 1]) / (2 * h) for k in range(8)])
    an = np.stack([F[:, mu, i, j] for mu, i, j in sites])
    scale = max(1.0, np.abs(F).max())
    print('fd', np.abs(fd - an).max() / scale)
    assert np.abs(fd - an).max() <= 1e-6 * scale


# ---------------------------------------------------------------- whole biased trajectories per chain against the twin
@pytest.mark.parametrize('c', BIASED, ids=FC.case_id)
def test_biased_trajectory_against_the_twin(c):
    path, B, L, nl, amp, beta, nstep, integ, tk, G, sc = c
    ref = FC.case(c)[5]
    tab = FC.inputs(c)[3]
    assert not ref['left_out'].any()
    r = run(c)
    for k in ('dH', 'H0', 'H1', 'plaq', 'Q', 'qm', 'vbias'):
        print(k, np.abs(H(r[k]) - ref[k]).max())
    assert np.array_equal(H(r['acc']) > 0.5, ref['acc'])
    angle_close(r['x_new'], ref['x_new'], 1e-6)                                         # test_hip_parity.py's flowed trajectories
    np.testing.assert_allclose(H(r['dH']), ref['dH'], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(H(r['H0']), ref['H0'], rtol=1e-10)
    np.testing.assert_allclose(H(r['H1']), ref['H1'], rtol=1e-7)
    np.testing.assert_allclose(H(r['plaq']), ref['plaq'], rtol=1e-6)
    np.testing.assert_allclose(H(r['Q']), ref['Q'], rtol=0, atol=1e-6)
    slope = max(1.0, float(np.abs(np.diff(tab.V, axis=1)).max() / ((2 * tab.qmax) / (tab.nb - 1))), tab.wall)
    np.testing.assert_allclose(H(r['qm']), ref['qm'], rtol=0, atol=1e-9)
    np.testing.assert_allclose(H(r['vbias']), ref['vbias'], rtol=0, atol=1e-9 * slope)
    st = H(r['state'])
    assert bits(st[1], r['plaq']) and bits(st[2], r['Q']) and bits(st[3], r['qm'])


def test_no_layers_is_meta_trajectory():
    """n_layers = 0: the accepts of ops.meta_trajectory's sequenced path and its fields (DESIGN 4.15's bounds: x_new 1e-9, dH 1e-8 / 1e-9)"""
    for c in [c for c in BIASED if c[0] == 'nolayers']:
        path, B, L, nl, amp, beta, nstep, integ, tk, G, sc = c
        x, v, u, w, V, tab = dev(c)
        r = run(c)
        p = ops.meta_trajectory(x, v, u, beta, FC.DT, nstep, V, tab.qmax, tab.wall, integrator=integ, path=2)
        assert np.array_equal(H(r['acc']), H(p['acc']))
        angle_close(r['x_new'], p['x_new'], 1e-9)
        np.testing.assert_allclose(H(r['dH']), H(p['dH']), rtol=1e-8, atol=1e-9)
        np.testing.assert_allclose(H(r['qm']), H(p['qm']), rtol=0, atol=1e-12)


# ---------------------------------------------------------------- bit for bit
# one rough-table case per path and row layout (G = 1, G = B)
ONE_OF_EACH = [next(c for c in BIASED if c[0] == p and c[8] == 'rough' and (c[9] == 1) == shared) for p, _ in FC.PATHS for shared in (True, False)]
ALL = KEYS + ('qm', 'vbias', 'state')


@pytest.mark.parametrize('c', ONE_OF_EACH, ids=FC.case_id)
def test_two_calls_chained_and_a_deposit_between_are_bit_for_bit(c):
    path, B, L, nl, amp, beta, nstep, integ, tk, G, sc = c
    x, v, u, w, V, tab = dev(c)
    a, b = run(c), run(c)
    assert all(bits(a[k], b[k]) for k in ALL)
    # the second trajectory of a chain of two: chained = stateless, under the same table and under one that gained hills between
    v2, u2 = D(MC.draws(B, L, 4242)[0]), D(MC.draws(B, L, 4242)[1])
    for deposit in (False, True):
        V2 = V.clone()
        if deposit:
            # hills at the walkers' charges, and where a walker sits on the wall (a deposit there adds nothing) in the table's last
            # interval on its side, which moves the edge value its wall stands on
            ops.meta_deposit(a['qm'], V2, tab.qmax, 0.37)
            ops.meta_deposit(torch.clamp(a['qm'], -0.999 * tab.qmax, 0.999 * tab.qmax), V2, tab.qmax, 0.21)
            assert not bits(V2, V)
        with setting(path):
            args = (a['x_new'], v2, u2, w, nl, beta, FC.DT, nstep, V2, tab.qmax, tab.wall)
            s = ops.ft_meta_trajectory(*args, integrator=integ)
            ch = ops.ft_meta_trajectory(*args, integrator=integ, state_in=a['state'])
        assert all(bits(s[k], ch[k]) for k in ALL), deposit


@pytest.mark.parametrize('c', [c for c in ONE_OF_EACH if c[9] == c[1]], ids=FC.case_id)
def test_a_chain_of_a_batch_is_the_chain_alone_with_its_row(c):
    path, B, L, nl, amp, beta, nstep, integ, tk, G, sc = c
    x, v, u, w, V, tab = dev(c)
    r = run(c)
    for b in range(B):
        with setting(path):
            o = ops.ft_meta_trajectory(x[b:b + 1], v[b:b + 1], u[b:b + 1], w, nl, beta, FC.DT, nstep, V[b:b + 1], tab.qmax, tab.wall,
                                       integrator=integ)
        assert all(bits(H(r[k])[b:b + 1] if k != 'state' else H(r[k])[:, b:b + 1], o[k]) for k in ALL), b


@pytest.mark.parametrize('c', [c for c in ONE_OF_EACH if c[1] % 2 == 0], ids=FC.case_id)
def test_groups_do_not_change_a_bit(c):
    r, g = run(c), run(c, groups=2)
    assert all(bits(r[k], g[k]) for k in ALL)


def test_groups_that_split_a_row_raise():
    c = next(c for c in BIASED if c[0] == 'one' and c[1] == 4 and c[9] == 4)
    x, v, u, w, V, tab = dev(c)
    V2 = V[:2].contiguous()                                                              # two rows of two chains
    with pytest.raises(ValueError):
        run(c, table=V2, groups=[1, 3])
    with pytest.raises(ValueError):
        run(c, table=V2, groups=4)
    assert all(bits(run(c, table=V2)[k], run(c, table=V2, groups=2)[k]) for k in ALL)


@pytest.mark.parametrize('c', [c for c in BIASED if c[0] == 'one'], ids=FC.case_id)
def test_one_launch_against_the_small_path_off(c):
    """the same accepts, and fields within the sum of the two paths' bounds against the twin"""
    a, b = run(c), run(c, path='off')
    assert np.array_equal(H(a['acc']), H(b['acc']))
    angle_close(a['x_new'], b['x_new'], 2e-6)
    np.testing.assert_allclose(H(a['dH']), H(b['dH']), rtol=2e-6, atol=2e-6)
    np.testing.assert_allclose(H(a['H0']), H(b['H0']), rtol=2e-10)
    np.testing.assert_allclose(H(a['qm']), H(b['qm']), rtol=0, atol=2e-9)


# ---------------------------------------------------------------- the driver
def _param(**kw):
    from fthmc_amd.config import Param
    return Param(**kw)


def module_flow(nl, L, seed=31):
    """-> (the flow as FieldTransformation takes it, the same weights as oracle.ref_cpu takes them)"""
    from fthmc_amd.utils import layers as LY
    from oracle import ref_cpu as R
    wts = R.default_flow(nl, torch.Generator().manual_seed(seed))
    flow = LY.make_u1_equiv_layers(n_layers=nl, n_mixture_comps=2, lattice_shape=(L, L), hidden_sizes=[8, 8], kernel_size=3)
    names = ('net.0.weight', 'net.0.bias', 'net.2.weight', 'net.2.bias', 'net.4.weight', 'net.4.bias')
    flow.load_state_dict({f'{li}.plaq_coupling.{n}': wts[li][pi].cuda() for li in range(nl) for pi, n in enumerate(names)})
    return flow.cuda().double(), wts


@pytest.mark.parametrize('L', [8, 20])
def test_run_ft_meta_captured_equals_eager_and_deposits_at_the_recorded_charge(L):
    from fthmc_amd.meta import MetaPotential, run_ft_meta
    flow, _ = module_flow(2, L)
    x0 = D(MC.links(6, L, 77, 1.0))
    out = []
    for use_graph in (True, False):
        pot = MetaPotential(41, 2.0, 10.0, groups=2)
        f, h, p = run_ft_meta(_param(beta=3.0, L=L, tau=0.3, nstep=3, ntraj=7, nrun=2, seed=5), flow, x=x0, potential=pot, n_build=9, w=0.05,
                              integrator='omelyan', use_graph=use_graph)
        out.append((f, h, pot.numpy()))
    (fa, ha, ta), (fb, hb, tb) = out
    assert bits(ta, tb) and ta.any() and all(bits(a, b) for a, b in zip(fa, fb))
    for n in (0, 1):
        assert ha[n]['build'] == hb[n]['build'] == [n * 7 + i < 9 for i in range(7)]
        for k in ('acc', 'dH', 'plaq', 'q', 'dq', 'qm', 'vbias'):
            assert len(ha[n][k]) == 7 and all(bits(a, b) for a, b in zip(ha[n][k], hb[n][k])), k
    tw = MC.Table(np.zeros((2, 41)), 2.0, 10.0)
    for n in (0, 1):
        for i in range(7):
            if ha[n]['build'][i]:
                tw.deposit(H(ha[n]['qm'][i]), 0.05)
    assert bits(ta, tw.V)
    # the recorded observables are those of the physical field of the latent field the run returns
    w = ops.pack_weights(module_flow(2, L)[1], device='cuda')
    y = ops.flow_forward(fa[1], w, 2)[0]
    S, Q, plaq = ops.wilson_action_charge(y, 3.0)
    np.testing.assert_allclose(H(ha[1]['q'][-1]), H(Q), rtol=0, atol=1e-9)
    np.testing.assert_allclose(H(ha[1]['plaq'][-1]), H(plaq), rtol=1e-9)
    np.testing.assert_allclose(H(ha[1]['qm'][-1]), H(ops.meta_action(y, 3.0, D(ta), 2.0, 10.0)[1]), rtol=0, atol=1e-9)


def test_run_ft_meta_without_layers_is_run_meta_and_run_meta_is_unchanged():
    from fthmc_amd.meta import MetaPotential, run_ft_meta, run_meta
    par = _param(beta=3.0, L=8, tau=0.3, nstep=3, ntraj=6, nrun=1, seed=9)
    x0 = D(MC.links(4, 8, 78, 1.0))

    def plain():
        return run_meta(par, x=x0, potential=MetaPotential(41, 2.0, 10.0), n_build=3, w=0.05)
    f0, h0, p0 = plain()                                                                 # before the flowed driver is touched
    f, h, p = run_ft_meta(par, torch.nn.ModuleList(), x=x0, potential=MetaPotential(41, 2.0, 10.0), n_build=3, w=0.05)
    f1, h1, p1 = plain()
    assert bits(f0[0], f1[0]) and bits(p0.numpy(), p1.numpy())
    for k in ('acc', 'dH', 'plaq', 'q', 'dq', 'qm', 'vbias'):
        assert all(bits(a, b) for a, b in zip(h0[0][k], h1[0][k])), k
    # zero layers: the latent field is the physical field; today's run_meta to 4.15's bounds
    for t in range(par.ntraj):
        assert np.array_equal(H(h[0]['acc'][t]), H(h0[0]['acc'][t])), t
        np.testing.assert_allclose(H(h[0]['dH'][t]), H(h0[0]['dH'][t]), rtol=1e-8, atol=1e-9)
        np.testing.assert_allclose(H(h[0]['qm'][t]), H(h0[0]['qm'][t]), rtol=0, atol=1e-9)
    angle_close(f[0], f0[0], 1e-9)
    np.testing.assert_allclose(p.numpy(), p0.numpy(), rtol=0, atol=1e-9)


# ---------------------------------------------------------------- physics: what the feature is for
def test_the_bias_through_the_flow_unfreezes_the_charge_and_reweights_to_the_exact_moment():
    """L = 16, beta = 6, 256 chains cold, a 2-layer default-init flow, one shared table (nb = 81, qmax = 4, wall = 50), w = 0.0025,
    300 build + 400 static leapfrog trajectories (tau = 1, 10 steps): the reweighted <Q^2> of the physical field (jackknife over the
    chains) within |z| <= 4 of the exact 1.1947014482, and more tunnelling per static trajectory than under a zero table."""
    from fthmc_amd.meta import MetaPotential, run_ft_meta
    from fthmc_amd.utils.observables import reweighted_mean
    flow, _ = module_flow(2, 16)
    par = _param(beta=6.0, L=16, tau=1.0, nstep=10, ntraj=700, nrun=1, seed=23)
    x0 = torch.zeros(256, 2, 16, 16, dtype=torch.float64, device='cuda')
    res = {}
    for name, w in (('biased', 0.0025), ('plain', 0.0)):
        f, h, pot = run_ft_meta(par, flow, x=x0, potential=MetaPotential(81, 4.0, 50.0), n_build=300, w=w)
        h = h[0]
        q = np.rint(np.stack([H(t) for t in h['q'][300:]]))
        vb = np.stack([H(t) for t in h['vbias'][300:]])
        q2, err = reweighted_mean(q ** 2, vb, n_block=256)
        tab = pot.numpy()
        res[name] = {'q2': q2, 'err': err, 'z': (q2 - Q2_EXACT_L16_B6) / err, 'dq': float(np.mean([H(t).mean() for t in h['dq'][300:]])),
                     'acc': float(np.mean([H(t).mean() for t in h['acc'][300:]])), 'range': float(tab.max() - tab.min())}
        print(name, {k: f'{val:.4f}' for k, val in res[name].items()})
    assert res['plain']['range'] == 0.0 and res['biased']['range'] > 1.0
    assert res['biased']['acc'] >= 0.2, res
    assert abs(res['biased']['z']) <= 4.0, res
    assert res['biased']['dq'] > res['plain']['dq'], res
