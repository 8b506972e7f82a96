"""GPU tests of boundary-condition tempering through the flow (ftHMC with a defect on the physical field) against the torch
float64 twin of tests/ft_defect_cases.py.  (Named to be collected behind the other GPU files; nothing depends on the order: the module
sets the library's default variant and small path, and every test that changes them puts them back.)

Cases (ft_defect_cases.CASES): ft_meta_cases.PATHS' shapes -- the one-launch sizes (3, 8, 2), (2, 12, 3), (4, 16, 4); the same sizes with
the small path off (3, 8, 2), (4, 16, 4); tiled (2, 20, 2) ragged, (2, 32, 2), (2, 64, 2); the VALU variant (2, 16, 2); the generic net
[4, 6, 5] / k = 5 / 3 components (2, 8, 2); no layers (2, 8, 0) -- each with the defects none, one, full, wrap, col0 of
defect_cases.defect_of and couplings mixed out of {0, beta / 3, beta}.  Default-init flows times 1 and times 3, beta 2 and 6, nstep 1
and 3, the three integrators, field amplitudes pi and 0.3.

Bounds: tests/test_z_ft_meta_gpu.py's for the flowed force, action and trajectories (stated at each check); Dsum takes that file's Q_m
bounds times 2 pi, rounded up: 1e-11 from the action call, 1e-8 behind a trajectory.  Accept flags are compared on every chain: the
twin leaves none out on these inputs (tests/test_ft_defect.py)."""
import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401

import defect_cases as DC
import ft_defect_cases as FD
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
    path, B, L, nl, amp, beta, nstep, integ, dk, sc = c
    x, v, u, g, df, flow = FD.inputs(c)
    w = ops.pack_weights(flow, device='cuda') if nl else None
    return D(x), D(v), D(u), w, D(g), df


def run(c, g=None, defect=None, **kw):
    path, B, L, nl, amp, beta, nstep, integ, dk, sc = c
    x, v, u, w, gd, df = dev(c)
    with setting(path):
        return ops.ft_defect_trajectory(x, v, u, w, nl, beta, gd if g is None else g, df if defect is None else defect, FD.DT, nstep,
                                        integrator=integ, **kw)


KEYS = ('x_new', 'dH', 'acc', 'H0', 'H1', 'plaq', 'Q')
ALL = KEYS + ('dsum', 'state')
DEFECTED = [c for c in FD.CASES if c[8] != 'none']


# ---------------------------------------------------------------- g = beta, or an empty defect: the periodic trajectory, bit for bit
@pytest.mark.parametrize('c', FD.CASES, ids=FD.case_id)
def test_g_equal_to_beta_and_an_empty_defect_give_the_bits_of_ft_trajectory(c):
    """every output and state rows 0 .. 2 are ops.ft_trajectory's on the same path, the one-launch leapfrog included: with g = beta on
    every chain whatever the defect, and with Ld = 0 whatever g"""
    path, B, L, nl, amp, beta, nstep, integ, dk, sc = c
    x, v, u, w, g, df = dev(c)
    with setting(path):
        p = ops.ft_trajectory(x, v, u, w, nl, beta, FD.DT, nstep, integrator=integ)
        r = ops.ft_defect_trajectory(x, v, u, w, nl, beta, torch.full_like(g, beta), df, FD.DT, nstep, integrator=integ)
        e = ops.ft_defect_trajectory(x, v, u, w, nl, beta, g, (df[0], df[1], 0), FD.DT, nstep, integrator=integ)
    for k in KEYS:
        assert bits(r[k], p[k]) and bits(e[k], p[k]), k
    assert bits(r['state'][:3], p['state']) and bits(e['state'][:3], p['state']) and not H(e['dsum']).any()


# ---------------------------------------------------------------- force and action against the twin and against each other
WORST = {}


def worst(key, val):
    WORST[key] = max(WORST.get(key, 0.0), float(val))


@pytest.mark.parametrize('c', FD.CASES, ids=FD.case_id)
def test_force_and_action_against_the_twin(c):
    path, B, L, nl, amp, beta, nstep, integ, dk, sc = c
    x, v, u, w, g, df = dev(c)
    xt, _, _, gt, _, flow = FD.inputs(c)
    gt = torch.from_numpy(gt)
    with setting(path):
        F = ops.ft_defect_force(x, w, nl, beta, g, df)
        S, ld, cs, ds, Q = ops.ft_defect_action(x, w, nl, beta, g, df)
    Ft = FD.force(xt, flow, beta, gt, df)
    with torch.no_grad():
        St, ldt, ct, dt_, Qt = FD.action(xt, flow, beta, gt, df)
    fmax = max(1.0, float(Ft.abs().max()))
    worst('action dsum', np.abs(H(ds) - H(dt_)).max())
    print('force', np.abs(H(F) - H(Ft)).max() / fmax, 'S', np.abs(H(S) - H(St)).max(), 'dsum', np.abs(H(ds) - H(dt_)).max(), 'worst', WORST)
    np.testing.assert_allclose(H(F), H(Ft), rtol=1e-8, atol=1e-10 * fmax)                # the flowed force
    np.testing.assert_allclose(H(S), H(St), rtol=1e-11)
    np.testing.assert_allclose(H(ld), H(ldt), rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(H(cs), H(ct), rtol=1e-11)
    np.testing.assert_allclose(H(ds), H(dt_), rtol=0, atol=1e-11)
    np.testing.assert_allclose(H(Q), np.rint(H(Qt)), rtol=0, atol=1e-6)


@pytest.mark.parametrize('c', [c for c in DEFECTED if c[8] in ('wrap', 'full')], ids=FD.case_id)
def test_force_is_the_gradient_of_the_devices_own_action(c):
    """central differences of ft_defect_action at 8 links per chain, two of them the defect's own: 1e-6 of the force's scale"""
    path, B, L, nl, amp, beta, nstep, integ, dk, sc = c
    x, v, u, w, g, df = dev(c)
    h = 1e-5
    rng = np.random.default_rng(3)
    sites = [(0, df[0], df[1]), (1, df[0], df[1])] + [tuple(rng.integers(0, n) for n in (2, L, L)) for _ in range(6)]
    with setting(path):
        F = H(ops.ft_defect_force(x, w, nl, beta, g, df))
        xs = x.repeat(16, 1, 1, 1).reshape(16, B, 2, L, L)                              # every chain moves the same link: one call per sign
        for k, (mu, i, j) in enumerate(sites):
            xs[2 * k, :, mu, i, j] += h
            xs[2 * k + 1, :, mu, i, j] -= h
        S = H(ops.ft_defect_action(xs.reshape(16 * B, 2, L, L), w, nl, beta, g.repeat(16), df)[0]).reshape(16, B)
    fd = np.stack([(S[2 * k] - S[2 * k + 1]) / (2 * h) for k in range(8)])
    an = np.stack([F[:, mu, i, j] for mu, i, j in sites])
    scale = max(1.0, np.abs(F).max())
    print('fd', np.abs(fd - an).max() / scale)
    assert np.abs(fd - an).max() <= 1e-6 * scale


# ---------------------------------------------------------------- whole trajectories per chain against the twin
@pytest.mark.parametrize('c', FD.CASES, ids=FD.case_id)
def test_trajectory_against_the_twin(c):
    path, B, L, nl, amp, beta, nstep, integ, dk, sc = c
    ref = FD.case(c)[6]
    assert not ref['left_out'].any()
    r = run(c)
    worst('trajectory dsum', np.abs(H(r['dsum']) - ref['dsum']).max())
    for k in ('dH', 'H0', 'H1', 'plaq', 'Q', 'dsum'):
        print(k, np.abs(H(r[k]) - ref[k]).max())
    print('worst', WORST)
    assert np.array_equal(H(r['acc']) > 0.5, ref['acc'])                                 # every chain
    angle_close(r['x_new'], ref['x_new'], 1e-6)
    np.testing.assert_allclose(H(r['dH']), ref['dH'], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(H(r['H0']), ref['H0'], rtol=1e-10)
    np.testing.assert_allclose(H(r['H1']), ref['H1'], rtol=1e-7)
    np.testing.assert_allclose(H(r['plaq']), ref['plaq'], rtol=1e-6)
    np.testing.assert_allclose(H(r['Q']), ref['Q'], rtol=0, atol=1e-6)
    np.testing.assert_allclose(H(r['dsum']), ref['dsum'], rtol=0, atol=1e-8)
    st = H(r['state'])
    assert bits(st[1], r['plaq']) and bits(st[2], r['Q']) and bits(st[3], r['dsum'])


def test_no_layers_gives_the_bits_of_the_plain_trajectory_with_a_defect():
    """n_layers = 0: ops.defect_trajectory's sequenced path, bit for bit"""
    for c in [c for c in FD.CASES if c[0] == 'nolayers']:
        path, B, L, nl, amp, beta, nstep, integ, dk, sc = c
        x, v, u, w, g, df = dev(c)
        r = run(c)
        p = ops.defect_trajectory(x, v, u, beta, g, df, FD.DT, nstep, integrator=integ, path=2)
        for k in ('x_new', 'dH', 'acc', 'H0', 'H1', 'dsum'):
            assert bits(r[k], p[k]), (k, FD.case_id(c))
        # Q here is ft_trajectory's, the sum of the wrapped plaquettes over 2 pi as it comes; the plain call hands out the integer
        assert np.array_equal(np.rint(H(r['Q'])), H(p['Q'])) and np.abs(H(r['Q']) - H(p['Q'])).max() <= 1e-12
        np.testing.assert_allclose(H(r['plaq']) * (L * L), H(p['csum']), rtol=1e-14)       # plaq is the mean, csum the sum: one rounding apart


# ---------------------------------------------------------------- bit for bit
# one case per path with a defect that wraps and one with the full row
ONE_OF_EACH = [next(c for c in FD.CASES if c[0] == p and c[8] == dk) for p, _ in FD.PATHS for dk in ('wrap', 'full')]


@pytest.mark.parametrize('c', ONE_OF_EACH, ids=FD.case_id)
def test_two_calls_chained_and_couplings_exchanged_between_are_bit_for_bit(c):
    path, B, L, nl, amp, beta, nstep, integ, dk, sc = c
    x, v, u, w, g, df = dev(c)
    a, b = run(c), run(c)
    assert all(bits(a[k], b[k]) for k in ALL)
    # the second trajectory of a chain of two: chained = stateless, under the same couplings and with g of chains 0 and 1 exchanged between
    v2, u2 = D(MC.draws(B, L, 4242)[0]), D(MC.draws(B, L, 4242)[1])
    for swapped in (False, True):
        g2 = g.clone()
        if swapped:
            g2[0], g2[1] = g[1], g[0]
            assert not bits(g2, g)
        with setting(path):
            args = (a['x_new'], v2, u2, w, nl, beta, g2, df, FD.DT, nstep)
            s = ops.ft_defect_trajectory(*args, integrator=integ)
            ch = ops.ft_defect_trajectory(*args, integrator=integ, state_in=a['state'])
        assert all(bits(s[k], ch[k]) for k in ALL), swapped


@pytest.mark.parametrize('c', ONE_OF_EACH, ids=FD.case_id)
def test_a_chain_of_a_batch_is_the_chain_alone_and_null_outputs_change_nothing(c):
    from fthmc_amd import _lib
    path, B, L, nl, amp, beta, nstep, integ, dk, sc = c
    x, v, u, w, g, df = dev(c)
    r = run(c)
    with setting(path):
        for b in range(B):
            o = ops.ft_defect_trajectory(x[b:b + 1], v[b:b + 1], u[b:b + 1], w, nl, beta, g[b:b + 1].clone(), df, FD.DT, nstep, integrator=integ)
            assert all(bits(H(r[k])[b:b + 1] if k != 'state' else H(r[k])[:, b:b + 1], o[k]) for k in ALL), b
        # every optional output null: the same x_new
        xn = torch.empty_like(x)
        ws, nb = ops._ws(x, B, L, nl, arch=ops.arch_of(w) if nl else None, defect=True)
        rc = _lib.load().fthmc_ft_defect_trajectory_v(ops._p(x), ops._p(v), ops._p(u), ops._p(w), ops._arch(ops.arch_of(w)) if nl else None, nl, B, L,
                                                      ops.act_code('silu'), beta, ops._p(g), *df, FD.DT, nstep, _lib.INTEGRATORS[integ], ops._p(xn),
                                                      None, None, None, None, None, None, None, None, None, ws, nb, ops._stream(x), 0)
    assert rc == 0 and bits(xn, r['x_new'])


@pytest.mark.parametrize('c', [c for c in ONE_OF_EACH if c[1] % 2 == 0], ids=FD.case_id)
def test_groups_do_not_change_a_bit(c):
    r, g = run(c), run(c, groups=2)
    assert all(bits(r[k], g[k]) for k in ALL)


def test_what_the_wrapper_refuses():
    c = ONE_OF_EACH[0]
    path, B, L, nl, amp, beta, nstep, integ, dk, sc = c
    x, v, u, w, g, df = dev(c)
    for bad in ((0, L, 1), (0, 0, L + 1), (-1, 0, 1), (0, 0)):
        with pytest.raises(ValueError):
            ops.ft_defect_trajectory(x, v, u, w, nl, beta, g, bad, 0.1, 1)
    with pytest.raises(ValueError):
        ops.ft_defect_trajectory(x, v, u, w, nl, beta, g, df, 0.1, 0)
    with pytest.raises(ValueError):
        ops.ft_defect_trajectory(x, v, u, w, nl, g, g, df, 0.1, 1)                         # ONE beta per call
    with pytest.raises(ops.FthmcError):
        ops.ft_defect_trajectory(x, v, u, w, nl, beta, g[:B - 1], df, 0.1, 1)
    assert ops.ft_defect_ws_bytes(B, L, nl) > ops.ws_bytes(B, L, nl)


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


def _series(h):
    return {k: np.asarray(h[k]) for k in ('plaq', 'Q', 'acc', 'dH', 'dsum', 'swap_rounds', 'rung', 'round_trips')}


@pytest.mark.parametrize('L', [8, 20])
def test_run_ft_ptbc_captured_equals_eager_and_two_hand_sequenced_iterations(L):
    from fthmc_amd.defect import run_ft_ptbc, shift_seed
    from fthmc_amd.tempering import swap_seed
    K, M, ntraj, nl = 4, 2, 8, 2
    par = _param(beta=3.0, L=L, tau=0.6, nstep=3, seed=5)
    cs = [0.0, 0.4, 0.75, 1.0]
    df = (L - 2, L - 1, 4)
    flow, wts = module_flow(nl, L)
    x0 = D(MC.links(K * M, L, 79, 1.0))
    ha, hb = (run_ft_ptbc(par, flow, cs, M, ntraj, defect=df, integrator='omelyan', x=x0, captured=cap) for cap in (True, False))
    a, b = _series(ha), _series(hb)
    for k in a:
        assert a[k].shape == b[k].shape and bits(a[k].astype(np.float64), b[k].astype(np.float64)), k
    assert bits(ha['x'], hb['x']) and bits(ha['g_b'], hb['g_b']) and bits(ha['rung_last'], hb['rung_last'])
    assert a['plaq'].shape == (ntraj, K, M) and a['rung'].shape == (ntraj, K * M) and ha['swap_acc'].shape == (K - 1,)
    assert list(ha['cs']) == cs and tuple(ha['defect']) == df and (a['swap_rounds'] >= 0).any()
    assert (np.sort(a['rung'].reshape(ntraj, M, K), axis=2) == np.arange(K)).all()
    assert np.array_equal(H(ha['g_b']), par.beta * np.array(cs)[H(ha['rung_last'])])
    # two hand-sequenced iterations: the first history rows, bit for bit; the shifts are multiples of 4
    B = K * M
    w = ops.pack_weights(wts, device='cuda')
    lad = ops.ladder_init([par.beta * c for c in cs], M, device='cuda')
    g_b, rung, chain_of = lad['beta_b'], lad['rung'], lad['chain_of']
    x = x0.clone()
    for t in range(2):
        seeds = ops.chain_seeds(par.seed, 0, B, t, device='cuda')
        v, u = ops.random_momenta(seeds, x.shape)
        r = ops.ft_defect_trajectory(x, v, u, w, nl, par.beta, g_b, df, par.tau / par.nstep, par.nstep, integrator='omelyan')
        rg = H(rung).astype(np.int64)
        order = (np.argsort(rg.reshape(M, K), axis=1) + (np.arange(M) * K)[:, None]).T      # [K, M] -> chain index
        assert np.array_equal(a['rung'][t], rg)
        for k in ('plaq', 'dsum', 'Q', 'dH', 'acc'):
            assert bits(a[k][t], H(r[k])[order]), (k, t)
        us = ops.random_uniform(ops.chain_seeds(swap_seed(par.seed), 0, M, t, device='cuda'), (M, K - 1), 0.0, 1.0)
        sw = ops.replica_swap(lad['betas'], r['dsum'], us, g_b, rung, chain_of, t % 2)
        assert bits(a['swap_rounds'][t], sw['swap_acc'])
        ush = ops.random_uniform(ops.chain_seeds(shift_seed(par.seed), 0, B, t, device='cuda'), (B, 2), 0.0, 1.0)
        shift = (torch.floor(ush * float(L // 4)) * 4.0).to(torch.int32)
        sh = H(shift)
        assert (sh % 4 == 0).all() and sh.min() >= 0 and sh.max() <= L - 4
        x = ops.defect_translate(r['x_new'], rung, K - 1, shift)
    # the recorded observables are those of the physical field of the latent field the run returns (translate=False: nothing moved it since)
    hn = run_ft_ptbc(par, flow, cs, M, 3, defect=df, integrator='omelyan', x=x0, translate=False)
    y = ops.flow_forward(hn['x'], w, nl)[0]
    _, cs_, ds_, Q_ = ops.defect_action(y, par.beta, hn['g_b'], df)
    n = _series(hn)
    rl = n['rung'][-1].astype(np.int64)                                                  # the rungs the last trajectory ran on: what its row is sorted by
    order = (np.argsort(rl.reshape(M, K), axis=1) + (np.arange(M) * K)[:, None]).T
    np.testing.assert_allclose(n['dsum'][-1], H(ds_)[order], rtol=0, atol=1e-9)
    np.testing.assert_allclose(n['plaq'][-1], H(cs_)[order] / (L * L), rtol=1e-9)
    np.testing.assert_allclose(n['Q'][-1], H(Q_)[order], rtol=0, atol=1e-9)
    # translate=False carries the g-free state from trajectory to trajectory: the same bits as trajectories that evaluate their own start
    lad = ops.ladder_init([par.beta * c for c in cs], M, device='cuda')
    g_b, rung, chain_of = lad['beta_b'], lad['rung'], lad['chain_of']
    x = x0.clone()
    for t in range(3):
        v, u = ops.random_momenta(ops.chain_seeds(par.seed, 0, B, t, device='cuda'), x.shape)
        r = ops.ft_defect_trajectory(x, v, u, w, nl, par.beta, g_b, df, par.tau / par.nstep, par.nstep, integrator='omelyan')   # stateless
        order = (np.argsort(H(rung).astype(np.int64).reshape(M, K), axis=1) + (np.arange(M) * K)[:, None]).T
        for k in ('plaq', 'dsum', 'Q', 'dH', 'acc'):
            assert bits(n[k][t], H(r[k])[order]), (k, t)
        us = ops.random_uniform(ops.chain_seeds(swap_seed(par.seed), 0, M, t, device='cuda'), (M, K - 1), 0.0, 1.0)
        ops.replica_swap(lad['betas'], r['dsum'], us, g_b, rung, chain_of, t % 2)
        x = r['x_new']
    # the driver refuses what it documents
    for bad in ([0.0, 0.5], [0.5, 0.4, 1.0], [-0.1, 1.0], [1.0]):
        with pytest.raises(ValueError):
            run_ft_ptbc(par, flow, bad, M, 2)
    with pytest.raises(ValueError):
        run_ft_ptbc(par, flow, cs, M, 2, defect=(0, 0, L + 1))
    with pytest.raises(ValueError):
        run_ft_ptbc(par, None, cs, M, 2)
    with pytest.raises(ValueError):
        run_ft_ptbc(par, flow, cs, M, 2, integrator='euler')


# ---------------------------------------------------------------- physics: what the feature is for
def _jackknife(per_ladder):
    M = len(per_ladder)
    jk = (per_ladder.sum() - per_ladder) / (M - 1)
    return float(per_ladder.mean()), float(np.sqrt((M - 1) * np.mean((jk - jk.mean()) ** 2)))


def _dq_following_the_chains(h, K):
    """mean |dQ| per trajectory of a chain, Q of the SAME chain at t and t + 1 (history['rung'] says on which rung every chain ran, the
    series themselves are sorted by rung): a swap exchanges two chains' places and does not count as tunnelling"""
    Q, rg = np.rint(np.asarray(h['Q'])), np.asarray(h['rung'])                           # [n, K, M] by rung, [n, B] by chain
    n, _, M = Q.shape
    ladder = np.arange(M * K) // K
    qc = Q[np.arange(n)[:, None], rg, ladder[None, :]]                                  # [n, B]: Q of every chain
    return float(np.abs(np.diff(qc, axis=0)).mean())


def test_ft_ptbc_unfreezes_the_charge_and_samples_the_periodic_rung():
    """L = 16, beta = 6, 32 ladders of K = 8 rungs linear in c (256 chains), a defect of 4 plaquettes, a 2-layer default-init flow, 600
    leapfrog trajectories (tau = 1, 10 steps) from a cold start, the first 100 left out: tests/test_z_defect_gpu.py's setting with
    tests/test_z_ft_meta_gpu.py's flow.  <Q^2> of the physical field on rung K - 1 within |z| <= 4 of the exact 1.1947014482 (jackknife
    over the ladders), every rung's defect <cos P> within |z| <= 4 of exact_defect_plaquette, and more |dQ| per trajectory, following
    each chain through the ladder, than tempered ftHMC over a ladder of beta that is as flat as a ladder may be."""
    from fthmc_amd.defect import run_ft_ptbc
    from fthmc_amd.tempering import run_tempered
    from fthmc_amd.utils.observables import exact_defect_plaquette
    M, K, ntraj, therm, Ld = 32, 8, 600, 100, 4
    cs = [k / (K - 1) for k in range(K - 1)] + [1.0]
    par = _param(beta=6.0, L=16, tau=1.0, nstep=10, seed=29)
    flow, _ = module_flow(2, 16)
    h = run_ft_ptbc(par, flow, cs, M, ntraj, defect=(0, 0, Ld))
    Q = np.rint(np.asarray(h['Q'])[:, K - 1, :])                                         # [ntraj, M]
    q2, err = _jackknife((Q[therm:] ** 2).mean(axis=0))
    z = (q2 - Q2_EXACT_L16_B6) / err
    dq = _dq_following_the_chains(h, K)
    ht = run_tempered(par, flow, [6.0 - 1e-6 * (K - 1 - k) for k in range(K)], M, ntraj)
    dqt = _dq_following_the_chains(ht, K)
    print(f'<Q^2> {q2:.4f} +- {err:.4f}, exact {Q2_EXACT_L16_B6:.4f}, z {z:+.2f}; |dQ| per trajectory following the chains {dq:.4f} against '
          f'{dqt:.4f} tempered flat; acceptance {float(np.asarray(h["acc"]).mean()):.3f}, swaps {np.round(h["swap_acc"], 3)}, '
          f'round trips {int(h["round_trips"].sum())}')
    assert abs(z) <= 4.0
    assert dq > dqt
    dp = np.asarray(h['dsum'])[therm:] / Ld                                              # [n, K, M]
    for k in range(K):
        m, e = _jackknife(dp[:, k, :].mean(axis=0))
        ex = exact_defect_plaquette(6.0, 16, cs[k], Ld)
        print(f'rung {k} c {cs[k]:.3f}: defect <cos P> {m:.4f} +- {e:.4f}, exact {ex:.4f}, z {(m - ex) / e:+.2f}')
        assert abs(m - ex) <= 4.0 * e, k
