"""GPU tests of replica exchange over a beta ladder: the per-chain-beta trajectory on every kernel path against the scalar entry
points (bit for bit) and against the CPU oracle, the beta-free carried state, k_replica_swap against the numpy round of
tests/tempering_cases.py, the ladder invariants, the captured driver against the eager one, and the exactness of the tempered
sampler at every rung against the finite-volume plaquette.

Inputs: seeded uniform links in +-pi, normal momenta, tau = 0.3; the ladder (1.5, 2, 3) repeated over the chains."""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401

import integrator_cases as IC
import tempering_cases as TC

from gpu_support import D, H, R, module_defaults, ops, switches

pytestmark = pytest.mark.gpu
_defaults = module_defaults()

KEYS = ('x_new', 'dH', 'acc', 'H0', 'H1', 'plaq', 'Q')


def flow_of(seed, nl, arch=None):
    gen = torch.Generator().manual_seed(seed)
    if arch is None:
        return R.default_flow(nl, gen)
    return R.default_flow(nl, gen, hidden=arch[0], k=arch[1], n_mix=arch[2])


def ft_rows():
    rows = []
    for case in TC.FT_PATHS:
        for name, nstep in TC.INTEGRATORS:
            if name == 'leapfrog' or case[0] in TC.ALL_INTEGRATORS_ON:
                rows.append(pytest.param(case, name, nstep, id=f'{case[0]}-{name}'))
    return rows


@functools.lru_cache(maxsize=None)
def ft_inputs(cid, L, B, nl, arch):
    seed = 100 + sum(map(ord, cid))
    x, v, u = IC.draw(seed, B, L)
    return flow_of(seed, nl, arch), x, v, u


def scalar_ft(case, name, nstep, beta):
    """the scalar entry point's result on the case's batch at one beta (computed once per (case, integrator, beta))"""
    return _scalar_ft(case, name, nstep, float(beta))


@functools.lru_cache(maxsize=None)
def _scalar_ft(case, name, nstep, beta):
    cid, L, B, nl, arch, variant, small = case
    flow, x, v, u = ft_inputs(cid, L, B, nl, arch)
    with switches(variant=variant, small=small):
        w = ops.pack_weights(flow, device='cuda') if nl else None
        r = ops.ft_trajectory(x.cuda(), v.cuda(), u.cuda(), w, nl, beta, TC.TAU / nstep, nstep, mode='md', integrator=name)
        torch.cuda.synchronize()
    return {k: t.clone() for k, t in r.items()}


def pb_ft(case, name, nstep, beta_b, state_in=None):
    cid, L, B, nl, arch, variant, small = case
    flow, x, v, u = ft_inputs(cid, L, B, nl, arch)
    with switches(variant=variant, small=small):
        w = ops.pack_weights(flow, device='cuda') if nl else None
        r = ops.ft_trajectory(x.cuda(), v.cuda(), u.cuda(), w, nl, D(beta_b), TC.TAU / nstep, nstep, mode='md', integrator=name,
                              state_in=state_in)
        torch.cuda.synchronize()
    return r


# ---------------------------------------------------------------- A: a constant beta_b is the scalar call
@pytest.mark.parametrize('case,name,nstep', ft_rows())
def test_constant_beta_b_equals_the_scalar_call(case, name, nstep):
    B, L, beta = case[2], case[1], 2.3                             # not a power of two: (-beta) C is rounded
    ref = scalar_ft(case, name, nstep, beta)
    r = pb_ft(case, name, nstep, np.full(B, beta))
    for k in KEYS:
        assert torch.equal(r[k], ref[k]), k
    assert TC.state_matches(H(r['state']), np.full(B, beta), L, H(ref['state']))
    assert np.array_equal(TC.state_to_scalar(H(r['state']), np.full(B, beta), L)[2], H(r['plaq'])) and torch.equal(r['state'][2], r['Q'])


# ---------------------------------------------------------------- B: a ladder: every chain is the scalar call at its beta
@pytest.mark.parametrize('case,name,nstep', ft_rows())
def test_ladder_chain_by_chain_equals_the_scalar_call_at_its_beta(case, name, nstep):
    B, L = case[2], case[1]
    beta_b = TC.ladder_betas(B)
    r = pb_ft(case, name, nstep, beta_b)
    for beta in sorted(set(beta_b.tolist())):
        ref = scalar_ft(case, name, nstep, beta)
        at = np.nonzero(beta_b == beta)[0]
        idx = torch.as_tensor(at).cuda()
        for k in KEYS:
            assert torch.equal(r[k][idx], ref[k][idx]), (k, beta)
        assert TC.state_matches(H(r['state'])[:, at], beta_b[at], L, H(ref['state'])[:, at]), beta
    assert len(set(H(r['dH']).tolist())) == B                      # the chains are different chains


PLAIN_ROWS = [pytest.param(c, n, s, id=f'{c[0]}-{n}') for c in TC.PLAIN_PATHS for n, s in TC.INTEGRATORS]
PKEYS = ('x_new', 'dH', 'acc', 'H0', 'H1')


@pytest.mark.parametrize('case,name,nstep', PLAIN_ROWS)
def test_plain_hmc_constant_and_ladder_equal_the_scalar_call(case, name, nstep):
    cid, L, B = case
    x, v, u = (t.cuda() for t in IC.draw(300 + L, B, L))
    dt = TC.TAU / nstep
    beta_b = TC.ladder_betas(B)
    ref = {beta: ops.hmc_trajectory(x, v, u, beta, dt, nstep, integrator=name) for beta in sorted(set(beta_b.tolist())) + [2.3]}
    r = ops.hmc_trajectory(x, v, u, D(np.full(B, 2.3)), dt, nstep, integrator=name)
    for k in PKEYS:
        assert torch.equal(r[k], ref[2.3][k]), k
    r = ops.hmc_trajectory(x, v, u, D(beta_b), dt, nstep, integrator=name)
    for b in range(B):
        for k in PKEYS:
            assert torch.equal(r[k][b], ref[float(beta_b[b])][k][b]), (k, b)
    # the operator of the same call
    import fthmc_amd.torch_ops  # noqa: F401
    from fthmc_amd import _lib
    xn, dH, acc = torch.ops.fthmc_hip.hmc_trajectory_pb(x, v, u, D(beta_b), dt, nstep, _lib.INTEGRATORS[name])
    assert torch.equal(xn, r['x_new']) and torch.equal(dH, r['dH']) and torch.equal(acc, r['acc'])


def test_operator_of_the_flowed_call_and_its_fake_shapes():
    import fthmc_amd.torch_ops  # noqa: F401
    case = TC.FT_PATHS[3]                                            # L32
    cid, L, B, nl, arch, variant, small = case
    flow, x, v, u = ft_inputs(cid, L, B, nl, arch)
    beta_b = TC.ladder_betas(B)
    r = pb_ft(case, 'omelyan', 3, beta_b)
    w = ops.pack_weights(flow, device='cuda')
    o = torch.ops.fthmc_hip.ft_trajectory_pb(x.cuda(), v.cuda(), u.cuda(), w, nl, D(beta_b), TC.TAU / 3, 3, 1, 0)
    for got, k in zip(o, ('x_new', 'dH', 'acc', 'plaq', 'Q', 'state')):
        assert torch.equal(got, r[k]), k
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        fx = torch.empty(B, 2, L, L, dtype=torch.float64, device='cuda')
        fo = torch.ops.fthmc_hip.ft_trajectory_pb(fx, fx, torch.empty(B, dtype=torch.float64, device='cuda'),
                                                  torch.empty(nl * 955, dtype=torch.float64, device='cuda'), nl,
                                                  torch.empty(B, dtype=torch.float64, device='cuda'), 0.1, 3, 1, 0)
        assert [tuple(t.shape) for t in fo] == [(B, 2, L, L), (B,), (B,), (B,), (B,), (3, B)]


# ---------------------------------------------------------------- C: against the CPU oracle, chain by chain at its beta
def test_ladder_against_the_oracle_chain_by_chain():
    """leapfrog at L = 8, 2 layers; tolerances of the traj_md_L8 golden test (tests/test_hip_parity.py); the accept decisions are
    decided on the oracle's numbers: |u - exp(-dH)| > 1e-3 for every chain"""
    case = TC.FT_PATHS[0]
    cid, L, B, nl, arch, variant, small = case
    flow, x, v, u = ft_inputs(cid, L, B, nl, arch)
    beta_b = TC.ladder_betas(B)
    nstep = 3
    dt = TC.TAU / nstep
    r = pb_ft(case, 'leapfrog', nstep, beta_b)
    for b in range(B):
        beta = float(beta_b[b])
        dH, e, acc, newx, h0, h1 = R.ft_hmc(x[b:b + 1], v[b:b + 1], u[b:b + 1], flow, beta, dt, nstep, mode='md')
        assert abs(float(u[b]) - float(e)) > 1e-3, 'the draw leaves an accept decision undecided'
        with torch.no_grad():
            y, _ = R.flow_forward(newx, flow)
            pq, q = R.plaq_mean(y, beta), R.charge(y)
        np.testing.assert_allclose(H(r['H0'][b]), H(h0)[0], rtol=1e-10)
        np.testing.assert_allclose(H(r['H1'][b]), H(h1)[0], rtol=1e-7)
        np.testing.assert_allclose(H(r['dH'][b]), H(dH)[0], rtol=1e-6, atol=1e-6)
        assert bool(r['acc'][b] > 0.5) == bool(acc[0])
        d = (H(r['x_new'][b]) - H(newx)[0] + np.pi) % (2 * np.pi) - np.pi
        assert np.max(np.abs(d)) < 1e-6
        np.testing.assert_allclose(H(r['plaq'][b]), H(pq)[0], rtol=1e-6)
        np.testing.assert_allclose(H(r['Q'][b]), H(q)[0], atol=1e-6)


# ---------------------------------------------------------------- D: the carried state is beta-free
@pytest.mark.parametrize('case', [TC.FT_PATHS[i] for i in (0, 3, 7, 8, 9, 10)], ids=lambda c: c[0])
def test_chained_call_after_a_permutation_of_beta_b_equals_the_stateless_call(case):
    cid, L, B, nl, arch, variant, small = case
    flow, x, v, u = ft_inputs(cid, L, B, nl, arch)
    _, v2, u2 = IC.draw(977, B, L)
    beta_b = TC.ladder_betas(B)
    perm = np.roll(beta_b, 1)
    assert not np.array_equal(perm, beta_b)
    nstep, dt = 3, TC.TAU / 3
    with switches(variant=variant, small=small):
        w = ops.pack_weights(flow, device='cuda') if nl else None
        u1 = u.clone(); u1[::2] = 0.0                               # every other chain accepts whatever its dH: both kinds of state are carried
        r1 = ops.ft_trajectory(x.cuda(), v.cuda(), u1.cuda(), w, nl, D(beta_b), dt, nstep)
        x1, st = r1['x_new'].clone(), r1['state'].clone()
        ra = ops.ft_trajectory(x1, v2.cuda(), u2.cuda(), w, nl, D(perm), dt, nstep, state_in=st)
        rb = ops.ft_trajectory(x1, v2.cuda(), u2.cuda(), w, nl, D(perm), dt, nstep)
        torch.cuda.synchronize()
    assert float(r1['acc'][::2].sum()) == len(r1['acc'][::2])
    for k in KEYS + ('state',):
        assert torch.equal(ra[k], rb[k]), k


# ---------------------------------------------------------------- E: k_replica_swap against the numpy round
def swap_inputs(K, M, seed):
    rng = np.random.default_rng(seed)
    betas = np.cumsum(rng.uniform(0.3, 1.2, K))
    bb, rung, chain_of = TC.random_ladders(rng, betas, M)
    C = rng.normal(0.0, 2.0, M * K)
    u = rng.uniform(0.0, 1.0, (M, K - 1))
    # edge inputs: C_a = C_c exactly in ladder 0 on the first pair of either parity (d = 0, exp(d) = 1: must accept for every
    # u < 1, here 0.999), and u = 0 on the last pair of the last ladder (must accept whatever d)
    C[chain_of[1]] = C[chain_of[0]]
    u[0, 0] = 0.999
    if K > 2:
        C[chain_of[2]] = C[chain_of[1]]
        u[0, 1] = 0.999
    u[M - 1, K - 2] = 0.0
    return betas, bb, rung, chain_of, C, u


@pytest.mark.parametrize('parity', [0, 1])
@pytest.mark.parametrize('M', [1, 3])
@pytest.mark.parametrize('K', [2, 3, 4, 7])
def test_replica_swap_against_the_numpy_round(K, M, parity):
    betas, bb, rung, chain_of, C, u = swap_inputs(K, M, 1000 + 10 * K + M)
    nb, nr, nc, acc, d, e = TC.swap_round(betas, C, u, bb, rung, chain_of, parity)
    tried = acc >= 0
    # condition, on the reference alone: no drawn u within 1e-12 relative of exp(d) -- a one-ulp exp cannot decide a case
    assert np.all(np.abs(u[tried] - e[tried]) > 1e-12 * e[tried])
    if parity < K - 1:
        assert acc[0, parity] == 1.0 and d[0, parity] == 0.0             # C_a = C_c: accepted
    if (K - 2) % 2 == parity:
        assert acc[M - 1, K - 2] == 1.0                                  # u = 0
    g_bb, g_r, g_c = D(bb), D(rung, torch.int32), D(chain_of, torch.int32)
    out = ops.replica_swap(D(betas), D(C), D(u), g_bb, g_r, g_c, parity)
    torch.cuda.synchronize()
    assert np.array_equal(H(out['swap_acc']), acc)
    assert np.array_equal(H(g_bb).view(np.int64), nb.view(np.int64)) and np.array_equal(H(g_r), nr) and np.array_equal(H(g_c), nc)
    gd = H(out['d'])
    assert np.all(np.abs(gd - d) <= 2 * np.spacing(np.abs(d)))
    assert np.all(gd[~tried] == 0.0)
    # the operator: the same bits from the same start
    import fthmc_amd.torch_ops  # noqa: F401
    o_bb, o_r, o_c = D(bb), D(rung, torch.int32), D(chain_of, torch.int32)
    o_acc, o_d = torch.ops.fthmc_hip.replica_swap(D(betas), D(C), D(u), o_bb, o_r, o_c, parity)
    assert torch.equal(o_acc, out['swap_acc']) and torch.equal(o_d, out['d'])
    assert torch.equal(o_bb, g_bb) and torch.equal(o_r, g_r) and torch.equal(o_c, g_c)


# ---------------------------------------------------------------- F: invariants after 50 rounds
@pytest.mark.parametrize('K,M', [(2, 1), (4, 3), (7, 5)])
def test_ladder_invariants_after_50_rounds(K, M):
    rng = np.random.default_rng(50 + K)
    betas = np.cumsum(rng.uniform(0.1, 0.4, K))
    lad = ops.ladder_init(betas, M, device='cuda')
    TC.check_ladders(betas, H(lad['beta_b']), H(lad['rung']), H(lad['chain_of']))
    assert np.array_equal(H(lad['rung']), np.tile(np.arange(K), M)) and np.array_equal(H(lad['betas']), betas)
    ref = (H(lad['beta_b']), H(lad['rung']), H(lad['chain_of']))
    moved = 0
    for it in range(50):
        C, u = rng.normal(0.0, 1.5, M * K), rng.uniform(0.0, 1.0, (M, K - 1))
        out = ops.replica_swap(lad['betas'], D(C), D(u), lad['beta_b'], lad['rung'], lad['chain_of'], it % 2)
        nb, nr, nc, acc, d, e = TC.swap_round(betas, C, u, *ref, it % 2)
        assert np.all(np.abs(u[acc >= 0] - e[acc >= 0]) > 1e-12 * e[acc >= 0])
        ref = (nb, nr, nc)
        moved += int((acc > 0.5).sum())
        assert np.array_equal(H(out['swap_acc']), acc)
    TC.check_ladders(betas, H(lad['beta_b']), H(lad['rung']), H(lad['chain_of']))
    assert np.array_equal(H(lad['rung']), ref[1]) and np.array_equal(H(lad['chain_of']), ref[2])
    assert moved > 10


# ---------------------------------------------------------------- G: the driver
def _param(L, tau=1.0, nstep=10, seed=143, randinit=True):
    from fthmc_amd.config import Param
    return Param(L=L, tau=tau, nstep=nstep, seed=seed, randinit=randinit)


HKEYS = ('plaq', 'Q', 'acc', 'dH', 'rung', 'swap_rounds')


def test_run_tempered_captured_equals_eager():
    from fthmc_amd.tempering import run_tempered
    flow = flow_of(61, 2)
    p = _param(8, tau=0.5, nstep=4)
    hc = run_tempered(p, flow, (1.0, 2.0, 3.0), 2, 6, captured=True)
    he = run_tempered(p, flow, (1.0, 2.0, 3.0), 2, 6, captured=False)
    for k in HKEYS:
        assert np.array_equal(hc[k], he[k]), k
    assert torch.equal(hc['x'], he['x']) and torch.equal(hc['beta_b'], he['beta_b']) and torch.equal(hc['rung_last'], he['rung_last'])
    assert hc['plaq'].shape == (6, 3, 2) and hc['rung'].shape == (6, 6) and hc['swap_rounds'].shape == (6, 2, 2)
    # parities alternate: pair 0 in rounds 0, 2, 4, pair 1 in rounds 1, 3, 5
    assert np.all(hc['swap_rounds'][0::2, :, 1] == -1) and np.all(hc['swap_rounds'][0::2, :, 0] >= 0)
    assert np.all(hc['swap_rounds'][1::2, :, 0] == -1) and np.all(hc['swap_rounds'][1::2, :, 1] >= 0)
    # an odd count runs the rest of the last period eagerly
    h7 = run_tempered(p, flow, (1.0, 2.0, 3.0), 2, 7, captured=True)
    for k in HKEYS:
        assert np.array_equal(h7[k][:6], hc[k]), k


def test_run_tempered_does_not_depend_on_groups():
    from fthmc_amd.tempering import run_tempered
    flow = flow_of(62, 1)
    p = _param(64, tau=0.2, nstep=2)
    h1 = run_tempered(p, flow, (1.0, 2.0, 3.0, 4.0), 8, 2, groups=1)
    h2 = run_tempered(p, flow, (1.0, 2.0, 3.0, 4.0), 8, 2, groups=2)
    for k in HKEYS:
        assert np.array_equal(h1[k], h2[k]), k
    assert torch.equal(h1['x'], h2['x'])


def test_two_shards_of_whole_ladders_equal_one_batch():
    from fthmc_amd.tempering import run_tempered
    flow = flow_of(63, 2)
    p = _param(8, tau=0.5, nstep=4)
    full = run_tempered(p, flow, (1.0, 2.0, 3.0), 4, 6)
    for rank in (0, 1):
        part = run_tempered(p, flow, (1.0, 2.0, 3.0), 4, 6, shard=(rank, 2))
        lad = slice(2 * rank, 2 * rank + 2)
        for k in ('plaq', 'Q', 'acc', 'dH'):
            assert np.array_equal(part[k], full[k][:, :, lad]), (k, rank)
        assert np.array_equal(part['rung'], full['rung'][:, 6 * rank:6 * rank + 6])
        assert np.array_equal(part['swap_rounds'], full['swap_rounds'][:, lad])
        assert torch.equal(part['x'], full['x'][6 * rank:6 * rank + 6])
    with pytest.raises(ValueError):
        run_tempered(p, flow, (1.0, 2.0, 3.0), 3, 6, shard=(0, 2))


# ---------------------------------------------------------------- H: the sampler is exact at every rung
@pytest.mark.parametrize('nl', [0, 2], ids=['plain', 'flowed'])
def test_tempered_sampler_is_exact_at_every_rung(nl):
    """L = 8, ladder (1, 2, 3, 4), 64 ladders, tau = 1, 10 leapfrog steps, 300 + 3000 trajectories, a swap round behind every
    trajectory, fixed seed: per rung |<plaq> - exact| <= 5 se, se from 30 block means of 100 trajectories (se <= 5e-4 is a condition),
    exact = sum_n I_n^(V-1) I_n' / sum_n I_n^V at V = 64; the pullback of the Wilson measure through a flow has the same plaquette.
    Plain run: swap acceptance per pair within 25 % of 0.0050, 0.061, 0.196 (a numpy run of the same set-up).  A reversed sign in
    the exchange rule misses the plaquette bound by hundreds of se."""
    from fthmc_amd.tempering import run_tempered
    betas = (1.0, 2.0, 3.0, 4.0)
    p = _param(8, tau=1.0, nstep=10, seed=2024, randinit=False)
    flow = flow_of(64, nl) if nl else None
    h = run_tempered(p, flow, betas, 64, 3300, swap_every=1)
    plaq = h['plaq'][300:]                                             # [3000, K, M]
    per_traj = plaq.mean(axis=2)                                        # [3000, K]
    blocks = per_traj.reshape(30, 100, 4).mean(axis=1)                  # 30 block means of 100 trajectories
    mean, se = blocks.mean(axis=0), blocks.std(axis=0, ddof=1) / math.sqrt(30)
    exact = np.array([TC.exact_plaquette(b, 64) for b in betas])
    print('plaq mean', mean, 'exact', exact, 'se', se, '(mean - exact) / se', (mean - exact) / se)
    print('swap acceptance', h['swap_acc'], 'tried', h['swap_tried'], 'HMC acceptance per rung', h['acc'][300:].mean(axis=(0, 2)),
          'round trips per ladder', h['round_trips'].sum() / 64)
    assert np.all(se <= 5e-4), se
    assert np.all(np.abs(mean - exact) <= 5 * se), (mean - exact) / se
    if nl == 0:
        want = np.array([0.0050, 0.061, 0.196])
        assert np.all(np.abs(h['swap_acc'] - want) <= 0.25 * want), h['swap_acc']
