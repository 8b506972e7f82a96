"""GPU tests of the instanton hit (fthmc_amd/csrc/topo.hip): the two sums, the decisions and every link of a call against the
longdouble twin of tests/instanton_cases.py inside the twin's derived bounds, on both launch shapes; the bit-equalities the header
promises; the compositions; the drivers; and the exact finite-volume charge distribution as the physics check.

Every number a device result is held against comes from the twin or from utils.observables.exact_charge_distribution."""
import math

import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401

import instanton_cases as IC
import local_update_cases as LC

from gpu_support import D, H, module_defaults, ops

pytestmark = pytest.mark.gpu
_defaults = module_defaults()

LD = np.longdouble


def S(seeds):
    return torch.from_numpy(np.asarray(seeds, dtype=np.int64)).cuda()


def call(xd, beta, sd, n_hit, hit0, path, out=None):
    """-> (x_new, k, nacc, cs) on the device"""
    o = {'cs': torch.empty(xd.shape[0], 2, dtype=torch.float64, device='cuda')}
    if out is not None:
        o['x'] = out
    xn, k, nacc = ops.instanton_hit(xd, beta, sd, n_hit=n_hit, hit0=hit0, path=path, out=o)
    return xn, k, nacc, o['cs']


IDS = lambda v: f'{v:g}'


# ---------------------------------------------------------------- 1. sums, decisions, links, action and charge against the twin
@pytest.mark.parametrize('path', [1, 2], ids=['chain', 'split'])
@pytest.mark.parametrize('hits', IC.HITS, ids=lambda v: f'{v[0]}x{v[1]}')
@pytest.mark.parametrize('B,L,amp,beta', IC.CASES, ids=IDS)
def test_a_call_against_the_twin(B, L, amp, beta, hits, path):
    x, seeds = IC.fields(B, L, amp)
    xd, sd = D(x), S(seeds)
    S0, Q0, _ = ops.wilson_action_charge(xd, beta)
    C1 = -H(ops.wilson_action_charge(xd, 1.0)[0])
    cs0 = H(ops.instanton_sums(xd, path=path))
    for n_hit, hit0 in (hits,):
        _, _, t = IC.case(B, L, amp, beta, n_hit, hit0)
        assert not t['ambiguous'].any(), 'a chain would be left out'
        xn, k, nacc, cs = call(xd, beta, sd, n_hit, hit0, path)
        assert torch.equal(xd, D(x)), 'the input was written'
        cs, y = H(cs), H(xn)
        assert np.array_equal(cs, cs0), 'the sums depend on n_hit'
        eC = np.abs((cs[:, 0].astype(LD) - t['C']).astype(np.float64)) / t['dC']
        eS = np.abs((cs[:, 1].astype(LD) - t['Sn']).astype(np.float64)) / t['dSn']
        eW = np.abs((C1.astype(LD) - t['C']).astype(np.float64)) / t['dC']
        assert np.array_equal(H(k), t['k']) and np.array_equal(H(nacc), t['nacc']), 'decisions differ from the twin'
        mv = t['moved']
        assert np.array_equal(y[~mv], x[~mv]), 'a zero-shift link is not bit-equal'
        still = t['k'] == 0
        assert np.array_equal(y[still], x[still]), 'a chain with k = 0 changed'
        ratio = LC.circ_dist(y, t['x']) / np.where(mv, t['bound'], 1.0)
        worst = float(ratio[mv].max()) if mv.any() else 0.0
        assert np.all(y[mv] >= -math.pi) and np.all(y[mv] < math.pi)
        # the action after - before = the closed form summed over the accepted steps: both evaluations of S within the bound of C
        # (that of the new field from the twin's own sums of it), every moved link in two plaquettes (|d cos P| <= |d P|)
        S1, Q1, _ = ops.wilson_action_charge(xn, beta)
        closed = (t['dS'] * t['accepted']).sum(axis=1)
        dC1 = IC.sums(t['x'].astype(np.float64))[2]
        tolS = beta * (t['dC'] + 1.01 * dC1 + 2.0 * t['bound'].reshape(B, -1).sum(axis=1)) + (t['dS_bound'] * t['accepted']).sum(axis=1) \
            + 4 * LC.U * np.abs(H(S0))
        eA = np.abs((H(S1).astype(LD) - H(S0).astype(LD) - closed).astype(np.float64)) / tolS
        dq_twin = IC.charge(t['x'])[0] - IC.charge(x)[0]
        dq = H(Q1) - H(Q0)
        assert np.array_equal(np.rint(dq).astype(np.int64), dq_twin) and np.abs(dq - np.rint(dq)).max() < 1e-8, 'dQ differs from the twin'
        if amp < 1.0:
            assert np.array_equal(dq_twin, t['k']), 'dQ != k on the smooth field'
        print(f'B {B} L {L} amp {amp:.3g} beta {beta} path {path} n_hit {n_hit} hit0 {hit0}: err / bound C {eC.max():.3f} Sn {eS.max():.3f} '
              f'wilson C {eW.max():.3f} links {worst:.3f} dS {eA.max():.3f}; acceptance {t["nacc"].mean() / n_hit:.3f}, max |k| {np.abs(t["k"]).max()}, '
              f'smallest margin {t["margin"].min():.2e}')
        assert max(eC.max(), eS.max(), eW.max()) <= 1.0 and worst <= 1.0 and eA.max() <= 1.0


# ---------------------------------------------------------------- 2. bit-equalities
@pytest.mark.parametrize('B,L', IC.SHAPES)
def test_paths_in_place_repeats_and_n_hit_zero_are_bit_equal(B, L):
    x, seeds = IC.fields(B, L, math.pi)
    xd, sd = D(x), S(seeds)
    for n_hit, hit0 in IC.HITS + ((0, 0),):
        a = call(xd, 2.0, sd, n_hit, hit0, 1)
        b = call(xd, 2.0, sd, n_hit, hit0, 2)
        c = call(xd, 2.0, sd, n_hit, hit0, 0)
        for u, v, w in zip(a, b, c):
            assert torch.equal(u, v) and torch.equal(u, w), 'one workgroup per chain and the split form differ'
        for path in (1, 2):
            z = xd.clone()
            r = call(z, 2.0, sd, n_hit, hit0, path, out=z)
            assert r[0].data_ptr() == z.data_ptr()
            for u, v in zip(a, r):
                assert torch.equal(u, v), 'x_out = x differs from a separate output'
            for u, v in zip(a, call(xd, 2.0, sd, n_hit, hit0, path)):
                assert torch.equal(u, v), 'two identical calls differ'
        if n_hit == 0:
            assert torch.equal(a[0], xd) and int(a[1].abs().max()) == 0 and int(a[2].abs().max()) == 0, 'n_hit = 0 is not the identity'
            y, k, nacc = ops.instanton_hit(xd, 2.0, None, n_hit=0)
            assert torch.equal(y, xd) and int(k.abs().max()) == 0
    assert torch.equal(xd, D(x)), 'the input was written'


@pytest.mark.parametrize('path', [1, 2], ids=['chain', 'split'])
@pytest.mark.parametrize('B,L', [(3, 4), (3, 8), (2, 12), (2, 20), (2, 64), (2, 68), (2, 128), (130, 16), (66000, 4)])
def test_a_chain_of_a_batch_equals_the_chain_alone_and_per_chain_beta_equals_scalar_calls(B, L, path):
    x, seeds = LC.uniform_links(B, L, 1000 + L), LC.chain_seeds(B, 3000 + L)      # SHAPES, two chains where it has one
    xd, sd = D(x), S(seeds)
    n_hit, hit0 = 5, 7
    full = call(xd, 2.0, sd, n_hit, hit0, path)
    for b in sorted({0, B // 2, B - 1}):
        one = call(xd[b:b + 1].contiguous(), 2.0, sd[b:b + 1].contiguous(), n_hit, hit0, path)
        for u, v in zip(full, one):
            assert torch.equal(u[b], v[0]), b
    const = torch.full((B,), 2.0, dtype=torch.float64, device='cuda')
    for u, v in zip(full, call(xd, const, sd, n_hit, hit0, path)):
        assert torch.equal(u, v), 'beta_b = beta differs from the scalar call'
    betas = torch.linspace(0.5, 40.0, B, dtype=torch.float64, device='cuda')
    pb = call(xd, betas, sd, n_hit, hit0, path)
    for b in sorted({0, B // 2, B - 1}):
        one = call(xd[b:b + 1].contiguous(), float(betas[b]), sd[b:b + 1].contiguous(), n_hit, hit0, path)
        for u, v in zip(pb, one):
            assert torch.equal(u[b], v[0]), b
    assert torch.equal(pb[3], full[3]) and (B < 100 or not torch.equal(pb[2], full[2]))


# ---------------------------------------------------------------- 3. composition
@pytest.mark.parametrize('path', [1, 2], ids=['chain', 'split'])
@pytest.mark.parametrize('B,L', [(3, 8), (2, 20), (130, 16)])
def test_five_hits_equal_five_calls_of_one(B, L, path):
    """one call decides its five steps on the sums of the field it received; five calls re-reduce the sums of the field as shifted
    so far.  The same decisions wherever the margins permit (the twin of the five calls says so: none left out), the links within
    the added bounds"""
    x, seeds = IC.fields(B, L, math.pi)
    xd, sd = D(x), S(seeds)
    hit0 = 2 ** 32 - 5
    xa, ka, na, _ = call(xd, 2.0, sd, 5, hit0, path)
    y, ty, ktot, ntot, bound = xd, x, torch.zeros_like(ka), torch.zeros_like(na), np.zeros(x.shape)
    for h in range(5):
        t = IC.hits(ty, 2.0, seeds, 1, hit0 + h)
        assert not t['ambiguous'].any(), 'choose other seeds: a chain would be left out'
        y, k1, n1, _ = call(y, 2.0, sd, 1, hit0 + h, path)
        assert np.array_equal(H(k1), t['k'])
        ty = H(y)
        ktot, ntot, bound = ktot + k1, ntot + n1, bound + t['bound']
    one = IC.hits(x, 2.0, seeds, 5, hit0)
    # the single call's steps see C, Sn of x, the h-th of the five calls those of the field as shifted so far; the closed form is an
    # identity, so the two differ by rounding only (below 1e-11 in exp(-dS) at these sizes: the bounds of the sums are 5e-13): the
    # same decisions unless a margin is of that size
    assert not one['ambiguous'].any() and float(one['margin'].min()) > 1e-9
    assert torch.equal(ka, ktot) and torch.equal(na, ntot)
    d = LC.circ_dist(H(xa), ty)
    tol = bound + one['bound'] + 2.0 ** -50
    assert np.all(d <= tol), float((d / tol).max())


# ---------------------------------------------------------------- 4. the drivers, the helper, the operator
def _hist_equal(a, b):
    assert a.keys() == b.keys()
    for n in a:
        assert a[n].keys() == b[n].keys()
        for k in a[n]:
            if k == 'dt':
                continue
            assert len(a[n][k]) == len(b[n][k]), k
            for u, v in zip(a[n][k], b[n][k]):
                assert torch.equal(torch.as_tensor(u).cpu(), torch.as_tensor(v).cpu()), (n, k)


def test_run_local_with_hits_captured_equals_eager():
    from fthmc_amd.config import Param
    from fthmc_amd.local import run_local
    param = Param(beta=2.0, L=8, ntraj=7, nrun=2, nprint=0)
    x0 = D(LC.uniform_links(4, 8, 31))
    fa, ha = run_local(param, x0, n_overrelax=1, loops=(3, 4), loops_every=3, use_graph=True, instanton=2)
    fb, hb = run_local(param, x0, n_overrelax=1, loops=(3, 4), loops_every=3, use_graph=False, instanton=2)
    _hist_equal(ha, hb)
    for u, v in zip(fa, fb):
        assert torch.equal(u, v)
    assert set(ha[0]) == {'traj', 'dt', 'acc', 'plaq', 'q', 'dq', 'wloops', 'inst_acc', 'inst_dq'} and len(ha[0]['inst_acc']) == 7
    acc = torch.stack(ha[0]['inst_acc'] + ha[1]['inst_acc'])
    dq = torch.stack(ha[0]['inst_dq'] + ha[1]['inst_dq'])
    assert tuple(acc.shape) == (14, 4) and set(np.unique(acc.numpy())) <= {0.0, 0.5, 1.0} and int(dq.abs().max()) in (1, 2) and float(acc.mean()) > 0.1
    assert tuple(ha[0]['wloops'][0].shape) == (3, 4)
    S_, Q_, plaq_ = ops.wilson_action_charge(fa[1], 2.0)
    assert torch.equal(plaq_.cpu(), ha[1]['plaq'][-1]) and torch.equal(Q_.cpu(), ha[1]['q'][-1])
    # the hits move the charge: without them the same sweeps give another history
    _, hc = run_local(param, x0, n_overrelax=1, loops=(3, 4), loops_every=3, use_graph=True)
    assert not torch.equal(torch.stack(hc[0]['q']), torch.stack(ha[0]['q']))
    with pytest.raises(ValueError):
        run_local(param, x0, instanton=-1)


def test_instanton_zero_changes_nothing_in_the_three_drivers(tmp_path):
    from fthmc_amd import train as T
    from fthmc_amd.config import Param, TrainConfig
    from fthmc_amd.hmc import run_hmc
    from fthmc_amd.local import run_local
    from fthmc_amd.utils import qed_helpers as qed
    param = Param(beta=2.0, L=8, ntraj=6, nrun=1, nprint=0, randinit=True)
    torch.manual_seed(5); fa, ha = run_hmc(param, overrelax=1)
    torch.manual_seed(5); fb, hb = run_hmc(param, overrelax=1, instanton=0)
    _hist_equal(ha, hb)
    assert all(torch.equal(u, v) for u, v in zip(fa[0], fb[0]))
    torch.manual_seed(5); fc, hc = run_hmc(param, overrelax=1, instanton=2)
    assert set(hc[0]) == set(ha[0]) | {'inst_acc', 'inst_dq'} and len(hc[0]['inst_dq']) == 6
    with pytest.raises(ValueError):
        run_hmc(param, instanton=-1)
    x0 = D(LC.uniform_links(4, 8, 31))
    for graph in (True, False):
        fa, ha = run_local(param, x0, n_overrelax=1, loops=(2, 2), use_graph=graph)
        fb, hb = run_local(param, x0, n_overrelax=1, loops=(2, 2), use_graph=graph, instanton=0)
        _hist_equal(ha, hb)
        assert torch.equal(fa[0], fb[0])
    cfg = TrainConfig(L=8, beta=2.0, n_layers=2, batch_size=1, print_freq=0)
    torch.manual_seed(21)
    model = T.get_model(cfg)
    fparam = Param(beta=2.0, L=8, tau=1.0, nstep=6, ntraj=4, nrun=1)
    f0 = (0.4 * (2 * torch.rand(2, 8, 8, dtype=torch.float64) - 1)).cuda()
    for graph in (True, False):
        res = []
        for kw in ({}, {'instanton': 0}, {'instanton': 2}):
            torch.manual_seed(8); torch.cuda.manual_seed(8)
            res.append(qed.ft_run(fparam, model.layers, f0.clone(), use_graph=graph, **kw))
        (f1, h1), (f2, h2), (f3, h3) = res
        assert torch.equal(f1, f2) and h1 == h2 and list(h1) == list(h2)
        assert set(h3) == set(h1) | {'inst_acc', 'inst_dq'} and len(h3['inst_dq']) == 4 and len(h3['plaq']) == 4
        S_, Q_, plaq_ = ops.wilson_action_charge(f3[None].contiguous(), 2.0)
        assert float(plaq_[0]) == h3['plaq'][-1] and float(Q_[0]) == h3['topo'][-1]     # measured behind the hits


def test_qed_helper_and_the_torch_operator():
    from fthmc_amd.config import Param
    from fthmc_amd.utils import qed_helpers as qed
    import fthmc_amd.torch_ops  # noqa: F401
    param = Param(beta=2.0, L=8)
    x, seeds = IC.fields(3, 8, math.pi)
    xd, sd = D(x), S(seeds)
    ref = ops.instanton_hit(xd, 2.0, sd, n_hit=5)
    for u, v in zip(qed.instanton_hit(param, xd, 5, sd), ref):
        assert torch.equal(u, v)
    y, k, nacc = qed.instanton_hit(param, xd[0])
    assert tuple(y.shape) == (2, 8, 8) and tuple(k.shape) == (1,) and k.dtype == torch.int32
    for u, v in zip(torch.ops.fthmc_hip.instanton_hit(xd, 2.0, None, sd, 5, 0), ref):
        assert torch.equal(u, v)
    bb = torch.linspace(1.0, 3.0, 3, dtype=torch.float64, device='cuda')
    for u, v in zip(torch.ops.fthmc_hip.instanton_hit(xd, 0.0, bb, sd, 64, 2 ** 32 - 64), ops.instanton_hit(xd, bb, sd, n_hit=64, hit0=2 ** 32 - 64)):
        assert torch.equal(u, v)
    big = D(LC.uniform_links(2, 128, 3))                                 # the library's choice here is the split form, with a workspace
    for u, v in zip(torch.ops.fthmc_hip.instanton_hit(big, 2.0, None, sd[:2].contiguous(), 3), ops.instanton_hit(big, 2.0, sd[:2].contiguous(), n_hit=3, path=1)):
        assert torch.equal(u, v)
    torch.library.opcheck(torch.ops.fthmc_hip.instanton_hit.default, (xd, 2.0, None, sd, 5, 7), test_utils=('test_schema', 'test_faketensor'))
    torch.library.opcheck(torch.ops.fthmc_hip.instanton_hit.default, (xd, 0.0, bb, None, 0), test_utils=('test_schema', 'test_faketensor'))
    with pytest.raises(RuntimeError):
        torch.ops.fthmc_hip.instanton_hit(xd, 2.0, None, None, 1)                # a hit without seeds
    with pytest.raises(ValueError):
        ops.instanton_hit(xd, 2.0, sd, n_hit=1025)
    with pytest.raises(ValueError):
        ops.instanton_hit(xd, 2.0, sd, n_hit=2, hit0=2 ** 32 - 1)


# ---------------------------------------------------------------- 5. the exact charge distribution
def test_hmc_with_hits_reproduces_the_exact_charge_distribution():
    """L = 8, beta = 4, 256 chains from a cold start, 100 + 400 plain-HMC trajectories (tau = 1) each followed by two hits: <Q^2> and
    P(0) against the exact finite-volume values, the standard error from the 256 chain means.  Measured z-scores: DESIGN 4.14."""
    from fthmc_amd.utils import observables as O
    B, L, beta, ntherm, nmeas, n_hit = 256, 8, 4.0, 100, 400, 2
    torch.manual_seed(77); torch.cuda.manual_seed(77)
    x = torch.zeros(B, 2, L, L, dtype=torch.float64, device='cuda')
    seeds = S(LC.chain_seeds(B, 7001))
    v, u = torch.empty_like(x), torch.empty(B, dtype=torch.float64, device='cuda')
    q2, p0 = torch.zeros(B, dtype=torch.float64, device='cuda'), torch.zeros(B, dtype=torch.float64, device='cuda')
    nacc = torch.zeros(B, dtype=torch.int64, device='cuda')
    for t in range(ntherm + nmeas):
        v.normal_(); u.uniform_()
        x = ops.hmc_trajectory(x, v, u, beta, 0.1, 10)['x_new']
        x, k, na = ops.instanton_hit(x, beta, seeds, n_hit=n_hit, hit0=n_hit * t)
        if t >= ntherm:
            Q = torch.round(ops.wilson_action_charge(x, beta)[1])
            q2 += Q * Q; p0 += (Q == 0).to(torch.float64); nacc += na
    q2, p0, acc = H(q2) / nmeas, H(p0) / nmeas, float(nacc.sum()) / (B * nmeas * n_hit)
    p = O.exact_charge_distribution(beta, L, 12)
    zs = []
    for name, val, exact in (('<Q^2>', q2, 0.4820159295), ('P(0)', p0, float(p[12]))):
        se = val.std(ddof=1) / math.sqrt(B)
        zs.append((val.mean() - exact) / se)
        print(f'{name}: {val.mean():.5f} +- {se:.5f}, exact {exact:.5f}, z {zs[-1]:+.2f}')
    print(f'hit acceptance {acc:.3f}')
    assert abs(zs[0]) <= 4.0 and abs(zs[1]) <= 4.0, zs
    assert 0.2 < acc < 0.7, acc
