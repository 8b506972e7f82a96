"""GPU tests of the local-update sampler (fthmc_amd/csrc/local.hip): every class of a heatbath and of an overrelaxation sweep against
the longdouble twin of tests/local_update_cases.py, link by link inside the twin's derived bound, on both paths (the one-launch
kernel with the chain in LDS, and one launch per class); the compositions the header promises, bit for bit; independence of the
batch; conservation of the action; the near-cancelling staple pair; the exact finite-volume loop table; the drivers.

Every number a device result is held against comes from the twin or from the exact formula (utils.observables.exact_wilson_loop)."""
import math

import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401

import local_update_cases as LC
import wilson_loop_cases as WC

from gpu_support import D, H, module_defaults, ops, switches

pytestmark = pytest.mark.gpu
_defaults = module_defaults()

BETA, SWEEP = LC.BETA, LC.SWEEP


# switches(small=resident): the one-launch kernel where it serves (True), or the class kernels at every L (False)
def S(seeds):
    return torch.from_numpy(np.asarray(seeds, dtype=np.int64)).cuda()


case = LC.case


def update(x, kind, seeds=None, beta=BETA, **kw):
    return ops.local_update(x, beta, seeds, n_hb=1 if kind == 'hb' else 0, n_or=1 if kind == 'or' else 0, **kw)


# ---------------------------------------------------------------- 1. per class, per link, against the twin
@pytest.mark.parametrize('resident', [True, False], ids=['one-launch', 'class-kernels'])
@pytest.mark.parametrize('kind', ['or', 'hb'])
@pytest.mark.parametrize('B,L,amp', LC.CASES, ids=lambda v: str(int(v)))
def test_every_class_alone_against_the_twin_link_by_link(B, L, amp, kind, resident):
    x, seeds, twin = case(B, L, kind, amp)
    xd, sd = D(x), S(seeds)
    for k, t in enumerate(twin):
        mu, p = LC.CLASSES[k]
        with switches(small=bool(resident)):
            y = H(update(xd, kind, sd, classes=1 << k, sweep0=SWEEP))
        other = np.ones((2, L, L), dtype=bool); other[mu, t['ii'], t['jj']] = False
        assert np.array_equal(y[:, other], x[:, other]), f'class {mu, p}: a link outside the class changed'
        new = y[:, mu, t['ii'], t['jj']]
        assert np.all(np.isfinite(new)) and np.all(new >= -math.pi) and np.all(new < math.pi)
        keep = t['margin'].min(axis=1) >= LC.MARGIN_MIN
        assert int((~keep).sum()) <= B // 10000, f'{int((~keep).sum())} chains left out'
        ratio = LC.circ_dist(new, t['new']) / t['bound']
        worst = float(ratio[keep].max())
        print(f'B {B} L {L} amp {amp:.3g} {kind} class {mu, p} resident {resident}: max err / bound {worst:.3f}, median bound '
              f'{np.median(t["bound"]):.2e}, left out {int((~keep).sum())}, attempts max {int(t["attempts"].max())}')
        assert worst <= 1.0, (mu, p, worst)
        assert float(np.median(t['bound'])) < 1e-12


# ---------------------------------------------------------------- 2. composition, device against device, bit for bit
@pytest.mark.parametrize('B,L', LC.SHAPES)
def test_compositions_are_bit_equal(B, L):
    x, seeds, _ = case(B, L, 'hb')
    xd, sd = D(x), S(seeds)
    outs = {}
    for resident in (True, False):
        with switches(small=bool(resident)):
            full = ops.local_update(xd, BETA, sd, n_hb=1, n_or=1, sweep0=5)
            y = xd
            for n_hb, n_or in ((1, 0), (0, 1)):
                for k in range(4):
                    y = ops.local_update(y, BETA, sd, n_hb=n_hb, n_or=n_or, sweep0=5, classes=1 << k)
            assert torch.equal(full, y), 'a full compound sweep is not its eight class updates in order'
            three = ops.local_update(xd, BETA, sd, n_hb=2, n_or=1, nsweep=3, sweep0=7)
            y = xd
            for s in range(3):
                y = ops.local_update(y, BETA, sd, n_hb=2, n_or=1, nsweep=1, sweep0=7 + 2 * s)
            assert torch.equal(three, y), 'nsweep = 3 is not three calls with sweep0 moved on by n_hb'
            z = xd.clone()
            r = ops.local_update(z, BETA, sd, n_hb=2, n_or=1, nsweep=3, sweep0=7, out=z)
            assert r.data_ptr() == z.data_ptr() and torch.equal(z, three), 'x_out = x differs from a separate output'
            assert torch.equal(ops.local_update(xd, BETA, sd, n_hb=2, n_or=1, nsweep=3, sweep0=7), three), 'two identical calls differ'
            assert torch.equal(xd, D(x)), 'the input was written'
            outs[resident] = (full, three)
    for a, b in zip(outs[True], outs[False]):
        assert torch.equal(a, b), 'the one-launch kernel and the class kernels differ'


# ---------------------------------------------------------------- 3. a chain's update depends on the chain alone
@pytest.mark.parametrize('resident', [True, False], ids=['one-launch', 'class-kernels'])
@pytest.mark.parametrize('B,L', [(3, 4), (3, 8), (2, 12), (2, 20), (2, 64), (2, 68), (2, 128), (130, 16), (66000, 4)])
def test_a_chain_of_a_batch_equals_the_chain_alone_and_per_chain_beta_equals_scalar_calls(B, L, resident):
    x, seeds = LC.uniform_links(B, L, 1000 + L), LC.chain_seeds(B, 2000 + L)      # the issue's shapes, two chains where it has one
    xd, sd = D(x), S(seeds)
    kw = dict(n_hb=1, n_or=1, nsweep=2, sweep0=1)
    with switches(small=bool(resident)):
        full = ops.local_update(xd, BETA, sd, **kw)
        for b in sorted({0, B // 2, B - 1}):
            assert torch.equal(ops.local_update(xd[b:b + 1].contiguous(), BETA, sd[b:b + 1].contiguous(), **kw)[0], full[b]), b
        const = torch.full((B,), BETA, dtype=torch.float64, device='cuda')
        assert torch.equal(ops.local_update(xd, const, sd, **kw), full), 'beta_b = beta differs from the scalar call'
        betas = torch.linspace(0.5, 6.0, B, dtype=torch.float64, device='cuda')
        pb = ops.local_update(xd, betas, sd, **kw)
        for b in sorted({0, B // 2, B - 1}):
            one = ops.local_update(xd[b:b + 1].contiguous(), float(betas[b]), sd[b:b + 1].contiguous(), **kw)
            assert torch.equal(one[0], pb[b]), b
        assert not torch.equal(pb, full)


# ---------------------------------------------------------------- 4. overrelaxation conserves the action and the charge
@pytest.mark.parametrize('resident', [True, False], ids=['one-launch', 'class-kernels'])
@pytest.mark.parametrize('B,L', [(3, 8), (2, 64), (1, 68)])
def test_overrelaxation_conserves_action_and_charge_over_ten_sweeps(B, L, resident):
    x, _, _ = case(B, L, 'or')
    # the twin's ten sweeps: what every link may be off by, summed; and how close a plaquette comes to +-pi on the way
    y, moved, gap = x, np.zeros(B), math.inf
    for _ in range(10):
        for mu, p in LC.CLASSES:
            r = LC.class_update(y, mu, p, 'or', BETA)
            y = r['x'].astype(np.float64)
            moved += r['bound'].sum(axis=1)
            P = (LC.plaquettes(y) + math.pi) % (2 * math.pi) - math.pi
            gap = min(gap, float((math.pi - np.abs(P)).min()))
    n = L * L
    # a link sits in two plaquettes (|d cos P| <= |d P|), and each of the two evaluations of S sums n cosines (3 u each with their
    # angle) in runs of at most n / 64 per thread and a 16-level tree
    tol = BETA * (2.0 * moved + 2.0 * LC.U * n * (n / 64.0 + 19.0))
    xd = D(x)
    S0, Q0, _ = ops.wilson_action_charge(xd, BETA)
    with switches(small=bool(resident)):
        yd = ops.local_update(xd, BETA, None, n_hb=0, n_or=10)
    S1, Q1, _ = ops.wilson_action_charge(yd, BETA)
    dS = np.abs(H(S1) - H(S0))
    print(f'B {B} L {L} resident {resident}: |dS| {dS.max():.3e}, tol {tol.min():.3e}, closest plaquette to pi {gap:.3e}')
    assert np.all(dS <= tol), (dS, tol)
    assert not torch.equal(yd, xd)
    assert gap > 1e-9, 'choose another field: a plaquette sits on the branch cut of the charge'
    assert float((Q1 - Q0).abs().max()) <= 1e-9


# ---------------------------------------------------------------- 5. the near-cancelling staple pair
@pytest.mark.parametrize('resident', [True, False], ids=['one-launch', 'class-kernels'])
def test_the_cancelling_staple_pair_gives_finite_links_in_range(resident):
    L = 8
    x = np.zeros((2, 2, L, L))
    x[:, 1, 3, 0::2] = math.pi                     # x0[2][j]: (a, b) = (pi, 0) for even j, (0, pi) for odd j: |A| = 1.2e-16
    x[1] += LC.uniform_links(1, L, 5, 1e-17)[0]
    r = LC.class_update(x, 0, 0, 'hb', BETA, LC.chain_seeds(2, 9), 0)
    assert r['kappa'].min() < 1e-15
    sd = S(LC.chain_seeds(2, 9))
    for kind in ('hb', 'or'):
        for classes in (1, 2, 4, 8, 15):
            with switches(small=bool(resident)):
                y = H(update(D(x), kind, sd, classes=classes, nsweep=3))
            assert np.all(np.isfinite(y)), (kind, classes)
            touched = y != x
            assert np.all(y[touched] >= -math.pi) and np.all(y[touched] < math.pi), (kind, classes)


# ---------------------------------------------------------------- 6. the exact loop table
@pytest.mark.parametrize('n_or', [0, 3])
def test_sampler_reproduces_the_exact_loop_table(n_or):
    """L = 8, beta = 2, 256 chains, 200 + 1000 compound sweeps of one heatbath and n_or overrelaxation sweeps, measured after every
    one; the error of an entry from the 256 chain means (plus the rounding bound of the table itself, which is all W(8, 8) = 1
    has).  Measured z-scores: DESIGN 4.13."""
    from fthmc_amd.utils import observables as O
    B, L, ntherm, nmeas = 256, 8, 200, 1000
    x = D(LC.uniform_links(B, L, 4242))
    seeds = S(LC.chain_seeds(B, 4243 + n_or))
    W = torch.empty(B, L, L, dtype=torch.float64, device='cuda')
    acc = torch.zeros_like(W)
    for k in range(ntherm + nmeas):
        ops.local_update(x, BETA, seeds, n_hb=1, n_or=n_or, sweep0=k, out=x)
        if k >= ntherm:
            ops.wilson_loops(x, L, L, out=W)
            acc += W
    chain = H(acc) / nmeas
    mean, se = chain.mean(axis=0), chain.std(axis=0, ddof=1) / math.sqrt(B)
    exact = np.array([[O.exact_wilson_loop(BETA, L, R, T) for T in range(1, L + 1)] for R in range(1, L + 1)])
    rnd = np.array([[WC.derived_bound(L, R, T, 1.0) for T in range(1, L + 1)] for R in range(1, L + 1)])
    z = (mean - exact) / np.maximum(se, 1e-300)
    with np.printoptions(precision=2, suppress=True, linewidth=150):
        print(f'n_or = {n_or}: plaquette {mean[0, 0]:.6f} +- {se[0, 0]:.6f}, exact {exact[0, 0]:.6f}; z-scores\n{np.where(se > 1e-12, z, 0.0)}')
    assert np.all(np.abs(mean - exact) <= 4.5 * se + rnd), float(np.abs(np.where(se > 1e-12, z, 0.0)).max())


# ---------------------------------------------------------------- 7. the drivers
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


def test_run_local_captured_equals_eager_and_reports_run_hmc_keys():
    from fthmc_amd.config import Param
    from fthmc_amd.local import run_local
    param = Param(beta=BETA, L=8, ntraj=7, nrun=2, nprint=0)
    x0 = D(LC.uniform_links(4, 8, 31))
    fa, ha = run_local(param, x0, n_overrelax=2, sweeps_per_traj=2, loops=(3, 4), loops_every=3, use_graph=True)
    fb, hb = run_local(param, x0, n_overrelax=2, sweeps_per_traj=2, loops=(3, 4), loops_every=3, use_graph=False)
    _hist_equal(ha, hb)
    for u, v in zip(fa, fb):
        assert torch.equal(u, v)
    assert set(ha[0]) == {'traj', 'dt', 'acc', 'plaq', 'q', 'dq', 'wloops'} and len(ha[0]['plaq']) == 7 and len(ha[0]['wloops']) == 3
    assert tuple(ha[0]['wloops'][0].shape) == (3, 4) and tuple(ha[0]['plaq'][0].shape) == (4,) and float(ha[0]['acc'][0].min()) == 1.0
    assert not torch.equal(fa[0], fa[1]) and ha[1]['traj'][0] == 8          # the second run goes on in the stream
    _, hc = run_local(param, x0, use_graph=True)
    assert 'wloops' not in hc[0] and 'dH' not in hc[0]
    # the last update's row is what the field gives
    S_, Q_, plaq_ = ops.wilson_action_charge(fa[1], BETA)
    assert torch.equal(plaq_.cpu(), ha[1]['plaq'][-1]) and torch.equal(Q_.cpu(), ha[1]['q'][-1])


def test_run_hmc_overrelax_zero_changes_nothing_and_two_sweeps_keep_the_plaquette():
    from fthmc_amd.config import Param
    from fthmc_amd.hmc import run_hmc
    from fthmc_amd.utils import observables as O
    param = Param(beta=BETA, L=8, ntraj=12, nrun=1, nprint=0, randinit=True)
    torch.manual_seed(5); fa, ha = run_hmc(param)
    torch.manual_seed(5); fb, hb = run_hmc(param, overrelax=0)
    _hist_equal(ha, hb)
    assert all(torch.equal(u, v) for u, v in zip(fa[0], fb[0]))
    torch.manual_seed(5); fc, hc = run_hmc(param, overrelax=2)
    assert hc[0].keys() == ha[0].keys() and not torch.equal(fc[0][-1], fa[0][-1])
    with pytest.raises(ValueError):
        run_hmc(param, overrelax=-1)
    param = Param(beta=BETA, L=8, ntraj=1100, nrun=1, nprint=0, randinit=True)
    torch.manual_seed(6); _, h = run_hmc(param, overrelax=2)
    plaq = np.array([float(p) for p in h[0]['plaq'][100:]])
    blocks = O.block_means(plaq, 20)
    mean, se = blocks.mean(), blocks.std(ddof=1) / math.sqrt(len(blocks))
    exact = O.exact_wilson_loop(BETA, 8, 1, 1)
    acc = float(np.mean([float(a) for a in h[0]['acc']]))
    print(f'run_hmc(overrelax=2): plaquette {mean:.5f} +- {se:.5f}, exact {exact:.5f}, z {(mean - exact) / se:+.2f}, acceptance {acc:.2f}')
    assert abs(mean - exact) <= 4.5 * se and acc > 0.5


def test_qed_helpers_and_the_torch_operator():
    from fthmc_amd.config import Param
    from fthmc_amd.utils import qed_helpers as qed
    import fthmc_amd.torch_ops  # noqa: F401
    param = Param(beta=BETA, L=8)
    x, seeds, _ = case(3, 8, 'hb')
    xd, sd = D(x), S(seeds)
    assert torch.equal(qed.heatbath(param, xd, sd), ops.local_update(xd, BETA, sd))
    assert torch.equal(qed.overrelax(param, xd, 2), ops.local_update(xd, BETA, None, n_hb=0, n_or=2))
    assert tuple(qed.heatbath(param, xd[0]).shape) == (2, 8, 8) and tuple(qed.overrelax(param, xd[0]).shape) == (2, 8, 8)
    y = torch.ops.fthmc_hip.local_update(xd, BETA, None, sd, 2, 1, 2, 4, 15)
    assert torch.equal(y, ops.local_update(xd, BETA, sd, n_hb=2, n_or=1, nsweep=2, sweep0=4))
    bb = torch.linspace(1.0, 3.0, 3, dtype=torch.float64, device='cuda')
    assert torch.equal(torch.ops.fthmc_hip.local_update(xd, 0.0, bb, sd), ops.local_update(xd, bb, sd))
    torch.library.opcheck(torch.ops.fthmc_hip.local_update.default, (xd, BETA, None, sd, 1, 1), test_utils=('test_schema', 'test_faketensor'))
    torch.library.opcheck(torch.ops.fthmc_hip.local_update.default, (xd, BETA, bb, None, 0, 2), test_utils=('test_schema', 'test_faketensor'))
    with pytest.raises(RuntimeError):
        torch.ops.fthmc_hip.local_update(xd, BETA, None, None, 1, 0)           # heatbath without seeds
