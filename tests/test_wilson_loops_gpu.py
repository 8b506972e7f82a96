"""GPU tests of the Wilson-loop observable (fthmc_amd/csrc/loops.hip): the device table against the longdouble oracle of
tests/wilson_loop_cases.py inside a derived error bound, consistency checks (plaquette, unit field, known answer, Polyakov
correlator, gauge invariance, determinism, batch mean, operator), the exact finite-volume expectation on plain-HMC and flowed
ensembles, and the drivers (captured loop against the eager one, loops_every, loops=None).

The tolerance of every comparison with the oracle is `wilson_loop_cases.derived_bound`, whose docstring derives it for the
arithmetic of loops.hip (compensated prefix sums: O(L) ulps); `tolerance()` asserts that it lies below the ceiling
2^-53 (2 pi L^2 + 8 (R + T) + 16) max(1, max|x| / pi).  A mis-indexed site moves an entry by about 1 / L^2 >= 6e-5."""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401

import wilson_loop_cases as WC

from gpu_support import D, H, module_defaults, ops

pytestmark = pytest.mark.gpu
_defaults = module_defaults()

# the shapes of the issue, the last lattice whose row lives in LDS and the first whose row lives in global scratch
SHAPES = WC.SHAPES + ((1, 1024, 1, 2), (1, 1028, 2, 3))


@functools.lru_cache(maxsize=None)
def case(shape):
    """(links, longdouble table, per-entry tolerance) of a shape: computed once, shared, never written"""
    B, L, Rmax, Tmax = shape
    x = WC.uniform_links(B, L, 1000 + 7 * L + Rmax)
    ref = WC.loops_ref(x, Rmax, Tmax)
    x.setflags(write=False); ref.setflags(write=False)
    return x, ref, WC.tolerance(L, Rmax, Tmax, WC.mu_of(x))


def check(W, ref, tol, what):
    err = np.abs(W.astype(np.longdouble) - ref).astype(np.float64)
    worst = float((err.reshape(-1, *tol.shape).max(axis=0) / tol).max())
    print(f'{what}: max |err| {err.max():.3e}, max |err| / tol {worst:.3f}')
    assert np.all(err <= tol), (what, float(err.max()), worst)


# ---------------------------------------------------------------- A. the device table against the oracle
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'B%d-L%d-R%d-T%d' % s)
def test_device_table_against_the_longdouble_oracle(shape):
    B, L, Rmax, Tmax = shape
    x, ref, tol = case(shape)
    W = ops.wilson_loops(D(x), Rmax, Tmax)
    assert tuple(W.shape) == (B, Rmax, Tmax)
    check(H(W), ref, tol, str(shape))


# ---------------------------------------------------------------- B. consistency
@pytest.mark.parametrize('shape', [(3, 8, 8, 8), (2, 20, 7, 20), (2, 64, 9, 64)], ids=lambda s: 'L%d' % s[1])
def test_plaquette_entry_unit_field_closed_loop_and_polyakov_column(shape):
    B, L, Rmax, Tmax = shape
    x, ref, tol = case(shape)
    xd = D(x)
    W = H(ops.wilson_loops(xd, L, L))
    plaq = H(ops.wilson_action_charge(xd, 1.7)[2])
    dp = float(np.abs(W[:, 0, 0] - plaq).max())
    print(f'L = {L}: |W(1,1) - plaq| = {dp:.3e}, bound {(L * L + 16) * WC.U:.3e}')
    assert dp <= (L * L + 16) * WC.U
    full = WC.tolerance(L, L, L, WC.mu_of(x))
    assert float(np.abs(W[:, L - 1, L - 1] - 1.0).max()) <= full[L - 1, L - 1]            # W(L, L) = 1
    pc = WC.polyakov_correlator_ref(x, L)                                              # the T = L column from the column phases
    assert np.all(np.abs(W[:, :, L - 1].astype(np.longdouble) - pc).astype(np.float64) <= full[None, :, L - 1])
    from fthmc_amd.utils import qed_helpers as qed
    assert torch.equal(qed.polyakov_correlator(xd), torch.from_numpy(W[:, :, L - 1]).cuda())
    assert torch.equal(qed.wilson_loops(xd[0], 3, 2), torch.from_numpy(W[:1, :3, :2]).cuda())
    one = H(ops.wilson_loops(torch.zeros_like(xd), L, L))
    assert np.all(one == 1.0)                                                          # x = 0: exactly 1 everywhere


@pytest.mark.parametrize('L,k', [(8, 1), (8, 3), (12, 1), (12, 3)])
def test_known_answer_field(L, k):
    x = WC.known_answer_field(L, k, B=2)
    W = H(ops.wilson_loops(D(x), L, L))
    tol = WC.tolerance(L, L, L, WC.mu_of(x))
    # the field's own rounding: 2 pi k j / L in doubles, R (and R) of them per side: R * 2 * 2^-53 * max|x| on top of the bound
    extra = np.arange(1, L + 1)[:, None] * 2 * WC.U * float(np.abs(x).max()) * np.ones((1, L))
    check(W, WC.loops_ref(x, L, L), tol, f'known answer L = {L}, k = {k} against the oracle')
    assert np.all(np.abs(W - WC.known_answer(L, k, L, L)[None]) <= (tol + extra)[None])


@pytest.mark.parametrize('shape', [(3, 8, 8, 8), (2, 12, 12, 5), (2, 64, 9, 64)], ids=lambda s: 'L%d' % s[1])
def test_gauge_invariance_at_amplitude_50(shape):
    B, L, Rmax, Tmax = shape
    x, ref, _ = case(shape)
    alpha = np.random.default_rng(L).uniform(-50, 50, (B, L, L))
    xg = WC.gauge_transform(x, alpha)
    tol = WC.tolerance(L, Rmax, Tmax, WC.mu_of(xg))                                    # at the transformed field's max|x|
    Wg = H(ops.wilson_loops(D(xg), Rmax, Tmax))
    check(Wg, WC.loops_ref(xg, Rmax, Tmax), tol, f'transformed field L = {L}')
    # against the untransformed table: the transformed links are rounded doubles of magnitude ~100, the loop of perimeter
    # 2 (R + T) sees their roundings
    per = 2 * (np.arange(1, Rmax + 1)[:, None] + np.arange(1, Tmax + 1)[None, :]) * WC.U * float(np.abs(xg).max())
    assert np.all(np.abs(Wg.astype(np.longdouble) - ref).astype(np.float64) <= (tol + per)[None])


def test_two_calls_bit_equal_batch_mean_in_index_order_and_operator():
    """Wmean: bit for bit the float64 sum of the chains' tables in index order, divided by B"""
    import fthmc_amd.torch_ops  # noqa: F401
    for shape in ((130, 16, 4, 4), (3, 8, 8, 8), (2, 64, 9, 64)):
        B, L, Rmax, Tmax = shape
        xd = D(case(shape)[0])
        mean = torch.empty(Rmax, Tmax, dtype=torch.float64, device='cuda')
        out = torch.empty(B, Rmax, Tmax, dtype=torch.float64, device='cuda')
        W1 = ops.wilson_loops(xd, Rmax, Tmax, out=out, mean_out=mean)
        assert W1.data_ptr() == out.data_ptr()
        W2 = ops.wilson_loops(xd, Rmax, Tmax)
        assert torch.equal(W1, W2)
        acc = np.zeros((Rmax, Tmax))
        for b in range(B):
            acc = acc + H(W1)[b]
        assert np.array_equal(H(mean), acc / B)
        assert torch.equal(torch.ops.fthmc_hip.wilson_loops(xd, Rmax, Tmax), W1)
    with pytest.raises(ValueError):
        ops.wilson_loops(xd, 65, 1)
    with pytest.raises((RuntimeError, ValueError)):
        torch.ops.fthmc_hip.wilson_loops(xd, 1, 0)


# ---------------------------------------------------------------- C, D. physics
def _judge(mean, se, beta, L, what):
    from fthmc_amd.utils import observables as O
    Rmax, Tmax = mean.shape
    V = L * L
    z = np.zeros_like(mean)
    for R in range(1, Rmax + 1):
        for T in range(1, Tmax + 1):
            z[R - 1, T - 1] = (mean[R - 1, T - 1] - O.exact_wilson_loop(beta, L, R, T)) / se[R - 1, T - 1] if R * T < V else 0.0
    print(f'{what}: (mean - exact) / se\n' + np.array2string(z, precision=2, suppress_small=True, max_line_width=200))
    assert float(np.abs(z).max()) <= 5.0, float(np.abs(z).max())
    for R in range(1, Rmax + 1):                                 # noise cannot pass: the next area's value is rejected
        for T in range(1, Tmax + 1):
            if R * T <= 6:
                other = O.exact_loop_of_area(beta, V, R * T + 1)
                assert abs(mean[R - 1, T - 1] - other) >= 5.0 * se[R - 1, T - 1], (R, T)
    return z


def test_plain_hmc_reproduces_the_exact_loops():
    """L = 8, beta = 2, 256 chains, tau = 1 in 10 steps, 300 + 1000 trajectories, the whole 8 x 8 table: per chain the mean over
    the trajectories, the standard error from the 256 independent chain means; every entry but (8, 8) within 5 se of the exact
    finite-volume value, every entry of area <= 6 at least 5 se away from the value of the next area."""
    L, beta, B, nstep = 8, 2.0, 256, 10
    torch.manual_seed(1234); torch.cuda.manual_seed(1234)
    x = (torch.rand(B, 2, L, L, dtype=torch.float64, device='cuda') * 2 - 1) * math.pi
    v, u = torch.empty_like(x), torch.empty(B, dtype=torch.float64, device='cuda')
    W = torch.empty(B, L, L, dtype=torch.float64, device='cuda')
    tot = torch.zeros_like(W)
    acc = 0.0
    for i in range(1300):
        v.normal_(); u.uniform_()
        r = ops.hmc_trajectory(x, v, u, beta, 1.0 / nstep, nstep)
        x = r['x_new']
        if i >= 300:
            tot += ops.wilson_loops(x, L, L, out=W)
            acc = acc + r['acc'].mean()
    chain = H(tot) / 1000.0
    print('acceptance', float(acc) / 1000.0)
    _judge(chain.mean(axis=0), chain.std(axis=0, ddof=1) / math.sqrt(B), beta, L, 'plain HMC')


def _flowed(L, beta, nl, B, nstep=10):
    from fthmc_amd import train as T
    from fthmc_amd.config import TrainConfig, lfConfig
    from fthmc_amd.ft_hmc import FieldTransformation
    cfg = TrainConfig(L=L, beta=beta, n_layers=nl, batch_size=B, print_freq=0)
    torch.manual_seed(11)
    model = T.get_model(cfg)
    return FieldTransformation(flow=model.layers, config=cfg, lfconfig=lfConfig(tau=1.0, nstep=nstep))


def test_flowed_hmc_reproduces_the_exact_loops_of_the_physical_field():
    """The same through FieldTransformation.run(batch=True, loops=(4, 4)) with a 2-layer default-init flow: the loops are of F(x).
    The history carries the BATCH-mean table of every trajectory, not the chains' own, so the standard error of the time mean
    comes from 50 block means of 20 trajectories each (utils.observables.loop_table; the autocorrelation at beta = 2 is a few
    trajectories) instead of from the 256 chain means."""
    from fthmc_amd.utils import observables as O
    L, beta, B = 8, 2.0, 256
    ft = _flowed(L, beta, 2, B)
    torch.manual_seed(77); torch.cuda.manual_seed(77)
    x0 = (torch.rand(B, 2, L, L, dtype=torch.float64, device='cuda') * 2 - 1) * math.pi
    ft.run(x0, nprint=0, num_trajs=300, batch=True)
    h = ft.run(ft.x_last, nprint=0, num_trajs=1000, batch=True, loops=(4, 4))
    assert len(h['wloops']) == 1000 and tuple(h['wloops'][0].shape) == (4, 4)
    print('acceptance', float(torch.stack(h['acc']).mean()))
    mean, se = O.loop_table(h['wloops'], n_block=50)
    _judge(mean, se, beta, L, 'ftHMC, 2 layers')
    # the history's plaquette is the same observable by another kernel
    assert abs(float(torch.stack(h['plaq']).mean()) - float(torch.stack(h['wloops'])[:, 0, 0].mean())) < 1e-12


# ---------------------------------------------------------------- E. drivers
PARENT_KEYS = {'traj', 'dt', 'acc', 'dh', 'exp_mdh', 'plaq', 'q', 'dq'}


def _seeded_run(ft, x0, n, **kw):
    torch.manual_seed(5); torch.cuda.manual_seed(5)
    return ft.run(x0.clone(), nprint=0, num_trajs=n, batch=True, **kw)


def _same(a, b, keys):
    for k in keys:
        assert len(a[k]) == len(b[k]), k
        for s, t in zip(a[k], b[k]):
            assert torch.equal(torch.as_tensor(s).cpu(), torch.as_tensor(t).cpu()), k


@pytest.mark.parametrize('L,nl,B', [(8, 2, 6), (32, 2, 4), (64, 2, 32)])
def test_captured_run_equals_the_eager_loop_and_loops_every(L, nl, B):
    """(64, 2, 32): two chain groups, as the headline shape -- the measurement flows ALL chains on the loop's stream, whose
    workspace the trajectory sized for one group"""
    n = 5
    assert (ops.default_groups(B, L) > 1) == (L == 64)
    x0 = (0.3 * (2 * torch.rand(B, 2, L, L, dtype=torch.float64, generator=torch.Generator().manual_seed(L)) - 1)).cuda()
    cap = _seeded_run(_flowed(L, 2.0, nl, B, 8), x0, n, loops=(3, 3))
    eag = _seeded_run(_flowed(L, 2.0, nl, B, 8), x0, n, loops=(3, 3), use_graph=False)
    assert set(cap.keys()) == PARENT_KEYS | {'wloops'} == set(eag.keys())
    _same(cap, eag, ('acc', 'dh', 'plaq', 'q', 'dq', 'wloops'))
    assert len(cap['wloops']) == n and tuple(cap['wloops'][0].shape) == (3, 3)
    # the table is that of F(x) of the accepted field: its (1, 1) entry is the history's plaquette, another kernel's sum
    for i in range(n):
        assert abs(float(cap['wloops'][i][0, 0]) - float(cap['plaq'][i].mean())) < 1e-13
    ft = _flowed(L, 2.0, nl, B, 8)
    ev2 = _seeded_run(ft, x0, n, loops=(3, 3), loops_every=2)
    assert len(ev2['wloops']) == 3
    _same(ev2, cap, ('acc', 'dh', 'plaq', 'q'))
    for i in range(3):
        assert torch.equal(ev2['wloops'][i].cpu(), cap['wloops'][2 * i].cpu())
    eg2 = _seeded_run(_flowed(L, 2.0, nl, B, 8), x0, n, loops=(3, 3), loops_every=2, use_graph=False)
    _same(ev2, eg2, ('acc', 'dh', 'plaq', 'q', 'wloops'))
    # a second run on the captured loop (its graphs are replayed from iteration 0 again)
    again = _seeded_run(ft, x0, n, loops=(3, 3), loops_every=2)
    _same(again, ev2, ('acc', 'dh', 'plaq', 'q', 'wloops'))


@pytest.mark.parametrize('L,nl,B', [(8, 2, 6), (32, 2, 4)])
def test_without_loops_the_history_is_the_parents(L, nl, B):
    """loops=None: the keys the driver had before `loops` existed and, on the same seeds, the bits of acc, dh, plaq, q of that
    code path -- the trajectory loop written out by hand on `_batch_hmc` with the carried state, as the driver ran it -- and of
    the run that measures loops besides."""
    n = 4
    x0 = (0.3 * (2 * torch.rand(B, 2, L, L, dtype=torch.float64, generator=torch.Generator().manual_seed(L)) - 1)).cuda()
    for use_graph in (True, False):
        h = _seeded_run(_flowed(L, 2.0, nl, B, 8), x0, n, use_graph=use_graph)
        assert set(h.keys()) == PARENT_KEYS
        ft = _flowed(L, 2.0, nl, B, 8)
        torch.manual_seed(5); torch.cuda.manual_seed(5)
        x = x0.clone()
        for i in range(n):
            x, m = ft._batch_hmc(x, step=i)
            p_, q_ = ft._last_obs
            for k, t in (('acc', m['acc']), ('dh', m['dh']), ('plaq', p_), ('q', q_)):
                assert torch.equal(h[k][i].cpu(), t.cpu()), (k, i, use_graph)
        with_loops = _seeded_run(_flowed(L, 2.0, nl, B, 8), x0, n, use_graph=use_graph, loops=(2, 3))
        _same(h, with_loops, ('acc', 'dh', 'plaq', 'q', 'dq'))


def test_run_hmc_gains_the_loop_history():
    from fthmc_amd.config import Param
    from fthmc_amd.hmc import run_hmc
    from fthmc_amd.utils import observables as O
    p = Param(L=8, beta=2.0, tau=1.0, nstep=10, ntraj=6, nrun=1, nprint=0)
    torch.manual_seed(3); torch.cuda.manual_seed(3)
    fields, hist = run_hmc(p, loops=(4, 5), loops_every=2)
    h = hist[0]
    assert len(h['wloops']) == 3 and tuple(h['wloops'][0].shape) == (4, 5)
    for k, i in enumerate((0, 2, 4)):
        x = fields[0][i].reshape(-1, 2, 8, 8)
        assert x.shape[0] == 1 and torch.equal(ops.wilson_loops(x, 4, 5)[0], h['wloops'][k])
        assert abs(float(h['wloops'][k][0, 0]) - float(torch.as_tensor(h['plaq'][i]).mean())) < 1e-13
    torch.manual_seed(3); torch.cuda.manual_seed(3)
    _, hist0 = run_hmc(p)
    assert 'wloops' not in hist0[0] and set(hist0[0].keys()) == set(h.keys()) - {'wloops'}
    for k in ('acc', 'dH', 'plaq', 'q'):
        for a, b in zip(hist0[0][k], h[k]):
            assert torch.equal(torch.as_tensor(a).cpu(), torch.as_tensor(b).cpu()), k
    mean, err = O.loop_table(h['wloops'], n_block=3)
    assert mean.shape == (4, 5) and err.shape == (4, 5)
