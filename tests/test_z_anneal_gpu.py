"""GPU tests of annealed importance sampling (fthmc_anneal: fthmc_amd/csrc/local.hip).  Deterministic: the fields
against the chain of ops.local_update calls the header names, bit for bit, on both paths; the trace and the work inside the bounds the
twin derives (tests/anneal_cases.py) from the device's own fields; the two paths, the cut, the batch, the aliases, n_step = 0 and a
captured replay under a new schedule, bit for bit; the flow start.  Statistical: one ramp at L = 16 against the exact partition
function, charge moment and plaquette."""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401

import anneal_cases as AC

from gpu_support import D, H, capture, module_defaults, ops, switches

pytestmark = pytest.mark.gpu
_defaults = module_defaults()

BETAS, N, B = AC.BETAS, AC.N_STEP, AC.B


def S(seeds):
    return torch.from_numpy(np.array(seeds, dtype=np.int64)).cuda()


def paths(L):
    return (1, 2) if L <= AC.LU_MAXL else (2,)


def ids(v):
    return 'x'.join(str(c) for c in v) if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def reference(L, counts):
    """Of a case, computed once and never written: the inputs on the device, the fields x_0 .. x_n of the chain of ops.local_update
    calls, the twin's sums C_k, dC_k of THOSE fields and the work and its bound from them."""
    n_hb, n_or, nsweep = counts
    x, seeds, w0 = AC.fields(L)
    xd, sd, wd = D(x), (S(seeds) if n_hb else None), D(w0)
    chain = [xd]
    for k in range(N):
        chain.append(ops.local_update(chain[-1], BETAS[k + 1], sd, n_hb=n_hb, n_or=n_or, nsweep=nsweep,
                                      sweep0=AC.SWEEP0 + k * nsweep * n_hb))
    sums = [AC.cos_sum(H(f)) for f in chain]
    C, dC = [s[0] for s in sums], [s[1] for s in sums]
    W, wb = AC.work_steps(BETAS, C, dC, w0)
    kw = dict(n_hb=n_hb, n_or=n_or, nsweep=nsweep, sweep0=AC.SWEEP0)
    return dict(x=xd, seeds=sd, work=wd, chain=chain, C=np.stack(C, 1), dC=np.stack(dC, 1), W=W, wb=wb, kw=kw,
                bt=torch.tensor(BETAS, dtype=torch.float64, device='cuda'))


def run(r, path, **kw):
    a = dict(r['kw']); a.update(work=r['work'], trace=True, path=path); a.update(kw)
    return ops.anneal(a.pop('x', r['x']), a.pop('betas', r['bt']), r['seeds'], **a)


# ---------------------------------------------------------------- 1. the fields are the chain of local_update calls
@pytest.mark.parametrize('L,counts', AC.cases(), ids=ids)
def test_fields_equal_the_chain_of_local_update_calls_bit_for_bit(L, counts):
    r = reference(L, counts)
    assert not torch.equal(r['chain'][1], r['chain'][0]) and not torch.equal(r['chain'][3], r['chain'][2])
    for path in paths(L):
        got = run(r, path)
        assert torch.equal(got['x'], r['chain'][N]), f'path {path}'
        # ... and depend on nothing but the schedule and the seeds: no work, no trace, the path left to the library
        bare = ops.anneal(r['x'], list(BETAS), r['seeds'], **r['kw'])
        assert bare['trace'] is None and torch.equal(bare['x'], r['chain'][N])
        assert torch.equal(bare['work'], run(r, path, work=None)['work'])
    assert torch.equal(r['x'], D(AC.fields(L)[0])), 'the input was written'


# ---------------------------------------------------------------- 2. the trace and the work inside the twin's bounds
@pytest.mark.parametrize('L,counts', AC.cases(), ids=ids)
def test_trace_and_work_sit_inside_the_derived_bounds(L, counts):
    r = reference(L, counts)
    for path in paths(L):
        got = run(r, path)
        tr, w = H(got['trace']), H(got['work'])
        assert tr.shape == (B, N + 1)
        et = np.abs((tr - r['C']).astype(np.float64)) / r['dC']
        ew = np.abs((w - r['W']).astype(np.float64)) / r['wb']
        print(f'L {L} counts {counts} path {path}: trace err / bound {et.max():.3f} (bound {r["dC"].max():.2e}), work err / bound '
              f'{ew.max():.3f} (bound {r["wb"].max():.2e}), |W| {np.abs(w).max():.1f}')
        assert et.max() <= 1.0 and ew.max() <= 1.0
        assert r['dC'].max() < 1e-15 * L * L * 40 and r['wb'].max() < 1e-14 * L * L * 40      # the bounds themselves say something
        # the steps did work: a rising, a zero and a falling one
        assert np.all(np.abs(w - AC.fields(L)[2]) > 1e-3)
    # a wrong sign, a wrong beta pair or a missed step is far outside: the smallest term of the work against the bound
    terms = np.abs(np.diff(BETAS)[None, :] * r['C'][:, :N].astype(np.float64))
    assert terms[:, [0, 2]].min() > 1e6 * r['wb'].max() and np.all(terms[:, 1] == 0)


# ---------------------------------------------------------------- 3. the two paths
@pytest.mark.parametrize('L,counts', [c for c in AC.cases() if c[0] <= AC.LU_MAXL], ids=ids)
def test_both_paths_give_the_same_bits_in_every_output(L, counts):
    r = reference(L, counts)
    a, b, c = run(r, 1), run(r, 2), run(r, 0)
    for k in ('x', 'work', 'trace'):
        assert torch.equal(a[k], b[k]), f'{k}: the one-launch kernel and the sequenced path differ'
        assert torch.equal(a[k], c[k]), k
    with switches(small=False):
        d = run(r, 0)
    assert all(torch.equal(a[k], d[k]) for k in ('x', 'work', 'trace'))


# ---------------------------------------------------------------- 4. the contracts, bit for bit
@pytest.mark.parametrize('L,counts', [(4, (1, 2, 1)), (12, (2, 1, 2)), (64, (2, 1, 2)), (68, (2, 1, 2))], ids=ids)
def test_cut_batch_aliases_and_zero_steps(L, counts):
    r = reference(L, counts)
    n_hb, n_or, nsweep = counts
    for path in paths(L):
        full = run(r, path)
        for m in (1, 2):
            a = run(r, path, betas=r['bt'][:m + 1])
            b = run(r, path, x=a['x'], betas=r['bt'][m:], work=a['work'], sweep0=AC.SWEEP0 + m * nsweep * n_hb)
            assert torch.equal(b['x'], full['x']) and torch.equal(b['work'], full['work']), f'path {path}, cut at {m}'
            assert torch.equal(torch.cat([a['trace'][:, :m], b['trace']], dim=1), full['trace']), f'path {path}, cut at {m}'
            assert torch.equal(a['trace'][:, m], b['trace'][:, 0])
        for c in range(B):
            one = ops.anneal(r['x'][c:c + 1].contiguous(), r['bt'], None if r['seeds'] is None else r['seeds'][c:c + 1].contiguous(),
                             work=r['work'][c:c + 1].contiguous(), trace=True, path=path, **r['kw'])
            assert all(torch.equal(one[k][0], full[k][c]) for k in ('x', 'work', 'trace')), f'path {path}, chain {c}'
        # in place: x_out = x and work_out = work_in
        z, w = r['x'].clone(), r['work'].clone()
        got = run(r, path, x=z, work=w, out={'x': z, 'work': w})
        assert got['x'].data_ptr() == z.data_ptr() and got['work'].data_ptr() == w.data_ptr()
        assert all(torch.equal(got[k], full[k]) for k in ('x', 'work', 'trace'))
        # n_step = 0: the field and the work are copied, C_0 is written
        zero = run(r, path, betas=r['bt'][:1])
        assert torch.equal(zero['x'], r['x']) and torch.equal(zero['work'], r['work']) and torch.equal(zero['trace'][:, 0], full['trace'][:, 0])
        assert tuple(zero['trace'].shape) == (B, 1)
        none = run(r, path, betas=r['bt'][:1], work=None, trace=False)
        assert torch.equal(none['x'], r['x']) and float(none['work'].abs().max()) == 0.0 and none['trace'] is None
    assert torch.equal(r['x'], D(AC.fields(L)[0])) and torch.equal(r['work'], D(AC.fields(L)[2])), 'an input was written'


@pytest.mark.parametrize('path', [1, 2])
def test_a_captured_replay_follows_the_schedule_the_tensor_holds(path):
    r = reference(8, (1, 2, 1))
    other = torch.tensor([3.0, 0.25, 1.0, 1.0], dtype=torch.float64, device='cuda')
    want_a, want_b = run(r, path), run(r, path, betas=other)
    assert not torch.equal(want_a['x'], want_b['x']) and not torch.equal(want_a['work'], want_b['work'])
    bt = r['bt'].clone()
    out = {'x': torch.empty_like(r['x']), 'work': torch.empty_like(r['work'])}
    tr = torch.empty(B, N + 1, dtype=torch.float64, device='cuda')
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        run(r, path, betas=bt, out=out, trace=tr)                      # once eagerly on this stream
        stream.synchronize()
        g = torch.cuda.CUDAGraph()
        with capture(g, stream):
            run(r, path, betas=bt, out=out, trace=tr)
        for want, sched in ((want_a, r['bt']), (want_b, other), (want_a, r['bt'])):
            bt.copy_(sched)
            out['x'].zero_(); out['work'].zero_(); tr.zero_()
            g.replay()
            stream.synchronize()
            assert torch.equal(out['x'], want['x']) and torch.equal(out['work'], want['work']) and torch.equal(tr, want['trace'])
    torch.cuda.current_stream().wait_stream(stream)


# ---------------------------------------------------------------- 5. the flow start
def test_flow_start_carries_the_proposal_density_as_work():
    from fthmc_amd import train as T
    from fthmc_amd.anneal import run_annealed
    from fthmc_amd.config import Param, TrainConfig
    from fthmc_amd.utils.layers import flow_weights
    L, beta, nb, nl = 8, 2.0, 5, 2
    torch.manual_seed(11)
    model = T.get_model(TrainConfig(L=L, beta=beta, n_layers=nl, batch_size=nb, print_freq=0))
    with torch.no_grad():
        for p in model.layers.parameters():
            p.add_(0.05 * torch.randn_like(p))
    param = Param(beta=beta, L=L, ntraj=nb, nrun=2, nprint=0, seed=99)
    fields, hist = run_annealed(param, 0, beta0=beta, model=model.layers)
    w = flow_weights(model.layers, torch.device('cuda'))
    for n in range(2):
        seeds = ops.chain_seeds(param.seed, 0, nb, n, device='cuda')
        z = ops.random_uniform(seeds, (nb, 2, L, L), -math.pi, math.pi)
        x, logdet = ops.flow_forward(z, w, nl)
        assert torch.equal(fields[n], x)
        _, Q, plaq = ops.wilson_action_charge(x, beta)
        want = -beta * (H(plaq).astype(np.longdouble) * (L * L)) - H(logdet).astype(np.longdouble)
        got = hist[n]['work'].numpy()
        # the right side to its rounding: plaq V is C within (V + 8) u V + V 40 u (a sum of V cosines in whatever order, each 40 u
        # with its angle |P| <= 4 pi of three roundings, a division and a product), C of the work likewise; the products and the
        # difference one rounding each
        u, V = 2.0 ** -53, L * L
        tol = 2 * beta * ((V + 8) * u * V + 40 * V * u) + 4 * u * (np.abs(got) + np.abs(H(logdet)))
        err = np.abs((got - want).astype(np.float64))
        print(f'run {n}: work {got}, |err| max {err.max():.2e}, tol min {tol.min():.2e}, logdet {H(logdet)}')
        assert np.all(err <= tol) and float(np.abs(H(logdet)).min()) > 1e-6
        assert torch.equal(hist[n]['q'], Q.cpu()) and torch.equal(hist[n]['plaq'], plaq.cpu())
        assert abs(hist[n]['logZ'] - float(np.log(np.mean(np.exp(-got))))) < 1e-9
    assert not torch.equal(fields[0], fields[1])


def test_run_annealed_cut_into_calls_equals_one_call_and_the_plain_start_is_uniform():
    from fthmc_amd.anneal import beta_schedule, run_annealed
    from fthmc_amd.config import Param
    param = Param(beta=3.0, L=8, ntraj=6, nrun=2, nprint=0, seed=5)
    fa, ha = run_annealed(param, 37, n_overrelax=1, sweeps_per_step=2, steps_per_call=8)
    fb, hb = run_annealed(param, 37, n_overrelax=1, sweeps_per_step=2, steps_per_call=64)
    seeds = ops.chain_seeds(5, 0, 6, 1, device='cuda')
    x0 = ops.random_uniform(seeds, (6, 2, 8, 8), -math.pi, math.pi)
    one = ops.anneal(x0, beta_schedule(0.0, 3.0, 37).tolist(), seeds, n_hb=1, n_or=1, nsweep=2)
    for n in range(2):
        assert torch.equal(fa[n], fb[n]) and torch.equal(ha[n]['work'], hb[n]['work'])
        assert set(ha[n]) >= {'work', 'plaq', 'q', 'ess', 'logZ', 'logZ_err'} and tuple(ha[n]['work'].shape) == (6,)
        assert 1.0 <= ha[n]['ess'] <= 6.0 and math.isfinite(ha[n]['logZ']) and math.isfinite(ha[n]['logZ_err'])
    assert torch.equal(fa[1], one['x']) and torch.equal(ha[1]['work'], one['work'].cpu())
    assert not torch.equal(fa[0], fa[1])
    with pytest.raises(ValueError):
        run_annealed(param, 8, beta0=1.0)                                # uniform links are no sample at beta0 = 1
    with pytest.raises(ValueError):
        ops.anneal(x0, [0.0, -1.0], seeds)
    with pytest.raises(ValueError):
        ops.anneal(x0, [0.0, 1.0], seeds, n_hb=0, n_or=0)


# ---------------------------------------------------------------- the statistics
def test_annealed_ensemble_reproduces_the_exact_partition_function_charge_and_plaquette():
    """L = 16, beta 0 -> 6, quadratic, 2048 steps, 1024 chains, fixed seed: ESS / B >= 0.2 (the numpy twin gives 0.42 to 0.54 at
    B = 256), log Z within 5 jackknife errors of the exact value (1077.30; one wrong work term late in the ramp moves it by about 1),
    the reweighted <Q^2> and plaquette within 5 errors of theirs.  The UNWEIGHTED <Q^2> is printed beside them: about 1.33 against
    1.19 exact -- the weights do work.  Measured z-scores: DESIGN 4.17."""
    from fthmc_amd.anneal import run_annealed
    from fthmc_amd.config import Param
    from fthmc_amd.utils import observables as O
    L, beta, n_step, nb = 16, 6.0, 2048, 1024
    param = Param(beta=beta, L=L, ntraj=nb, nrun=1, nprint=0, seed=20260101)
    _, hist = run_annealed(param, n_step)
    h = hist[0]
    work, q, plaq = h['work'].numpy(), h['q'].numpy(), h['plaq'].numpy()
    ess = h['ess'] / nb
    exact_z = O.exact_log_partition(beta, L)
    z_logz = (h['logZ'] - exact_z) / h['logZ_err']
    q2, q2_err = O.reweighted_mean(q * q, -work)
    q2_exact = O.exact_charge_moment(beta, L)
    pl, pl_err = O.reweighted_mean(plaq, -work)
    pl_exact = O.exact_loop_of_area(beta, L * L, 1)
    print(f'ESS / B {ess:.3f}; log Z {h["logZ"]:.4f} +- {h["logZ_err"]:.4f}, exact {exact_z:.4f}, z {z_logz:+.2f}; <Q^2> {q2:.4f} +- '
          f'{q2_err:.4f}, exact {q2_exact:.4f}, z {(q2 - q2_exact) / q2_err:+.2f}, unweighted {float(np.mean(q * q)):.4f}; plaquette '
          f'{pl:.6f} +- {pl_err:.6f}, exact {pl_exact:.6f}, z {(pl - pl_exact) / pl_err:+.2f}; {h["dt"]:.2f} s')
    assert np.all(np.abs(q - np.rint(q)) < 1e-6)
    assert ess >= 0.2
    assert abs(h['logZ'] - exact_z) < 5 * h['logZ_err']
    assert abs(q2 - q2_exact) < 5 * q2_err
    assert abs(pl - pl_exact) < 5 * pl_err
