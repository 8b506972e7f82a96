"""CPU checks behind tests/test_batch_kernels_gpu.py: tests/golden/batch_kernels.npz regenerates bit for bit, the float64 twins of
the kernels (tests/batch_kernel_cases.py) stay inside the derived bounds on every case, the conditions the GPU tests rely on hold on
the references alone, and every named mutant of a twin leaves a bound or breaks an exact assertion on at least one case of its
family -- a bound that lets a mutant through is too loose."""
import math

import numpy as np
import pytest

from conftest import GOLDEN, load_golden  # noqa: F401

import batch_kernel_cases as C
import tempering_cases as TC

U = C.U


@pytest.fixture(scope='module')
def G():
    return load_golden('batch_kernels')


def test_fixture_regenerates_bit_for_bit(G):
    import os
    import sys
    sys.path.insert(0, GOLDEN)
    import make_golden_batch_kernels as M     # mpmath is a plain import there: a machine without it fails here, it does not skip
    new = M.generate()
    assert sorted(new) == sorted(G)
    for k in sorted(G):
        a, b = np.asarray(new[k]), G[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    assert os.path.getsize(os.path.join(GOLDEN, 'batch_kernels.npz')) < 1000000


# ---------------------------------------------------------------- 1. train metrics
def tm_errors(G, B, fam, mutant=None):
    d = C.tm_inputs(B, fam)
    loss_ref, ess_ref = C.tm_reference_of(G, B, fam)
    loss, ess = C.train_metrics_twin(d['logq'], d['logp'], C.TM_F, mutant)
    bl, be = C.tm_bounds(d['logq'], d['logp'], C.TM_F, loss_ref, ess_ref)
    return C.frac(abs(loss - loss_ref), bl), C.frac(abs(ess / ess_ref - 1.0), be)


def test_train_metrics_twin_inside_its_bounds(G):
    worst = [0.0, 0.0]
    for B, fam in C.tm_cases():
        fl, fe = tm_errors(G, B, fam)
        assert fl <= 1.0 and fe <= 1.0, (B, fam, fl, fe)
        worst = [max(worst[0], fl), max(worst[1], fe)]
    print('train_metrics twin: worst loss, ess error as a fraction of the bound', worst)


def test_train_metrics_references_are_what_the_families_say(G):
    for B, fam in C.tm_cases():
        loss_ref, ess_ref = C.tm_reference_of(G, B, fam)
        d = C.tm_inputs(B, fam)
        lw = d['logp'] - d['logq']
        assert 1.0 / B * (1 - 1e-12) <= ess_ref <= 1.0, (B, fam)
        if fam == 'equal':
            assert ess_ref == 1.0 and loss_ref == C.TM_F * -700.0
        if fam == 'wide' and B >= 63:
            w = np.exp(lw - lw.max())
            assert ess_ref < 4.0 / B and np.sum(w < 1e-30) > B // 2 and np.sum(w == 0.0) >= 1      # a few weights carry the sum
        if fam == 'far':
            assert lw.min() > 9900 > 710                               # exp(logw) itself overflows
        if fam.startswith('max_') and B > 1:
            assert abs(ess_ref * B - 1.0) <= 4 * U                       # one weight carries everything
            assert np.sort(lw)[-1] - np.sort(lw)[-2] > 1400


# ---------------------------------------------------------------- 2. run statistics
def st_check(G, B, mutant=None):
    """-> (exact assertions hold, worst fraction of the float bounds)"""
    inp = C.st_inputs(B)
    ref = G['st'][C.B_LIST.index(B)]
    vec, qold = C.stats_twin(inp, mutant)
    exact = np.array_equal(vec[:, list(C.ST_INT_COLS)], C.st_exact_ints(inp).astype(np.float64)) and \
        np.array_equal(qold.view(np.int64), inp['Q'].view(np.int64))
    return exact, C.frac(np.abs(vec[:, list(C.ST_FLOAT_COLS)] - ref), C.st_bounds(inp, ref))


def test_stats_twin_inside_its_bounds(G):
    worst = 0.0
    for B in C.B_LIST:
        exact, f = st_check(G, B)
        assert exact and f <= 1.0, (B, exact, f)
        worst = max(worst, f)
    print('stats_accumulate twin: worst float-column error as a fraction of the bound', worst)


def test_stats_inputs_carry_their_planted_values():
    for B in C.B_LIST:
        dH = C.st_inputs(B)['dH']
        assert dH[0, B - 1] == (800.0 if B >= 3 else 0.0) or B < 3
        if B >= 3:
            assert list(dH[0, B - 3:]) == [0.0, -30.0, 800.0] and list(dH[2, :3]) == [0.0, -30.0, 800.0]
        if B > 258:
            assert list(dH[1, 256:259]) == [0.0, -30.0, 800.0]
        if B == 257:
            assert dH[1, 256] == 0.0
    assert math.exp(-800.0) == 0.0


# ---------------------------------------------------------------- 3. Adam
def adam_check(G, mode, k, mutant=None):
    """twin step k + 1 of a mode from the stored state -> fractions (p, m, v) of the bounds over the sampled elements"""
    wd, dec = C.AD_MODES[mode]
    g = C.adam_master()['g'][G['adam_idx']]
    pre, ref = C.adam_chain(G, mode, k)
    got = C.adam_twin(pre[0], g, pre[1], pre[2], float(k), C.AD_LR[k], wd, dec, mutant)
    bnd = C.adam_bounds(pre[0], g, pre[1], pre[2], float(k), C.AD_LR[k], wd, dec, ref)
    return tuple(C.frac(np.abs(a - r), b) for a, r, b in zip(got, ref, bnd))


def test_adam_twin_inside_its_bounds(G):
    worst = np.zeros(3)
    for mode in range(len(C.AD_MODES)):
        for k in range(C.AD_STEPS):
            f = adam_check(G, mode, k)
            assert max(f) <= 1.0, (mode, k, f)
            worst = np.maximum(worst, f)
    print('adam twin: worst p, m, v error as a fraction of the bound', worst.tolist())


def test_adam_inputs_and_references(G):
    A, idx = C.adam_master(), G['adam_idx']
    for k in ('adam_p', 'adam_m', 'adam_v'):
        assert np.all(np.isfinite(G[k])), k
    assert np.all(G['adam_v'] >= 0.0)
    for n in C.AD_N:                                            # every size sees edge values; the large ones below their end too
        g, p = A['g'][:n], A['p'][:n]
        if n >= 255:
            for e in C.G_EDGES:
                assert np.sum((g == e) & (np.signbit(g) == np.signbit(e))) >= 2, (n, e)
            for e in C.P_EDGES:
                assert np.sum(p == e) >= 2, (n, e)
            assert np.abs(g[n - 13:n]).max() == 1e150
    assert np.all(np.isin(np.arange(C.AD_FULL), idx)) and np.all(np.isin(A['zero_g'], idx))
    for n in C.AD_N:
        if n > C.AD_FULL:
            assert np.all(np.isin(np.arange(n - 300, n), idx)) and np.sum(idx < n) >= C.AD_FULL + 300 + 1000
    # g = +-0 with m = 0: the exact step leaves p where it is in the mode without decay, at every step
    z = np.nonzero(np.isin(idx, A['zero_g']))[0]
    for k in range(C.AD_STEPS):
        assert np.array_equal(G['adam_p'][0, k][z], A['p'][idx][z]) and np.all(G['adam_m'][0, k][z] == 0.0)


# ---------------------------------------------------------------- 4. kinetic energy, action and charge
def test_kinetic_and_action_twins_inside_their_bounds(G):
    worst = {'K': 0.0, 'S': 0.0, 'plaq': 0.0, 'Q': 0.0}
    for li, L in enumerate(C.KA_L):
        v = C.ka_momenta(L)
        f = C.frac(np.abs(C.kinetic_twin(v) - G['kin'][li]), C.kinetic_bound(v, G['kin'][li]))
        assert f <= 1.0, (L, f)
        worst['K'] = max(worst['K'], f)
        for si, kind in enumerate(C.KA_SETS):
            x = C.ka_links(L, kind)
            S, Q, plaq = C.action_twin(x)
            bS, bp = C.action_bounds(x, G['act_S'][li, si], G['act_plaq'][li, si])
            fs = (C.frac(np.abs(S - G['act_S'][li, si]), bS), C.frac(np.abs(plaq - G['act_plaq'][li, si]), bp),
                  C.frac(np.abs(Q - G['act_Q'][li, si]), C.Q_TOL))
            assert max(fs) <= 1.0, (L, kind, fs)
            for k, t in zip(('S', 'plaq', 'Q'), fs):
                worst[k] = max(worst[k], t)
    print('kinetic / action twins: worst error as a fraction of the bound', worst)


def test_action_conditions_hold_on_the_reference(G):
    assert np.all(G['act_margin'] >= C.PI_MARGIN), G['act_margin'].min()
    assert np.all(G['act_Q'][:, C.KA_SETS.index('flux3')] == C.FLUX_K)
    # the shapes sit on both sides of each block-size threshold
    assert [C.nt_kinetic(L) for L in C.KA_L] == [256, 256, 512, 512, 512, 1024]
    assert [C.nt_action(L) for L in C.KA_L] == [256, 256, 512, 512, 512, 1024]
    assert 2 * 28 * 28 < 2048 <= 2 * 32 * 32 and 2 * 60 * 60 < 8192 <= 2 * 64 * 64


def test_kinetic_bound_would_see_a_lost_wave_or_pass(G):
    """the same mutants on the per-chain sums: the last wave's partial dropped, the loop stopped after its first pass"""
    for li, L in enumerate(C.KA_L):
        v = C.ka_momenta(L).reshape(C.KA_B, -1)
        nt = C.nt_kinetic(L)
        b = C.kinetic_bound(C.ka_momenta(L), G['kin'][li])
        lost = np.array([C.block_sum(C.strided_partials(t * t, nt), drop_wave=nt // 64 - 1) for t in v])
        if 2 * L * L > nt - 64:
            assert np.all(np.abs(lost - G['kin'][li]) > b), L
        if 2 * L * L > nt:
            first = np.array([C.block_sum(C.strided_partials(t * t, nt, passes=1)) for t in v])
            assert np.all(np.abs(first - G['kin'][li]) > b), L


# ---------------------------------------------------------------- 5. exchange
def swap_cases():
    for K, M in C.SWAP_SHAPES:
        yield K, M, C.swap_inputs(K, M, 2000 + 10 * K + M)
    for K in C.LADDER_K:
        betas, bb, rung, chain_of = C.ladder_init_twin(C.ladder_betas(K), C.LADDER_M)
        rng = np.random.default_rng(9400 + K)
        yield K, C.LADDER_M, (betas, bb, rung, chain_of, rng.normal(0.0, 40.0, C.LADDER_M * K), rng.uniform(0.0, 1.0, (C.LADDER_M, K - 1)))


def test_swap_conditions_hold_on_the_numpy_round():
    for K, M, (betas, bb, rung, chain_of, Cs, u) in swap_cases():
        TC.check_ladders(betas, bb, rung, chain_of)
        moved = 0
        for parity in (0, 1):
            nb, nr, nc, acc, d, e = TC.swap_round(betas, Cs, u, bb, rung, chain_of, parity)
            tried = acc >= 0
            assert np.all(np.abs(u[tried] - e[tried]) > 1e-12 * e[tried]), (K, M, parity)
            assert M * (K - 1) > 256 or K in C.LADDER_K
            moved += int((acc == 1).sum())
            assert int((acc == 0).sum()) > 0 or K == 2
            if (K, M) in C.SWAP_SHAPES:
                eq, zero = C.swap_edge_ladders(K, M)
                for m in eq:
                    if parity < K - 1:
                        assert acc[m, parity] == 1.0 and d[m, parity] == 0.0 and u[m, parity] in (0.999, 0.0)
                for m in zero:
                    if (K - 2) % 2 == parity:
                        assert acc[m, K - 2] == 1.0 and u[m, K - 2] == 0.0
        assert moved > 0


def test_ladder_init_twin_is_the_plain_definition():
    for K in C.LADDER_K:
        betas = C.ladder_betas(K)
        dev, bb, rung, chain_of = C.ladder_init_twin(betas, C.LADDER_M)
        assert np.array_equal(dev, betas) and np.array_equal(bb, np.tile(betas, C.LADDER_M))
        assert np.array_equal(rung, np.tile(np.arange(K), C.LADDER_M)) and np.array_equal(chain_of, rung)
        assert np.all(np.diff(betas) > 0)


# ---------------------------------------------------------------- the tests can fail: every mutant is caught
def test_every_mutant_is_caught(G):
    caught = {}
    for mu in C.TM_MUTANTS:
        hits = []
        for B, fam in C.tm_cases():
            fl, fe = tm_errors(G, B, fam, mu)
            if not (fl <= 1.0 and fe <= 1.0):
                hits.append(f'B={B} {fam}')
        caught['train_metrics:' + mu] = hits
    for mu in C.ST_MUTANTS:
        hits = []
        for B in C.B_LIST:
            exact, f = st_check(G, B, mu)
            if not (exact and f <= 1.0):
                hits.append(f'B={B}')
        caught['stats:' + mu] = hits
    for mu in C.AD_MUTANTS:
        hits = []
        for mode in range(len(C.AD_MODES)):
            for k in range(C.AD_STEPS):
                if not max(adam_check(G, mode, k, mu)) <= 1.0:
                    hits.append(f'mode={mode} step={k + 1}')
        caught['adam:' + mu] = hits
    hits = []
    for K in C.LADDER_K:
        betas = C.ladder_betas(K)
        good, bad = C.ladder_init_twin(betas, C.LADDER_M), C.ladder_init_twin(betas, C.LADDER_M, 'chunk2_at_0')
        assert np.array_equal(good[0], betas)
        if not (np.array_equal(bad[0].view(np.int64), betas.view(np.int64)) and np.array_equal(bad[1].view(np.int64), good[1].view(np.int64))):
            hits.append(f'K={K}')
    caught['ladder:chunk2_at_0'] = hits
    for k, hits in caught.items():
        print(f'{k}: caught by {len(hits)} cases, first {hits[:3]}')
    assert all(caught.values()), [k for k, h in caught.items() if not h]
    # each where its family says: the second pass and wave 3 at the sizes that have them, the maximum behind the first pass
    assert caught['train_metrics:drop_ge256'][0].startswith('B=257') and caught['stats:drop_ge256'][0] == 'B=257'
    assert caught['train_metrics:drop_wave3'][0].startswith('B=255') and caught['stats:drop_wave3'][0] == 'B=255'
    assert set(caught['train_metrics:max_first_pass']) >= {'B=257 max_256', 'B=511 max_256', 'B=1000 max_256', 'B=1000 max_last'}
    assert len(caught['train_metrics:ess_no_invB']) >= len(C.tm_cases()) - len(C.tm_families(1))
    assert caught['stats:qold_stuck_ge256'] == ['B=257', 'B=511', 'B=1000']
    assert 'mode=1 step=1' in caught['adam:decay_in_coupled'] and caught['ladder:chunk2_at_0'] == ['K=65', 'K=130']
