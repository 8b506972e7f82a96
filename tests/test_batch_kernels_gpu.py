"""GPU tests of the one-workgroup and one-thread-per-chain kernels past their first wave and their first workgroup: k_train_metrics,
k_stats_accumulate, k_adam, k_kinetic / k_action_charge at the block-size thresholds, k_replica_swap, k_ladder_set / k_ladder_init,
and the per-chain-beta trajectories at B = 300 (k_pb_from_state, k_lincomb at b >= 256).

References: tests/golden/batch_kernels.npz (mpmath at 60 digits on the fp64 inputs; tests/golden/make_golden_batch_kernels.py) and
the numpy twins of tests/batch_kernel_cases.py, where every bound is derived; tests/test_batch_kernels.py holds the twins to the same
bounds on the CPU and shows that each named mutant of a twin leaves them.  Each test prints its worst error as a fraction of the
bound.  Outputs land in slices of NaN-filled buffers whose guard words must keep their bits."""
import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden  # noqa: F401

import batch_kernel_cases as C
import integrator_cases as IC
import tempering_cases as TC

from gpu_support import D, H, Poisoned, R, bits, module_defaults, ops  # noqa: F401

pytestmark = pytest.mark.gpu
_defaults = module_defaults()

U = C.U


@pytest.fixture(scope='module')
def G():
    return load_golden('batch_kernels')


def report(name, value):
    print(f'WORST {name} {value:.4f}')


# ---------------------------------------------------------------- 1. k_train_metrics
@pytest.mark.parametrize('B', C.B_LIST)
def test_train_metrics_against_mpmath(G, B):
    L, beta = C.TM_L, C.TM_BETA
    worst = [0.0, 0.0]
    for fam in C.tm_families(B):
        d = C.tm_inputs(B, fam)
        loss_ref, ess_ref = C.tm_reference_of(G, B, fam)
        x, xi, logq, logp = D(d['x']), D(d['xi']), D(d['logq']), D(d['logp'])
        out = Poisoned(2 + 5 * B)
        row = ops.train_metrics(xi, x, logq, logp, beta, dkl_factor=C.TM_F, out=out.t)
        torch.cuda.synchronize()
        assert row.data_ptr() == out.t.data_ptr() and out.intact(), fam
        m = {k: H(t) for k, t in ops.split_metrics(row, B).items()}
        bl, be = C.tm_bounds(d['logq'], d['logp'], C.TM_F, loss_ref, ess_ref)
        fl, fe = C.frac(abs(float(m['loss_dkl']) - loss_ref), bl), C.frac(abs(float(m['ess']) / ess_ref - 1.0), be)
        print(f'B={B} {fam}: loss {float(m["loss_dkl"])!r} ref {loss_ref!r} ({fl:.3f} of the bound), ess {float(m["ess"])!r} ref {ess_ref!r} ({fe:.3f})')
        assert fl <= 1.0 and fe <= 1.0, (fam, fl, fe)
        worst = [max(worst[0], fl), max(worst[1], fe)]
        if fam == 'equal':
            assert float(m['ess']) == 1.0
        assert np.array_equal(bits(m['logp']), bits(d['logp'])) and np.array_equal(bits(m['logq']), bits(d['logq'])), fam
        q, qi = H(ops.wilson_action_charge(x, beta)[1]), H(ops.wilson_action_charge(xi, beta)[1])
        assert np.array_equal(bits(m['q']), bits(q)), fam
        assert np.array_equal(m['dq'], np.abs(q - qi)), fam
        pr = d['logp'] / (beta * L * L)
        assert np.all(np.abs(m['plaq'] - pr) <= 2 * np.spacing(np.abs(pr))), fam
    report('train_metrics.loss', worst[0]); report('train_metrics.ess', worst[1])


# ---------------------------------------------------------------- 2. k_stats_accumulate
@pytest.mark.parametrize('B', C.B_LIST)
def test_stats_accumulate_three_rounds(G, B):
    inp = C.st_inputs(B)
    ref = G['st'][C.B_LIST.index(B)]
    ints = C.st_exact_ints(inp)
    bnd = C.st_bounds(inp, ref)
    vec, qold = Poisoned(8, np.zeros(8)), Poisoned(B, inp['qold0'])
    worst = 0.0
    for r in range(C.ST_ROUNDS):
        ops.stats_accumulate(D(inp['acc'][r]), D(inp['plaq'][r]), D(inp['Q'][r]), qold.t, D(inp['dH'][r]), vec.t)
        torch.cuda.synchronize()
        v = H(vec.t)
        assert np.array_equal(v[list(C.ST_INT_COLS)], ints[r].astype(np.float64)), (r, v, ints[r])
        f = C.frac(np.abs(v[list(C.ST_FLOAT_COLS)] - ref[r]), bnd[r])
        print(f'B={B} round {r}: plaq, dH, exp(-dH) sums {v[list(C.ST_FLOAT_COLS)].tolist()} ref {ref[r].tolist()} ({f:.3f} of the bound)')
        assert f <= 1.0, (r, f)
        worst = max(worst, f)
        assert np.array_equal(bits(qold.t), bits(inp['Q'][r])), r
        assert vec.intact() and qold.intact(), r
    report('stats_accumulate', worst)


# ---------------------------------------------------------------- 3. k_adam
class AdamState:
    def __init__(self, n):
        A = C.adam_master()
        self.n = n
        self.p, self.m, self.v = Poisoned(n, A['p'][:n]), Poisoned(n, A['m'][:n]), Poisoned(n, A['v'][:n])
        self.g = Poisoned(n, A['g'][:n])
        self.hyper = Poisoned(3, [0.0, C.AD_LR[0], 0.0])
        self.gbits = bits(self.g.t)

    def step(self, wd, dec):
        ops.adam_step(self.p.t, self.g.t, self.m.t, self.v.t, self.hyper.t, betas=C.AD_BETAS, eps=C.AD_EPS, weight_decay=wd, decoupled=dec)

    def set_lr(self, k):
        self.hyper.t[1:2].fill_(C.AD_LR[k])                  # on the device, on the stream of the steps: no host sync

    def state(self):
        return H(self.p.t), H(self.m.t), H(self.v.t)

    def intact(self):
        return all(t.intact() for t in (self.p, self.m, self.v, self.g, self.hyper)) and np.array_equal(bits(self.g.t), self.gbits)


@pytest.mark.parametrize('mode', range(len(C.AD_MODES)), ids=['adam', 'adam-wd', 'adamw'])
@pytest.mark.parametrize('n', C.AD_N)
def test_adam_three_steps(G, n, mode):
    wd, dec = C.AD_MODES[mode]
    A = C.adam_master()
    g = A['g'][:n]
    # A: three launches back to back, the rate changed on the device before the third, one sync at the end
    a = AdamState(n)
    for k in range(C.AD_STEPS):
        a.set_lr(k)
        a.step(wd, dec)
    torch.cuda.synchronize()
    hy = H(a.hyper.t)
    assert hy[0] == 3.0 and hy[1] == C.AD_LR[2] and bits(a.hyper.t)[2] == 0, hy
    assert a.intact()
    final = a.state()
    assert all(np.all(np.isfinite(t)) for t in final)
    # B: one at a time; every step against the numpy restatement applied to the device's own state before it, every element
    b = AdamState(n)
    worst = np.zeros(3)
    zg = A['zero_g'][A['zero_g'] < n]
    for k in range(C.AD_STEPS):
        pre = b.state()
        b.set_lr(k)
        b.step(wd, dec)
        torch.cuda.synchronize()
        post = b.state()
        assert H(b.hyper.t)[0] == k + 1.0 and bits(b.hyper.t)[2] == 0
        tw = C.adam_twin(pre[0], g, pre[1], pre[2], float(k), C.AD_LR[k], wd, dec)
        bnd = C.adam_bounds(pre[0], g, pre[1], pre[2], float(k), C.AD_LR[k], wd, dec, tw)
        f = [C.frac(np.abs(x - y), z) for x, y, z in zip(post, tw, bnd)]
        assert max(f) <= 1.0, ('twin', k, f)
        worst = np.maximum(worst, f)
        if wd == 0.0 and zg.size:                               # g = +-0 with m = 0: p stands still
            assert np.all(np.abs(post[0][zg] - pre[0][zg]) <= U * np.abs(pre[0][zg])) and np.all(post[1][zg] == 0.0), k
    for x, y in zip(b.state(), final):
        assert np.array_equal(bits(x), bits(y))                 # the unsynchronised run took the same three steps
    assert b.intact()
    report(f'adam.twin[n={n},{mode}]', float(worst.max()))
    # C: one at a time from the stored fp64 states at the sampled elements, against the exact step from those states
    idx = G['adam_idx'][G['adam_idx'] < n]
    sel = slice(0, idx.size)
    assert n > C.AD_FULL or idx.size == n
    c = AdamState(n)
    gi = g[idx]
    ti = torch.as_tensor(idx).cuda()
    worst = np.zeros(3)
    for k in range(C.AD_STEPS):
        pre, ref = C.adam_chain(G, mode, k)
        pre, ref = [t[sel] for t in pre], [t[sel] for t in ref]
        for buf, val in zip((c.p, c.m, c.v), pre):
            buf.t[ti] = D(val)
        c.set_lr(k)
        c.step(wd, dec)
        torch.cuda.synchronize()
        post = [t[idx] for t in c.state()]
        bnd = C.adam_bounds(pre[0], gi, pre[1], pre[2], float(k), C.AD_LR[k], wd, dec, ref)
        f = [C.frac(np.abs(x - y), z) for x, y, z in zip(post, ref, bnd)]
        print(f'n={n} mode {mode} step {k + 1}: p, m, v against mpmath at {idx.size} elements: {f} of the bounds')
        assert max(f) <= 1.0, ('mpmath', k, f)
        worst = np.maximum(worst, f)
    assert c.intact() and all(np.all(np.isfinite(t)) for t in c.state())
    report(f'adam.mpmath[n={n},{mode}]', float(worst.max()))


# ---------------------------------------------------------------- 4. k_kinetic, k_action_charge at the block-size thresholds
@pytest.mark.parametrize('L', C.KA_L)
def test_kinetic_and_action_at_the_block_size_thresholds(G, L):
    li = C.KA_L.index(L)
    v = C.ka_momenta(L)
    K = H(ops.kinetic(D(v)))
    fk = C.frac(np.abs(K - G['kin'][li]), C.kinetic_bound(v, G['kin'][li]))
    print(f'L={L}: K {K.tolist()} ref {G["kin"][li].tolist()} ({fk:.3f} of the bound)')
    assert fk <= 1.0
    report('kinetic', fk)
    for si, kind in enumerate(C.KA_SETS):
        x = C.ka_links(L, kind)
        S, Q, plaq = (H(t) for t in ops.wilson_action_charge(D(x), C.KA_BETA))
        bS, bp = C.action_bounds(x, G['act_S'][li, si], G['act_plaq'][li, si])
        fs, fp = C.frac(np.abs(S - G['act_S'][li, si]), bS), C.frac(np.abs(plaq - G['act_plaq'][li, si]), bp)
        fq = C.frac(np.abs(Q - G['act_Q'][li, si]), C.Q_TOL)
        print(f'L={L} {kind}: S {S.tolist()} ({fs:.3f}), plaq {plaq.tolist()} ({fp:.3f}), Q {Q.tolist()} ({fq:.2e} of 1e-10)')
        assert fs <= 1.0 and fp <= 1.0 and fq <= 1.0, (kind, fs, fp, fq)
        report('action.S', fs); report('action.plaq', fp); report('action.Q', fq)


# ---------------------------------------------------------------- 5. exchange kernels past one workgroup
def swap_against_numpy(betas, bb, rung, chain_of, Cs, u, parity, g=None, edges=None):
    """one round on the device against TC.swap_round: the assertions of test_tempering_gpu.test_replica_swap_against_the_numpy_round;
    g: device (betas, beta_b, rung, chain_of) to run on in place (else fresh copies) -> the round's (beta_b, rung, chain_of)"""
    K, M = len(betas), len(bb) // len(betas)
    nb, nr, nc, acc, d, e = TC.swap_round(betas, Cs, u, bb, rung, chain_of, parity)
    tried = acc >= 0
    assert np.all(np.abs(u[tried] - e[tried]) > 1e-12 * e[tried])
    if edges is not None:
        eq, zero = edges
        for m in eq:
            if parity < K - 1:
                assert acc[m, parity] == 1.0 and d[m, parity] == 0.0
        for m in zero:
            if (K - 2) % 2 == parity:
                assert acc[m, K - 2] == 1.0
    g_b, g_bb, g_r, g_c = g if g is not None else (D(betas), D(bb), D(rung, torch.int32), D(chain_of, torch.int32))
    out = ops.replica_swap(g_b, D(Cs), D(u), g_bb, g_r, g_c, parity)
    torch.cuda.synchronize()
    assert np.array_equal(H(out['swap_acc']), acc)
    assert np.array_equal(bits(g_bb), nb.view(np.int64)) and np.array_equal(H(g_r), nr) and np.array_equal(H(g_c), nc)
    gd = H(out['d'])
    assert np.all(np.abs(gd - d) <= 2 * np.spacing(np.abs(d)))
    assert np.all(gd[~tried] == 0.0)
    if g is None:                                                # the operator: the same bits from the same start
        import fthmc_amd.torch_ops  # noqa: F401
        o_bb, o_r, o_c = D(bb), D(rung, torch.int32), D(chain_of, torch.int32)
        o_acc, o_d = torch.ops.fthmc_hip.replica_swap(D(betas), D(Cs), D(u), o_bb, o_r, o_c, parity)
        assert torch.equal(o_acc, out['swap_acc']) and torch.equal(o_d, out['d'])
        assert torch.equal(o_bb, g_bb) and torch.equal(o_r, g_r) and torch.equal(o_c, g_c)
    TC.check_ladders(betas, nb, nr, nc)
    return nb, nr, nc


@pytest.mark.parametrize('parity', [0, 1])
@pytest.mark.parametrize('K,M', C.SWAP_SHAPES)
def test_replica_swap_past_one_workgroup(K, M, parity):
    betas, bb, rung, chain_of, Cs, u = C.swap_inputs(K, M, 2000 + 10 * K + M)
    assert M * (K - 1) > 256
    swap_against_numpy(betas, bb, rung, chain_of, Cs, u, parity, edges=C.swap_edge_ladders(K, M))


@pytest.mark.parametrize('K', C.LADDER_K)
def test_ladder_init_past_one_chunk_then_a_round_of_each_parity(K):
    M = C.LADDER_M
    betas = C.ladder_betas(K)
    lad = ops.ladder_init(betas, M, device='cuda')
    torch.cuda.synchronize()
    tb, tbb, tr, tc = C.ladder_init_twin(betas, M)
    assert np.array_equal(bits(lad['betas']), betas.view(np.int64)), np.nonzero(H(lad['betas']) != betas)[0]
    assert np.array_equal(bits(lad['beta_b']), tbb.view(np.int64))
    assert H(lad['rung']).dtype == np.int32 and np.array_equal(H(lad['rung']), tr) and np.array_equal(H(lad['chain_of']), tc)
    rng = np.random.default_rng(9400 + K)
    Cs, u = rng.normal(0.0, 40.0, M * K), rng.uniform(0.0, 1.0, (M, K - 1))
    state = (tbb, tr, tc)
    g = (lad['betas'], lad['beta_b'], lad['rung'], lad['chain_of'])
    for parity in (0, 1):
        state = swap_against_numpy(betas, *state, Cs, u, parity, g=g)
    assert not np.array_equal(state[1], tr)                          # chains moved


KEYS = ('x_new', 'dH', 'acc', 'H0', 'H1', 'plaq', 'Q')
PKEYS = ('x_new', 'dH', 'acc', 'H0', 'H1')
NSTEP, DT = 3, TC.TAU / 3


def test_plain_hmc_per_chain_beta_at_300_chains():
    B, L = C.PB_B, 8
    x, v, u = (t.cuda() for t in IC.draw(4300 + L, B, L))
    beta_b = TC.ladder_betas(B)
    r = ops.hmc_trajectory(x, v, u, D(beta_b), DT, NSTEP)
    for beta in TC.LADDER:
        ref = ops.hmc_trajectory(x, v, u, beta, DT, NSTEP)
        idx = torch.as_tensor(np.nonzero(beta_b == beta)[0]).cuda()
        assert int(idx.max()) >= 256
        for k in PKEYS:
            assert torch.equal(r[k][idx], ref[k][idx]), (k, beta)
    assert len(set(H(r['dH']).tolist())) == B


@pytest.mark.parametrize('L,nl', [(8, 2), (32, 1)], ids=['small-L8', 'L32'])
def test_flowed_per_chain_beta_at_300_chains(L, nl):
    """every chain bit-equal to the scalar call at its beta; a chained call with state_in after rolling beta_b bit-equal to the
    stateless one (keys and the two-rounding rule for S_eff as in tests/test_tempering_gpu.py)"""
    B = C.PB_B
    flow = R.default_flow(nl, torch.Generator().manual_seed(4400 + L))
    w = ops.pack_weights(flow, device='cuda')
    x, v, u = (t.cuda() for t in IC.draw(4400 + L, B, L))
    beta_b = TC.ladder_betas(B)
    r = ops.ft_trajectory(x, v, u, w, nl, D(beta_b), DT, NSTEP, mode='md')
    torch.cuda.synchronize()
    for beta in TC.LADDER:
        ref = ops.ft_trajectory(x, v, u, w, nl, beta, DT, NSTEP, mode='md')
        at = np.nonzero(beta_b == beta)[0]
        idx = torch.as_tensor(at).cuda()
        assert at.max() >= 256
        for k in KEYS:
            assert torch.equal(r[k][idx], ref[k][idx]), (k, beta)
        assert TC.state_matches(H(r['state'])[:, at], beta_b[at], L, H(ref['state'])[:, at]), beta
    assert len(set(H(r['dH']).tolist())) == B
    # the carried state is beta-free at b >= 256 too
    _, v2, u2 = IC.draw(4977, B, L)
    perm = np.roll(beta_b, 1)
    u1 = u.clone(); u1[::2] = 0.0
    r1 = ops.ft_trajectory(x, v, u1, w, nl, D(beta_b), DT, NSTEP)
    x1, st = r1['x_new'].clone(), r1['state'].clone()
    ra = ops.ft_trajectory(x1, v2.cuda(), u2.cuda(), w, nl, D(perm), DT, NSTEP, state_in=st)
    ra = {k: t.clone() for k, t in ra.items()}
    rb = ops.ft_trajectory(x1, v2.cuda(), u2.cuda(), w, nl, D(perm), DT, NSTEP)
    torch.cuda.synchronize()
    assert float(r1['acc'][::2].sum()) == len(r1['acc'][::2])
    for k in KEYS + ('state',):
        assert torch.equal(ra[k], rb[k]), k
