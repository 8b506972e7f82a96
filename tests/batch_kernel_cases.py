"""The numpy side of the batch-kernel tests (tests/test_batch_kernels.py, tests/test_batch_kernels_gpu.py): the seeded inputs, a
float64 twin of each kernel's arithmetic (fthmc_amd/csrc/wilson.hip: k_train_metrics, k_stats_accumulate, k_adam, k_kinetic,
k_action_charge, k_ladder_set / k_ladder_init), the derived error bounds and the named mutants of the twins.  No mpmath here: the
60-digit references live in tests/golden/batch_kernels.npz (tests/golden/make_golden_batch_kernels.py).

Summation order of a workgroup sum, stated once (common.h ft_wave_sum, ft_block_sum): thread t adds its terms b = t, t + nt,
t + 2 nt, ... in order onto 0.0; the 64 lanes of a wave are folded by the xor tree v += v[lane ^ o], o = 32, 16, 8, 4, 2, 1; the
waves' sums are added in order onto 0.0.  Roundings on the way of one term (u = 2^-53 relative each, first-order analysis):
npass - 1 in the thread (npass = ceil(n / nt); the first addition onto 0.0 is exact), 6 in the tree, nw - 1 over the waves:
    sum_roundings(n, nt) = ceil(n / nt) + 5 + nt / 64 - 1
which is ceil(n / 256) + 8 for the one-workgroup kernels of 256 threads.  Every bound below is that count, plus the roundings
of the terms themselves, times u times the sum of the terms' magnitudes; the constants the bounds carry are never below the count
(the difference pays for the second-order terms), and every stored reference
carries its own rounding to fp64: half an ulp, which is up to u relative (u |ref|, not u / 2: half an ulp of x is u 2^e, |x| >= 2^e)."""
import math

import numpy as np

U = 2.0 ** -53
TINY = 8 * 2.0 ** -1074                      # absolute allowance where an intermediate underflows (g^2 at g = 1e-170)
B_LIST = (1, 63, 64, 65, 255, 256, 257, 511, 1000)


# ---------------------------------------------------------------- the workgroup sum
def strided_partials(terms, nt=256, fill=0.0, passes=None):
    """[nt] per-thread partials: thread t holds fill-started ((0.0 + terms[t]) + terms[t + nt]) + ...; passes: only the first so
    many passes of the loop (a mutant)"""
    terms = np.asarray(terms, dtype=np.float64)
    npass = -(-terms.size // nt)
    a = np.zeros(npass * nt)
    a[:terms.size] = terms
    a = a.reshape(npass, nt)
    acc = np.full(nt, fill)
    for r in range(npass if passes is None else min(passes, npass)):
        acc = acc + a[r]
    return acc


def wave_sum(v):
    """ft_wave_sum over the last axis of 64 lanes (every lane ends with the same bits: lane 0 is returned)"""
    v = np.array(v, dtype=np.float64)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ o]
    return v[..., 0]


def block_sum(part, drop_wave=None):
    """ft_block_sum of [nt] per-thread values: the wave sums added in order onto 0.0; drop_wave: a wave left out (a mutant)"""
    w = wave_sum(np.asarray(part, dtype=np.float64).reshape(-1, 64))
    t = np.float64(0.0)
    for i in range(w.size):
        if i != drop_wave:
            t = t + w[i]
    return t


def sum_roundings(n, nt=256):
    return -(-n // nt) + 5 + nt // 64 - 1


def npass256(B):
    return -(-B // 256)


# ---------------------------------------------------------------- 1. k_train_metrics
TM_L, TM_BETA, TM_F = 4, 3.0, 0.7
TM_FAMILIES = ('narrow', 'wide', 'far', 'equal', 'max_first', 'max_last', 'max_256')
TM_MUTANTS = ('drop_ge256', 'drop_wave3', 'max_first_pass', 'ess_no_invB')
PLANT = 1500.0      # a planted maximum stands this far above the others: exp(logw - m) overflows if m misses it


def tm_families(B):
    return tuple(f for f in TM_FAMILIES if f != 'max_256' or B > 256)


def tm_cases():
    return [(B, f) for B in B_LIST for f in tm_families(B)]


def tm_inputs(B, fam):
    """-> dict(logq, logp [B], x, xi [B, 2, L, L]); logw = logp - logq:
      narrow     sigma 3 each, offset 700 (the suite's one family so far)
      wide       sigma 150: ESS -> 1 / B, most exp(logw - m) underflow
      far        sigma 3, offset 1e4: exp overflows unless the maximum is subtracted
      equal      logq on multiples of 2^-20, logp = logq + 700 exactly: ESS = 1 exactly
      max_first / max_last / max_256   narrow with one logw raised by PLANT at index 0 / B - 1 / 256 + 3 (256 at B = 257)"""
    rng = np.random.default_rng(7000 + 16 * B + TM_FAMILIES.index(fam))
    sig, off = (150.0, 700.0) if fam == 'wide' else ((3.0, 1e4) if fam == 'far' else (3.0, 700.0))
    logq = rng.normal(0.0, sig, B) - off * 5.0 / 7.0                 # offset 700: -500 and +200, the suite's earlier inputs
    logp = rng.normal(0.0, sig, B) + off * 2.0 / 7.0
    if fam == 'equal':
        logq = np.round(logq * 2.0 ** 20) / 2.0 ** 20
        logp = logq + 700.0
        assert np.all(logp - logq == 700.0)
    at = {'max_first': 0, 'max_last': B - 1, 'max_256': min(256 + 3, B - 1)}.get(fam)
    if at is not None:
        logp[at] = logq[at] + 700.0 + PLANT
        assert int(np.argmax(logp - logq)) == at
    x = rng.uniform(-math.pi, math.pi, (B, 2, TM_L, TM_L))
    xi = rng.uniform(-math.pi, math.pi, (B, 2, TM_L, TM_L))
    return {'logq': logq, 'logp': logp, 'x': x, 'xi': xi}


def train_metrics_twin(logq, logp, f=TM_F, mutant=None):
    """(loss_dkl, ess) by k_train_metrics' expressions and order; numpy's exp stands in for the device's.  Mutants:
      drop_ge256      the strided loops stop after their first pass
      drop_wave3      ft_block_sum leaves wave 3's partial out
      max_first_pass  the maximum over the first 256 chains only
      ess_no_invB     ESS without 1 / B"""
    B = logq.size
    passes = 1 if mutant == 'drop_ge256' else None
    dw = 3 if mutant == 'drop_wave3' else None
    lw = logp - logq
    m = float(np.max(lw[:256] if mutant in ('max_first_pass', 'drop_ge256') else lw))
    with np.errstate(over='ignore', invalid='ignore', under='ignore'):
        e = np.exp(lw - m)
        t1 = block_sum(strided_partials(e, passes=passes), dw)
        t2 = block_sum(strided_partials(e * e, passes=passes), dw)
        td = block_sum(strided_partials(logq - logp, passes=passes), dw)
        loss = f * td / B
        ess = t1 * t1 / t2 if mutant == 'ess_no_invB' else t1 * t1 / t2 / B
    return loss, ess


def tm_bounds(logq, logp, f, loss_ref, ess_ref):
    """-> (absolute bound on loss_dkl, RELATIVE bound on ess).

    loss = fl(fl(f td) / B), td the workgroup sum of d_b = fl(logq_b - logp_b): one rounding per term, npass + 8 in the sum
    (sum_roundings), each relative to a partial sum of magnitude <= sum |d_b|; the product and the quotient: 2 u |loss|:
        |loss - exact| <= (npass + 9) u |f| mean|logw| + 2 u |loss|
    The bound keeps the constant npass + 12, which covers the second-order terms.

    ess = t1^2 / t2 / B does not depend on the shift m (it cancels between t1^2 and t2), so m is an exact constant of the
    analysis.  The exponent a_b = fl(fl(logp_b - logq_b) - m) is off by <= u (|logw_b| + |logw_b - m|) absolutely; the device's exp
    is within 1 ulp = 2 u: e_b carries eta = u (|logw_b| + |logw_b - m| + 2) relatively, e_b^2 carries 2 eta + u.  Sums of positive
    terms keep the relative error of their terms and add npass + 8 roundings; t1 t1 / t2 / B adds 3:
        |ess / exact - 1| <= 2 (eta + (npass + 8) u) + (2 eta + u + (npass + 8) u) + 3 u = 4 eta + 3 u (npass + 8) + 4 u
    The bound keeps 4 u (max|logw| + max|logw - m| + 2) + 3 u (npass + 12): 8 u above the count.  Terms that underflow: the largest
    term is exp(0) = 1, so t1, t2 >= 1 and B terms below 2^-1022 change them by less than 1e-300 relatively."""
    B = logq.size
    lw = logp - logq
    m = float(lw.max())
    n = npass256(B)
    b_loss = (n + 12) * U * abs(f) * float(np.abs(lw).mean()) + 3 * U * abs(loss_ref)
    b_ess = 4 * U * (float(np.abs(lw).max()) + float(np.abs(lw - m).max()) + 2.0) + 3 * U * (n + 12) + U
    return b_loss, b_ess


# ---------------------------------------------------------------- 2. k_stats_accumulate
ST_ROUNDS = 3
ST_MUTANTS = ('drop_ge256', 'drop_wave3', 'exp_pos', 'qold_stuck_ge256')
ST_INT_COLS, ST_FLOAT_COLS = (0, 1, 3, 4, 5), (2, 6, 7)


def st_inputs(B):
    """-> dict(acc, plaq, Q, dH [rounds, B], qold0 [B]).  acc in {0, 1}, Q integers in +-5, plaq uniform, dH normal with planted
    +800 (exp(-dH) = 0), -30 (one term of 1e13) and 0: at the last three indices (the last, partial wave) in round 0, at
    256 .. 258 (the second pass of the loop) in round 1, at 0 .. 2 in round 2; indices that B does not have are left out"""
    rng = np.random.default_rng(8000 + B)
    R = ST_ROUNDS
    d = {'acc': rng.integers(0, 2, (R, B)).astype(np.float64), 'plaq': rng.uniform(0.0, 1.0, (R, B)),
         'Q': rng.integers(-5, 6, (R, B)).astype(np.float64), 'dH': rng.normal(0.0, 1.0, (R, B)),
         'qold0': rng.integers(-5, 6, B).astype(np.float64)}
    for r, first in enumerate((B - 3, 256, 0)):
        for j, val in enumerate((0.0, -30.0, 800.0)):
            if 0 <= first + j < B:
                d['dH'][r, first + j] = val
    return d


def st_terms(inp, r, qold):
    """[8, B] terms of round r as the kernel forms them (numpy's exp for the device's)"""
    q, dH = inp['Q'][r], inp['dH'][r]
    with np.errstate(over='ignore', under='ignore'):
        return np.stack([np.ones_like(q), inp['acc'][r], inp['plaq'][r], q, q * q, np.abs(q - qold), dH, np.exp(-dH)])


def stats_twin(inp, mutant=None):
    """-> (vec [rounds, 8] after each round, qold [rounds, B] after each round).  Mutants:
      drop_ge256         the loop stops after its first pass (and moves no qold behind it)
      drop_wave3         wave 3's partial left out
      exp_pos            exp(dH) in place of exp(-dH)
      qold_stuck_ge256   qold not moved for b >= 256"""
    B = inp['qold0'].size
    passes = 1 if mutant == 'drop_ge256' else None
    dw = 3 if mutant == 'drop_wave3' else None
    qold = inp['qold0'].copy()
    vec = np.zeros(8)
    vecs, qolds = [], []
    for r in range(ST_ROUNDS):
        t = st_terms(inp, r, qold)
        if mutant == 'exp_pos':
            with np.errstate(over='ignore'):
                t[7] = np.exp(inp['dH'][r])
        with np.errstate(over='ignore', invalid='ignore'):
            vec = vec + np.array([block_sum(strided_partials(t[k], passes=passes), dw) for k in range(8)])
        moved = 256 if mutant in ('drop_ge256', 'qold_stuck_ge256') else B
        qold = qold.copy()
        qold[:moved] = inp['Q'][r][:moved]
        vecs.append(vec.copy()); qolds.append(qold.copy())
    return np.array(vecs), np.array(qolds)


def st_exact_ints(inp):
    """[rounds, 5] the integer-valued columns (n, acc, Q, Q^2, |Q - Qold|) after each round by integer sums"""
    qold = inp['qold0'].astype(np.int64)
    tot = np.zeros(5, dtype=np.int64)
    out = []
    for r in range(ST_ROUNDS):
        q, a = inp['Q'][r].astype(np.int64), inp['acc'][r].astype(np.int64)
        tot = tot + np.array([q.size, a.sum(), q.sum(), (q * q).sum(), np.abs(q - qold).sum()])
        qold = q
        out.append(tot.copy())
    return np.array(out)


def st_bounds(inp, ref):
    """[rounds, 3] absolute bounds on the plaq, dH and exp(-dH) columns after each round; ref [rounds, 3] the stored references.
    A round's workgroup sum: npass + 8 roundings; vec += t: one more per round behind the first, on everything added so far:
        (npass + 8 + rounds - 1) u sum|terms|     kept as (npass + 12 + rounds) u sum|terms|
    the exp column: the device's exp(-dH) within 1 ulp = 2 u of the exact one per term (-dH is exact) -- + 2 u sum|terms|;
    exp(-800) is 0 on the device and 1e-348 in the reference."""
    B = inp['qold0'].size
    tot = np.zeros(3)
    out = []
    for r in range(ST_ROUNDS):
        t = st_terms(inp, r, inp['qold0'])
        tot = tot + np.abs(t[list(ST_FLOAT_COLS)]).sum(axis=1)
        c = npass256(B) + 12 + (r + 1)
        out.append((c + np.array([0.0, 0.0, 2.0])) * U * tot + U * np.abs(ref[r]))
    return np.array(out)


# ---------------------------------------------------------------- 3. k_adam
AD_N = (1, 255, 257, 1025, 2865, 262144, 262145, 600001)
AD_FULL = 2865                                   # every element below this index has an mpmath reference
AD_MODES = ((0.0, False), (1e-2, False), (1e-2, True))
AD_BETAS, AD_EPS = (0.9, 0.999), 1e-8
AD_LR = (3e-3, 3e-3, 1e-3)                       # the rate in hyper[1] is changed on the device before the third step
AD_STEPS = 3
AD_MUTANTS = ('bias_t', 'eps_in_sqrt', 'decay_in_coupled')
G_EDGES = (0.0, -0.0, 1e-170, -1e-170, 1e150, -1e150)
P_EDGES = (0.0, 1e-300, 1e6, -1e6)
POW_ULP = 2.0                                    # the device's pow(b, t) is taken to be within 2 ulp (ocml documents 1)

_AD = {}


def adam_master():
    """One seeded set of 600001 elements; size n uses its first n (the update is elementwise: an element's reference does not
    depend on n).  g = normal x 10^U(-12, 6), p = normal x 10^U(-3, 3), m = normal x 10^U(-6, 2), v = (normal x 10^U(-6, 2))^2.
    Edge values sit at 1 .. 12 and below the end of every size from 255 on (n - 2 - j; 16 lower where the next size is within 12): the six g edges (at g = +-0 the moment m
    is 0 as well, and v at +0: p must stand still), the four p edges, and g = 0 with p = 1e6, g = 1e150 with p = 0.
    -> dict(p, g, m, v, zero_g: indices with g = +-0 and m = 0)"""
    if _AD:
        return _AD
    rng = np.random.default_rng(9001)
    N = max(AD_N)
    g = rng.normal(size=N) * 10.0 ** rng.uniform(-12, 6, N)
    p = rng.normal(size=N) * 10.0 ** rng.uniform(-3, 3, N)
    m = rng.normal(size=N) * 10.0 ** rng.uniform(-6, 2, N)
    v = (rng.normal(size=N) * 10.0 ** rng.uniform(-6, 2, N)) ** 2
    zero_g = []

    def plant(i0, step):
        i = i0
        for ge in G_EDGES:
            g[i] = ge
            if ge == 0.0:
                m[i] = 0.0
                zero_g.append(i)
                if not np.signbit(ge):
                    v[i] = 0.0
            i += step
        for pe in P_EDGES:
            p[i] = pe
            i += step
        g[i], p[i] = 0.0, 1e6; m[i] = 0.0; zero_g.append(i); i += step
        g[i], p[i] = 1e150, 0.0
    plant(1, 1)
    for n in AD_N:
        if n >= 255:
            plant(n - 2 - (16 if any(n < k <= n + 12 for k in AD_N) else 0), -1)      # clear of the next size's set
    assert len(set(zero_g)) == len(zero_g) and np.all(g[zero_g] == 0.0) and np.all(m[zero_g] == 0.0)
    _AD.update(p=p, g=g, m=m, v=v, zero_g=np.array(sorted(zero_g)))
    return _AD


def adam_sample():
    """sorted unique indices with an mpmath reference: everything below AD_FULL, the last 300 of every larger size, 100 around
    every multiple of 65536, 1000 seeded others below 262144 and 300 more above"""
    N = max(AD_N)
    rng = np.random.default_rng(9002)
    idx = [np.arange(AD_FULL)]
    for n in AD_N:
        if n > AD_FULL:
            idx.append(np.arange(n - 300, n))
    for c in range(65536, N, 65536):
        idx.append(np.arange(c - 50, c + 50))
    idx.append(rng.integers(AD_FULL, 262144, 1000))
    idx.append(rng.integers(262145, N, 300))
    return np.unique(np.concatenate(idx))


def adam_twin(p, g, m, v, t0, lr, wd, decoupled, mutant=None, betas=AD_BETAS, eps=AD_EPS):
    """one k_adam step in float64 numpy from (p, m, v) and the count t0 of steps taken -> (p, m, v).  Mutants:
      bias_t            bias corrections with t in place of t + 1
      eps_in_sqrt       m / sqrt(v / bc2 + eps)
      decay_in_coupled  p *= 1 - lr wd in the coupled mode too"""
    b1, b2 = betas
    t = t0 + (0.0 if mutant == 'bias_t' else 1.0)
    with np.errstate(all='ignore'):
        bc1, bc2s = 1.0 - math.pow(b1, t), math.sqrt(1.0 - math.pow(b2, t))
        step = np.float64(lr) / np.float64(bc1)
        pi, gi = np.array(p, dtype=np.float64), np.array(g, dtype=np.float64)
        if wd != 0.0:
            if decoupled or mutant == 'decay_in_coupled':
                pi = pi * (1.0 - lr * wd)
            if not decoupled:
                gi = gi + wd * np.asarray(p)
        mi = m + (gi - m) * (1.0 - b1)
        vi = v * b2 + (1.0 - b2) * gi * gi
        if mutant == 'eps_in_sqrt':
            den = np.sqrt(vi / (bc2s * bc2s) + eps)
        else:
            den = np.sqrt(vi) / bc2s + eps
        return pi - step * (mi / den), mi, vi


def adam_bounds(p, g, m, v, t0, lr, wd, decoupled, ref, betas=AD_BETAS, eps=AD_EPS):
    """Elementwise absolute bounds (bp, bm, bv) on one step from the pre-state (p, m, v); ref = (p', m', v') the exact step,
    rounded.  c1 = 1 - b1, c2 = 1 - b2, T = t0 + 1; with or without contraction into fused multiply-adds (fewer roundings):
      g_e = g (+ wd p, coupled): fl(wd p) and the sum, dg = 2 u (|g| + |wd p|)
      m' = m + (g_e - m) c1: the difference, fl(c1), the product, the sum:      bm = c1 (3 u |g_e - m| + dg) + u |m'|
      v' = v b2 + ((c2 g_e) g_e): one, three and one roundings:                 bv = u (|v b2| + 3 c2 g_e^2 + |v'|) + 2 c2 |g_e| dg
      dp = (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps), formed from the device's OWN m', v':
        bc = 1 - pow(b, T): the pow within POW_ULP ulp, the difference u: relative POW_ULP 2 u b^T / bc + u, halved under the root;
        the quotient lr / bc1, sqrt(v') (2 u allowed), sqrt(bc2), the quotient, + eps, m' / den, the product: 9.5 u; v' itself is a sum
        of non-negative terms: bv / v' relative, halved under the root.  Kept: 16 u + the pow terms + bv / (2 v')
      p' = p_e - dp, p_e = p (1 - lr wd) decoupled (three roundings):
        bp = u |p'| + 3 u |p| [decoupled] + (lr / bc1) bm / den + |dp| rel
    and TINY where g_e^2 underflows; each of the three carries u |ref| more for the stored reference's rounding (the 2 u in the code)."""
    b1, b2 = betas
    c1, c2, T = 1.0 - b1, 1.0 - b2, t0 + 1.0
    pr, mr, vr = ref
    coupled = wd != 0.0 and not decoupled
    with np.errstate(all='ignore'):
        ge = g + wd * p if coupled else g
        dg = 2 * U * (np.abs(g) + np.abs(wd * p)) if coupled else 0.0
        bm = c1 * (3 * U * np.abs(ge - m) + dg) + 2 * U * np.abs(mr) + TINY
        bv = U * (np.abs(v * b2) + 3 * c2 * ge * ge + 2 * np.abs(vr)) + 2 * c2 * np.abs(ge) * dg + TINY
        bc1, bc2 = 1.0 - b1 ** T, 1.0 - b2 ** T
        den = np.sqrt(vr) / math.sqrt(bc2) + eps
        step = lr / bc1
        dp = step * mr / den
        rel = U * (16.0 + POW_ULP * 2 * (b1 ** T / bc1 + 0.5 * b2 ** T / bc2)) + np.where(vr > 0, 0.5 * bv / np.where(vr > 0, vr, 1.0), 0.0)
        bp = 2 * U * np.abs(pr) + (3 * U * np.abs(p) if (wd != 0.0 and decoupled) else 0.0) + step * bm / den + np.abs(dp) * rel + TINY
    return bp, bm, bv


# ---------------------------------------------------------------- 4. k_kinetic, k_action_charge at the block-size thresholds
KA_B, KA_BETA = 3, 2.3
KA_L = (4, 28, 32, 44, 60, 64)
KA_SETS = ('uniform', 'flux3')
FLUX_K = 3


def nt_kinetic(L):
    n = 2 * L * L
    return 1024 if n >= 8192 else (512 if n >= 2048 else 256)


def nt_action(L):
    return 1024 if L * L >= 4096 else (512 if L * L >= 1024 else 256)


def ka_momenta(L):
    rng = np.random.default_rng(9100 + L)
    return rng.normal(size=(KA_B, 2, L, L)) * 10.0 ** rng.uniform(-3, 3, (KA_B, 2, L, L))


def ka_links(L, kind):
    """uniform: links uniform in +-pi.  flux3: the uniform-flux field of charge 3 -- x0[i][j] = -F j, x1[i][L-1] = (2 pi k / L) i,
    F = 2 pi k / L^2, every plaquette = F (mod 2 pi) -- under a random gauge transform x_mu(n) += alpha(n) - alpha(n + mu) with
    normal noise of sigma 0.02 on every link"""
    rng = np.random.default_rng(9200 + 2 * L + KA_SETS.index(kind))
    if kind == 'uniform':
        return rng.uniform(-math.pi, math.pi, (KA_B, 2, L, L))
    x = np.zeros((KA_B, 2, L, L))
    x[:, 0] = -(2.0 * math.pi * FLUX_K / (L * L)) * np.arange(L)[None, None, :]
    x[:, 1, :, L - 1] = (2.0 * math.pi * FLUX_K / L) * np.arange(L)[None, :]
    alpha = rng.uniform(-math.pi, math.pi, (KA_B, L, L))
    x[:, 0] += alpha - np.roll(alpha, -1, axis=-2)
    x[:, 1] += alpha - np.roll(alpha, -1, axis=-1)
    return x + rng.normal(0.0, 0.02, x.shape)


def kinetic_twin(v, nt=None):
    B, _, L, _ = v.shape
    nt = nt or nt_kinetic(L)
    return np.array([block_sum(strided_partials(vb * vb, nt)) for vb in v.reshape(B, -1)])


def plaq_angles(x):
    """the kernel's two angles per site: (a + d - cc - bb) for the cosine and (a - bb - cc + d) for the charge, each left to right"""
    a, bb = x[:, 0], x[:, 1]
    cc, d = np.roll(x[:, 0], -1, axis=-1), np.roll(x[:, 1], -1, axis=-2)
    return a + d - cc - bb, a - bb - cc + d


def action_twin(x, beta=KA_BETA, nt=None):
    """-> (S, Q, plaq) [B] by k_action_charge's expressions (numpy's cos and remainder for the device's cos and ft_wrap)"""
    B, _, L, _ = x.shape
    nt = nt or nt_action(L)
    pc, pq = plaq_angles(x)
    wq = np.remainder(pq + math.pi, 2.0 * math.pi) - math.pi
    c = np.array([block_sum(strided_partials(t, nt)) for t in np.cos(pc).reshape(B, -1)])
    q = np.array([block_sum(strided_partials(t, nt)) for t in wq.reshape(B, -1)])
    s = (-beta) * c
    return s, q / (2.0 * math.pi), (-s) / (beta * float(L * L))


def half_ulps(a):
    """sum of half an ulp of every entry: what rounding to these results can have cost"""
    return float(np.sum(np.spacing(np.abs(np.asarray(a, dtype=np.float64))))) / 2.0


def sum_rounding_bound(terms, nt):
    """First-order bound on the rounding error of a workgroup sum of non-negative terms, evaluated on the terms: half an ulp of the
    result of every rounded addition -- thread t's partials behind its first term, the distinct results of each level of the xor
    tree (32, 16, .. 1 per wave), the running sum over the waves behind wave 0.  (Errors made earlier reach the result with factor
    1: all terms are added, none multiplied.)"""
    a = np.asarray(terms, dtype=np.float64)
    assert np.all(a >= 0.0)
    npass = -(-a.size // nt)
    pad = np.zeros(npass * nt)
    pad[:a.size] = a
    pad = pad.reshape(npass, nt)
    acc, err = pad[0], 0.0
    for r in range(1, npass):
        acc = acc + pad[r]
        err += half_ulps(acc)
    v = acc.reshape(-1, 64)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ o]
        err += half_ulps(v[:, :o])
    t = 0.0
    for i in range(v.shape[0]):
        t = t + v[i, 0]
        if i:
            err += half_ulps(t)
    return err


def kinetic_cap(v, K_ref):
    """the ceiling no tolerance may exceed: (ceil(2 L^2 / nt) + 12) u K, and u K for the stored reference's rounding"""
    L = v.shape[-1]
    return (-(-2 * L * L // nt_kinetic(L)) + 13) * U * np.abs(K_ref)


def kinetic_bound(v, K_ref):
    """K = sum v^2, evaluated per chain: half an ulp of every square, sum_rounding_bound of the additions, 1e-6 of it for the second
    order, half an ulp of the stored reference.  A count of roundings alone would be (npass + 5 + nw) u K, nw = nt / 64 = 4, 8, 16
    waves, which passes the ceiling (npass + 12) u K at 512 and 1024 threads: it charges every later wave an error of u K where the
    running sum over the waves has only reached its share of K, and u |x| for a rounding that costs half an ulp of x.  On these
    inputs the evaluated bound lies below the ceiling, which is asserted here."""
    B, _, L, _ = v.shape
    nt = nt_kinetic(L)
    sq = (v * v).reshape(B, -1)
    bound = np.array([half_ulps(t) + sum_rounding_bound(t, nt) for t in sq]) * (1.0 + 1e-6) + np.spacing(np.abs(K_ref)) / 2.0
    assert np.all(bound <= kinetic_cap(v, K_ref)), (L, bound / (U * np.abs(K_ref)))
    return bound


def action_bounds(x, S_ref, plaq_ref, beta=KA_BETA):
    """-> (bound on S, bound on plaq) [B].  Links of magnitude <= pi mu.  The angle ((a + d) - cc) - bb: three roundings of partial
    sums of magnitude <= 2, 3, 4 pi mu: 9 pi mu u; the cosine moves by no more than its argument, the device's cos is within
    2 ulp = 4 u of magnitude <= 1: per plaquette (9 pi mu + 4) u; the sum: sum_roundings(L^2, nt) u sum|cos P| (+ 4 kept for the
    second order); (-beta) C: u |S|:
        |S - exact| <= beta [L^2 (9 pi mu + 4) + (npass + nw + 8) sum|cos P|] u + 1.5 u |S|
        plaq = (-S) / fl(beta L^2): the same over beta L^2, + 2 u |plaq|"""
    B, _, L, _ = x.shape
    nt = nt_action(L)
    mu = max(1.0, float(np.abs(x).max()) / math.pi)
    sc = np.abs(np.cos(plaq_angles(x)[0])).reshape(B, -1).sum(axis=1)
    core = beta * (L * L * (9 * math.pi * mu + 4) + (sum_roundings(L * L, nt) + 4) * sc) * U
    return core + 2 * U * np.abs(S_ref), core / (beta * L * L) + 3 * U * np.abs(plaq_ref)


Q_TOL = 1e-10            # |Q - the reference's integer|
PI_MARGIN = 1e-9         # condition on the reference: no plaquette angle nearer than this to +-pi


# ---------------------------------------------------------------- 5. exchange kernels
SWAP_SHAPES = ((2, 257), (5, 65), (3, 1000))       # (K, M): M (K - 1) = 257, 260, 2000 threads
LADDER_K, LADDER_M, LADDER_CHUNK = (64, 65, 130), 3, 64
PB_B = 300


def swap_edge_ladders(K, M):
    """-> (ladders with C_a = C_c planted on their first pairs, ladders with u = 0 on their last pair): the first and the last
    ladder for both; with one pair per ladder (K = 2) the u = 0 edge moves to the second and the last-but-one"""
    return (0, M - 1), ((1, M - 2) if K == 2 else (0, M - 1))


def swap_inputs(K, M, seed):
    """test_tempering_gpu.swap_inputs with its two edges in the last ladder as well as the first: C_a = C_c exactly on the first pair
    of either parity (d = 0, exp(d) = 1: accepted at u = 0.999), u = 0 on the last pair (accepted whatever d)"""
    import tempering_cases as TC
    rng = np.random.default_rng(seed)
    betas = np.cumsum(rng.uniform(0.3, 1.2, K))
    bb, rung, chain_of = TC.random_ladders(rng, betas, M)
    C = rng.normal(0.0, 2.0, M * K)
    u = rng.uniform(0.0, 1.0, (M, K - 1))
    eq, zero = swap_edge_ladders(K, M)
    for m in eq:
        o = m * K
        C[o + chain_of[o + 1]] = C[o + chain_of[o]]
        u[m, 0] = 0.999
        if K > 2:
            C[o + chain_of[o + 2]] = C[o + chain_of[o + 1]]
            u[m, 1] = 0.999
    for m in zero:
        u[m, K - 2] = 0.0
    return betas, bb, rung, chain_of, C, u


def ladder_betas(K):
    rng = np.random.default_rng(9300 + K)
    return np.cumsum(rng.uniform(0.01, 0.05, K))


def ladder_init_twin(betas, M, mutant=None):
    """fthmc_ladder_init: the ladder written in chunks of 64 rungs at betas + k0, then chain m K + k on rung k at betas[k].
    Mutant chunk2_at_0: every chunk written at betas + 0.  -> (betas, beta_b, rung, chain_of)"""
    betas = np.asarray(betas, dtype=np.float64)
    K = betas.size
    dev = np.full(K, np.nan)
    for k0 in range(0, K, LADDER_CHUNK):
        n = min(LADDER_CHUNK, K - k0)
        at = 0 if mutant == 'chunk2_at_0' else k0
        dev[at:at + n] = betas[k0:k0 + n]
    k = np.arange(M * K) % K
    return dev, dev[k], k.astype(np.int32), k.astype(np.int32)


# ---------------------------------------------------------------- readers of tests/golden/batch_kernels.npz
def adam_chain(G, mode, k):
    """-> (pre, ref): the fp64 state s_k = (p, m, v) at G['adam_idx'] before step k + 1 of mode `mode` and the stored exact step
    from it (s_0: the seeded inputs)"""
    A, idx = adam_master(), G['adam_idx']
    mv = 0 if mode == 2 else mode
    pre = (A['p'][idx], A['m'][idx], A['v'][idx]) if k == 0 else (G['adam_p'][mode, k - 1], G['adam_m'][mv, k - 1], G['adam_v'][mv, k - 1])
    return pre, (G['adam_p'][mode, k], G['adam_m'][mv, k], G['adam_v'][mv, k])


def tm_reference_of(G, B, fam):
    return G['tm'][tm_cases().index((B, fam))]


def frac(err, bound):
    """largest error as a fraction of its bound (nan if any error is nan: a nan is never inside a bound)"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    if np.any(np.isnan(err)):
        return math.nan
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.where(err == 0.0, 0.0, err / bound)
    return float(np.max(r))


def inside(err, bound):
    return bool(np.all(np.asarray(err) <= np.asarray(bound)))
