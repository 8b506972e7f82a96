"""Shared pieces of the replica-exchange tests (tests/test_tempering.py, tests/test_tempering_gpu.py): the swap round in plain
numpy -- the reference k_replica_swap is held to --, the exact finite-volume plaquette of 2D U(1), the path matrix of the
per-chain-beta trajectory and the helpers that rebuild (S_eff, plaq) from the beta-free state by the kernels' expressions."""
import math

import numpy as np

LADDER = (1.5, 2.0, 3.0)

# (id, L, B, layers, net shape, variant, small path): the smallest shape that reaches each kernel instance of the flowed call
#   small path                 k_ft_small<.., SCHED, PB> (one launch)
#   tiled-L16                  the tuned kernels at a small-path size with the small path off
#   L32 / L64                  k_force<2, PB> / k_gp_rows<8, PB> seeds, k_traj_energy<PB>
#   L128                       the tuned branch at a large lattice with few chains (its action sums are k_traj_energy<PB>'s)
#   net-4-3-1-L128, plain-ft-L128   the GENERAL branch at B < 128, L >= 128: the action sums run one wave per workgroup
#                              (k_action_charge_waves + k_action_charge_fin_pb) -- another net shape, and zero layers
#   ragged-L20                 tiles that do not divide the lattice
#   net-4-3-1-L8               another net shape: the general branch (k_action_charge_pb, k_pb_from_state)
#   valu-L16                   the VALU variant
FT_PATHS = [('small-L8', 8, 6, 2, None, 1, True), ('small-L16', 16, 6, 2, None, 1, True), ('tiled-L16', 16, 6, 2, None, 1, False),
            ('L32', 32, 4, 2, None, 1, True), ('L64', 64, 4, 2, None, 1, True), ('L128', 128, 2, 1, None, 1, True),
            ('ragged-L20', 20, 6, 2, None, 1, True), ('net-4-3-1-L8', 8, 6, 2, ((4,), 3, 1), 1, True),
            ('valu-L16', 16, 6, 2, None, 0, False),
            ('net-4-3-1-L128', 128, 2, 1, ((4,), 3, 1), 1, True), ('plain-ft-L128', 128, 2, 0, None, 1, True)]
# plain HMC: the one-launch kernel (L <= 64) and the fused row-strip steps + k_action_charge_pb
PLAIN_PATHS = [('plain-L8', 8, 6), ('plain-L128', 128, 2)]
# every integrator on these rows, the leapfrog on all
ALL_INTEGRATORS_ON = ('small-L8', 'L32')
INTEGRATORS = (('leapfrog', 3), ('omelyan', 3), ('force_gradient', 2))
TAU = 0.3


def ladder_betas(B, ladder=LADDER):
    """the ladder repeated over B chains"""
    return np.array([ladder[b % len(ladder)] for b in range(B)], dtype=np.float64)


def swap_round(betas, C, u, beta_b, rung, chain_of, parity):
    """One replica-exchange round on copies of the arrays, pair by pair:
    for every ladder m and every k = parity (mod 2) with k + 1 < K: a = chain on rung k, c = chain on rung k + 1,
    d = (beta_k - beta_{k+1}) (C_c - C_a), accept iff u[m][k] < exp(d); on accept the two chains exchange rung, beta_b, chain_of.
    -> (beta_b, rung, chain_of, swap_acc [M, K - 1] in {1, 0, -1 = not attempted}, d [M, K - 1], e = exp(d) where attempted)"""
    betas = np.asarray(betas, dtype=np.float64)
    K = betas.size
    beta_b = np.array(beta_b, dtype=np.float64)
    rung = np.array(rung, dtype=np.int32)
    chain_of = np.array(chain_of, dtype=np.int32)
    M = beta_b.size // K
    C = np.asarray(C, dtype=np.float64).reshape(-1)
    u = np.asarray(u, dtype=np.float64).reshape(M, K - 1)
    acc = -np.ones((M, K - 1))
    d = np.zeros((M, K - 1))
    e = np.full((M, K - 1), np.nan)
    for m in range(M):
        for k in range(parity, K - 1, 2):
            al, cl = int(chain_of[m * K + k]), int(chain_of[m * K + k + 1])
            a, c = m * K + al, m * K + cl
            d[m, k] = (betas[k] - betas[k + 1]) * (C[c] - C[a])
            e[m, k] = math.exp(d[m, k]) if d[m, k] < 700 else math.inf
            if u[m, k] < e[m, k]:
                acc[m, k] = 1.0
                rung[a], rung[c] = k + 1, k
                beta_b[a], beta_b[c] = betas[k + 1], betas[k]
                chain_of[m * K + k], chain_of[m * K + k + 1] = cl, al
            else:
                acc[m, k] = 0.0
    return beta_b, rung, chain_of, acc, d, e


def random_ladders(rng, betas, M):
    """M ladders in a random arrangement -> (beta_b, rung, chain_of)"""
    K = len(betas)
    rung = np.concatenate([rng.permutation(K) for _ in range(M)]).astype(np.int32)
    chain_of = np.empty_like(rung)
    for m in range(M):
        chain_of[m * K + rung[m * K:(m + 1) * K]] = np.arange(K, dtype=np.int32)
    return np.asarray(betas, dtype=np.float64)[rung], rung, chain_of


def check_ladders(betas, beta_b, rung, chain_of):
    """rung is a permutation within each ladder, chain_of its inverse, beta_b[b] == betas[rung[b]] bitwise"""
    betas = np.asarray(betas, dtype=np.float64)
    K = betas.size
    M = rung.size // K
    for m in range(M):
        r, c = rung[m * K:(m + 1) * K], chain_of[m * K:(m + 1) * K]
        assert sorted(r.tolist()) == list(range(K)), (m, r)
        assert np.array_equal(c[r], np.arange(K)) and np.array_equal(r[c], np.arange(K)), (m, r, c)
    assert np.array_equal(beta_b.view(np.int64), betas[rung].view(np.int64))


def exact_plaquette(beta, V):
    """<cos P> of 2D U(1) on a periodic lattice of V plaquettes: sum_n I_n^(V-1) I_n' / sum_n I_n^V (character expansion;
    I_n' = (I_{n-1} + I_{n+1}) / 2), in 50 digits"""
    import mpmath as mp
    mp.mp.dps = 50
    b = mp.mpf(beta)
    num = den = mp.mpf(0)
    for n in range(-20, 21):                       # I_n^V beyond |n| = 20 is below 1e-1000 of the sum for beta <= 8
        i_n = mp.besseli(n, b)
        d_n = (mp.besseli(n - 1, b) + mp.besseli(n + 1, b)) / 2
        num += i_n ** (V - 1) * d_n
        den += i_n ** V
    return float(num / den)


def state_to_scalar(state, beta_b, L):
    """(S_eff, S_eff fused, plaq, Q) as numpy arrays from the beta-free state [3, B] = (log det J, C, Q) by the kernels' expressions:
    S_W = (-beta) C; S_eff = S_W - log det J; plaq = (-S_W) / (beta L^2).  The compiler is free to contract the first two into ONE
    fused multiply-add (one rounding of (-beta) C - log det J instead of two), and does so in the kernels that keep S_W in a
    register: both roundings of that one expression are given, S_eff of a chain must be one of them; plaq has one form."""
    from fractions import Fraction
    st = np.asarray(state, dtype=np.float64)
    bb = np.asarray(beta_b, dtype=np.float64)
    ld, C, Q = st[0], st[1], st[2]
    s = (-bb) * C
    fused = np.array([float(Fraction(-float(b)) * Fraction(float(c)) - Fraction(float(l))) for b, c, l in zip(bb, C, ld)])
    return s - ld, fused, (-s) / (bb * float(L * L)), Q


def state_matches(state, beta_b, L, ref_state):
    """the beta-free state against a scalar call's (S_eff, plaq, Q): plaq and Q bit for bit, S_eff one of its two roundings"""
    seff, fused, plaq, Q = state_to_scalar(state, beta_b, L)
    ref = np.asarray(ref_state, dtype=np.float64)
    return bool(np.all((seff == ref[0]) | (fused == ref[0])) and np.array_equal(plaq, ref[1]) and np.array_equal(Q, ref[2]))
