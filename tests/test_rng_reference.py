"""The reference of the random streams (tests/philox_ref.py) pinned to published vectors, and the design of the streams pinned
on the reference: what tests/test_rng_gpu.py then holds the kernels to, bit for bit.  No GPU.

Statistics: every bound is fixed beforehand -- a Kolmogorov-Smirnov distance whose chance of being exceeded is below 1e-9
(Massart's form of the DKW inequality: P(D > e) <= 2 exp(-2 N e^2)), and |z| < 6 for sums whose exact variance is known
(P = 2e-9 each) -- never fitted to what the streams give.
"""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import philox_ref as PR
from fthmc_amd import parallel

SHAPES = [(1331, 128, 64), (7, 16, 16), (78, 32, 32)]      # (seed, chains, L): bench's SEED at its headline shape, two small ones
BENCH_SEEDS = (1331, 1332, 1338, 1362)                     # bench.py: SEED, SEED + 1, + 7, + 31


# ----------------------------------------------------------------------------------------------------------- known answers
KAT = PR.KAT


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32 with 10 rounds, one at a time and as one vectorised call"""
    for ctr, key, want in KAT:
        assert tuple(int(x) for x in PR.philox4x32_10(ctr, key)) == want
    ctr = [np.array([k[0][i] for k in KAT]) for i in range(4)]
    key = [np.array([k[1][i] for k in KAT]) for i in range(2)]
    got = np.stack(PR.philox4x32_10(ctr, key), axis=1)
    assert np.array_equal(got, np.array([k[2] for k in KAT], dtype=np.uint64))
    # nine rounds are another function
    assert tuple(int(x) for x in PR.philox4x32_10(*KAT[0][:2], rounds=9)) != KAT[0][2]


def test_u53_and_the_exact_value_builders():
    """k = m + 1 covers [1, 2^53]; the low 11 bits of the word pair do not count; accept_u is exact and in [0, 1);
    uniform (bulk) = uniform_exact (Fraction) wherever they are compared, edges included"""
    assert int(PR.u53(0, 0)) == 1 and int(PR.u53(0xffffffff, 0xffffffff)) == 1 << 53
    assert int(PR.u53(0, 0x7ff)) == 1 and int(PR.u53(0, 0x800)) == 2 and int(PR.u53(1, 0)) == (1 << 21) + 1
    g = np.random.default_rng(1)
    k = np.concatenate([g.integers(1, (1 << 53) + 1, 20000, dtype=np.uint64), np.array([1, 2, 3, (1 << 52), (1 << 52) + 1,
                        (1 << 53) - 1, 1 << 53], dtype=np.uint64)])
    hi, lo = PR.words_of(k)
    assert np.array_equal(PR.u53(hi, lo), k)
    u = PR.accept_u(k)
    assert u.min() == 0.0 and u.max() == 1.0 - 2.0 ** -53
    for kk, uu in zip(k[-7:], u[-7:]):
        assert Fraction(float(uu)) == 1 - Fraction(int(kk), 1 << 53)
    for lo_, hi_ in ((0.0, 1.0), (-math.pi, math.pi), (1e6, 1e6 + 1), (-3.0, 3.0), (-1e-3, 7.0)):
        assert np.array_equal(PR.uniform(k, lo_, hi_), PR.uniform_exact(k, lo_, hi_)), (lo_, hi_)
    # the prior's range as the reference rounds it: [lo, hi) on (0, 1) and on (-pi, pi), the top value of k = 1 included
    assert PR.uniform_exact([1], 0.0, 1.0)[0] == 1.0 - 2.0 ** -53 and PR.uniform_exact([1 << 53], 0.0, 1.0)[0] == 0.0
    top = PR.uniform_exact([1], -math.pi, math.pi)[0]
    assert top < math.pi and PR.uniform_exact([1 << 53], -math.pi, math.pi)[0] == -math.pi
    # ... and not on every range: where the width is small next to |lo| the correctly rounded top value IS hi
    assert PR.uniform_exact([1], 1e6, 1e6 + 1)[0] == 1e6 + 1


def test_normal_pair_references_agree():
    """longdouble (bulk) against mpmath at 40 digits (edge sets) on random and extreme k: within 2^-59 of the radius
    (1 / 64 of the unit rad 2^-53 the device is held to)"""
    mpmath = pytest.importorskip('mpmath')
    mpmath.mp.dps = 40
    assert np.finfo(np.longdouble).nmant == 63
    g = np.random.default_rng(2)
    k1 = np.concatenate([g.integers(1, (1 << 53) + 1, 300, dtype=np.uint64), np.array([1, 1 << 53, (1 << 53) - 1, 2], dtype=np.uint64)])
    k2 = np.concatenate([g.integers(1, (1 << 53) + 1, 300, dtype=np.uint64), np.array([1, 1 << 53, 1 << 52, 1 << 51], dtype=np.uint64)])
    a, b, rad = PR.normal_pair_ld(k1, k2)
    for i in range(len(k1)):
        ma, mb, mr = PR.normal_pair_mp(k1[i], k2[i])
        scale = max(float(mr), 1e-8) * 2.0 ** -59
        assert abs(mpmath.mpf(float(rad[i])) - mr) <= 2.0 ** -52 * max(float(mr), 1e-8)
        for dev, ref in ((a[i], ma), (b[i], mb)):
            hi, lo = float(dev), float(dev - np.longdouble(float(dev)))
            assert abs(mpmath.mpf(hi) + mpmath.mpf(lo) - ref) <= scale, (int(k1[i]), int(k2[i]))


# ----------------------------------------------------------------------------------------------------------- statistics
def _momenta(seeds, n):
    k1, k2 = PR.momenta_bits(seeds, n)
    rad = np.sqrt(-2.0 * np.log(k1.astype(np.float64) * 2.0 ** -53))
    ang = 2.0 * math.pi * (k2.astype(np.float64) * 2.0 ** -53)
    pairs = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=-1)          # [B, npair, 2]
    return pairs.reshape(len(seeds), -1)[:, :n], pairs


def _z(prod, var=1.0):
    """z-score of a sum of products of independent centred variables whose product has variance `var`"""
    prod = np.asarray(prod, dtype=np.float64).ravel()
    return float(prod.sum() / math.sqrt(var * prod.size))


@pytest.mark.parametrize('s,B,L', SHAPES)
def test_reference_momenta_are_standard_normal_and_uncorrelated(s, B, L):
    n = 2 * L * L
    seeds = parallel.chain_seeds(s, 0, B, 0).numpy()
    v, pairs = _momenta(seeds, n)
    N = v.size
    # Kolmogorov-Smirnov distance to the normal distribution function
    x = np.sort(v.ravel())
    cdf = torch.special.ndtr(torch.from_numpy(x)).numpy()
    i = np.arange(1, N + 1)
    D = max(float((i / N - cdf).max()), float((cdf - (i - 1) / N).max()))
    bound = math.sqrt(math.log(2 / 1e-9) / (2 * N))
    print(f'KS {D:.3e} (bound {bound:.3e})')
    assert D < bound
    z = {'mean': _z(v), 'variance': _z(v ** 2 - 1, 2.0), 'third moment': _z(v ** 3, 15.0), 'fourth moment': _z(v ** 4 - 3, 96.0),
         'inside a Box-Muller pair': _z(pairs[..., 0] * pairs[..., 1]),
         'lag 1': _z(v[:, :-1] * v[:, 1:]),
         'chain b and b + 1': _z(v[:-1] * v[1:])}
    v1, _ = _momenta(parallel.chain_seeds(s, 0, B, 1).numpy(), n)
    z['trajectory t and t + 1'] = _z(v * v1)
    u = PR.accept_u(PR.accept_bits(seeds))
    z['u[b] and v[b, 0]'] = _z((u - 0.5) * v[:, 0], 1.0 / 12)
    xi = PR.accept_u(PR.uniform_bits(seeds, n))                              # the prior on (0, 1)
    z['momenta plane and prior plane'] = _z((xi - 0.5) * v, 1.0 / 12)
    z['prior mean'] = _z(xi - 0.5, 1.0 / 12)
    z['accept uniform mean'] = _z(u - 0.5, 1.0 / 12)
    print({k: round(val, 2) for k, val in z.items()})
    for name, val in z.items():
        assert abs(val) < 6, (name, val)
    assert np.abs(v).max() <= math.sqrt(2 * 53 * math.log(2))


def test_the_three_counter_planes_are_disjoint():
    """momenta (p, 0, 0, 0), accept (0, 0, 1, 0), prior (p, 0, 2, 0): no counter is shared, so no draw reuses a block; with the
    planes swapped (the accept uniform taken from the momenta's block 0) u would be a function of v[0]"""
    seeds = parallel.chain_seeds(1331, 0, 64, 0).numpy()
    k1, _ = PR.momenta_bits(seeds, 8)
    ka = PR.accept_bits(seeds)
    kp = PR.uniform_bits(seeds, 8)
    assert not np.any(ka == k1[:, 0]) and not np.any(ka == kp[:, 0]) and not np.any(kp[:, 0] == k1[:, 0])
    # a chain's stream is a function of its seed alone: any subset, any order
    perm = np.random.default_rng(3).permutation(64)
    assert np.array_equal(PR.momenta_bits(seeds[perm], 8)[0], k1[perm])
    assert np.array_equal(PR.uniform_bits(seeds[5:9], 8), kp[5:9])
    # an odd n is the even n + 1 cut short
    assert np.array_equal(PR.uniform_bits(seeds, 7), kp[:, :7])


# ----------------------------------------------------------------------------------------------------------- chain seeds
def test_chain_seeds_are_distinct_non_negative_and_shardable():
    """parallel.chain_seeds over the bench's four seeds, chains < 1024 and trajectories < 2048: 8 388 608 distinct non-negative
    values; shards of a chain range are slices of the whole"""
    allv = np.empty((len(BENCH_SEEDS), 2048, 1024), dtype=np.int64)
    for si, s in enumerate(BENCH_SEEDS):
        for t in range(2048):
            allv[si, t] = parallel.chain_seeds(s, 0, 1024, t).numpy()
    assert allv.min() >= 0
    assert np.unique(allv.ravel()).size == allv.size
    for s in BENCH_SEEDS:
        for t in (0, 1, 2047):
            full = allv[BENCH_SEEDS.index(s), t]
            for ws in (2, 3, 8):
                for r in range(ws):
                    lo, hi = parallel.shard_range(1024, r, ws)
                    assert np.array_equal(parallel.chain_seeds(s, lo, hi, t).numpy(), full[lo:hi])
