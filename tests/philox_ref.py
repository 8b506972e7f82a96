"""A definition of the project's random streams that owes nothing to the kernels: numpy, integer arithmetic and mpmath only.

Philox4x32-10 is the generator of Salmon, Moraes, Dror and Shaw (Random123, SC'11), restated here from its definition: four
32-bit counter words, two key words, ten rounds of two 32 x 32 -> 64 bit multiplications by the constants M0, M1, with the key
moved on by the Weyl constants W0, W1 between rounds.  tests/test_rng_reference.py pins it to Random123's known answers.

The streams (include/fthmc_hip.h: fthmc_random_momenta, fthmc_random_uniform), per chain seed s, key (s & 0xffffffff, s >> 32):
    momenta   pair p  = block at counter (p, 0, 0, 0): u1 from words (0, 1), u2 from words (2, 3), Box-Muller
    accept uniform    = block at counter (0, 0, 1, 0): words (0, 1)
    prior     pair p  = block at counter (p, 0, 2, 0): value 2 p from words (0, 1), value 2 p + 1 from words (2, 3)
Two words (hi, lo) give the 53-bit integer m = (hi << 32 | lo) >> 11; every draw is a function of k = m + 1 in [1, 2^53]:
    u53 = k / 2^53 in (0, 1]      accept u = 1 - k / 2^53 in [0, 1)      prior = round((1 - k / 2^53) w + lo), w = fl(hi - lo)
    normal pair = sqrt(-2 ln u1) (cos 2 pi u2, sin 2 pi u2)
The functions below return the integers k (exact) and build the values from them with more precision than fp64.

Not collected as a test (the name does not match test_*.py).
"""
from fractions import Fraction

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57           # Random123 PHILOX_M4x32_0, _1
W0, W1 = 0x9E3779B9, 0xBB67AE85           # Random123 PHILOX_W32_0, _1: golden ratio, sqrt(3) - 1
_MASK = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)
TWO53 = 1 << 53
LD = np.longdouble
# pi to the longdouble's 64 bits: the fp64 value plus the fp64 value of the remainder (their sum rounds once, to 64 bits)
PI_LD = LD(3.141592653589793) + LD(1.2246467991473532e-16)


# Random123's known answers for philox4x32 with 10 rounds (its kat_vectors): (counter, key, output)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def philox4x32_10(counter4, key2, rounds=10):
    """-> the four output words (uint64 arrays < 2^32) of the blocks at `counter4` under `key2`; every entry an integer or an
    array of integers, broadcast against each other, masked to 32 bits"""
    c = [np.asarray(x, dtype=np.uint64) & _MASK for x in counter4]
    k = [np.asarray(x, dtype=np.uint64) & _MASK for x in key2]
    for _ in range(rounds):
        p0 = np.uint64(M0) * c[0]                     # < 2^64: exact in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> _32) ^ c[1] ^ k[0], p1 & _MASK, (p0 >> _32) ^ c[3] ^ k[1], p0 & _MASK]
        k = [(k[0] + np.uint64(W0)) & _MASK, (k[1] + np.uint64(W1)) & _MASK]
    return c


def u53(hi, lo):
    """-> k = m + 1 with m = (hi << 32 | lo) >> 11, as uint64 (1 <= k <= 2^53); the value is k / 2^53 in (0, 1]"""
    hi = np.asarray(hi, dtype=np.uint64) & _MASK
    lo = np.asarray(lo, dtype=np.uint64) & _MASK
    return (((hi << _32) | lo) >> np.uint64(11)) + np.uint64(1)


def _key(seed):
    s = np.asarray(seed).astype(np.uint64)            # int64 seeds keep their bit pattern
    return s & _MASK, s >> _32


def momenta_bits(seed, n):
    """-> (k1, k2), each [..., (n + 1) // 2]: the integers behind u1 and u2 of every Box-Muller pair of a chain of n momenta;
    seed: one integer or an array of them (leading axes of the result)"""
    k0, k1 = _key(seed)
    p = np.arange((n + 1) // 2, dtype=np.uint64)
    r = philox4x32_10((p, 0, 0, 0), (k0[..., None], k1[..., None]))
    return u53(r[0], r[1]), u53(r[2], r[3])


def accept_bits(seed):
    """-> k of the chain's Metropolis uniform (shape of seed)"""
    k0, k1 = _key(seed)
    r = philox4x32_10((0, 0, 1, 0), (k0, k1))
    return u53(r[0], r[1])


def uniform_bits(seed, n):
    """-> k [..., n] of the chain's n prior values"""
    k0, k1 = _key(seed)
    p = np.arange((n + 1) // 2, dtype=np.uint64)
    r = philox4x32_10((p, 0, 2, 0), (k0[..., None], k1[..., None]))
    a, b = u53(r[0], r[1]), u53(r[2], r[3])
    return np.stack([a, b], axis=-1).reshape(a.shape[:-1] + (2 * a.shape[-1],))[..., :n]


# ------------------------------------------------------------------------------------------------------------ exact values
def accept_u(k):
    """1 - k / 2^53, exact in fp64: 2^53 - k is an integer in [0, 2^53)"""
    t = np.uint64(TWO53) - np.asarray(k, dtype=np.uint64)
    return t.astype(np.float64) * 2.0 ** -53


def uniform_exact(k, lo, hi):
    """round_to_nearest((1 - k / 2^53) w + lo), w = fl(hi - lo), one value at a time in exact rational arithmetic
    (float(Fraction) rounds correctly)"""
    lo, hi = float(lo), float(hi)
    w, fl = Fraction(hi - lo), Fraction(lo)
    k = np.asarray(k, dtype=np.uint64)
    out = np.array([float(Fraction(TWO53 - int(v), TWO53) * w + fl) for v in k.ravel()], dtype=np.float64)
    return out.reshape(k.shape)


def uniform(k, lo, hi):
    """uniform_exact for bulk: the value in longdouble (64-bit significand: t = 1 - k / 2^53 and w are exact there, the product
    and the sum round once each, each within 2^-64 of the largest magnitude S in play: error <= 2^-63 S), rounded to fp64; every
    element whose longdouble value lies within 2^-62 S of a point where the fp64 rounding changes -- the midpoint of two fp64
    neighbours, in either binade at a power of two -- or whose fp64 spacing is not far above that error (results near 0) is
    redone with uniform_exact."""
    lo, hi = float(lo), float(hi)
    w = hi - lo
    k = np.asarray(k, dtype=np.uint64)
    t = (np.uint64(TWO53) - k).astype(LD) * LD(2.0) ** -53
    r = t * LD(w) + LD(lo)
    out = r.astype(np.float64)
    tol = LD(2.0) ** -62 * LD(max(abs(lo), abs(hi), abs(w)))
    d = np.abs(r - out.astype(LD))
    h = (np.abs(np.spacing(out)) / 2).astype(LD)
    redo = (np.abs(d - h) <= tol) | (np.abs(d - h / 2) <= tol) | (h <= 4 * tol)
    if redo.any():
        out[redo] = uniform_exact(k[redo], lo, hi)
    return out


def normal_pair_ld(k1, k2):
    """-> (rad cos, rad sin, rad) in longdouble: rad = sqrt(-2 ln(k1 / 2^53)), angle 2 pi k2 / 2^53 with pi to 64 bits"""
    u1 = np.asarray(k1, dtype=np.uint64).astype(LD) * LD(2.0) ** -53
    u2 = np.asarray(k2, dtype=np.uint64).astype(LD) * LD(2.0) ** -53
    rad = np.sqrt(LD(-2.0) * np.log(u1))
    ang = (LD(2.0) * PI_LD) * u2
    return rad * np.cos(ang), rad * np.sin(ang), rad


def normal_pair_mp(k1, k2):
    """-> (rad cos, rad sin, rad) as mpmath numbers at the caller's precision, from exact rationals and mpmath's pi"""
    import mpmath
    u1 = mpmath.mpf(int(k1)) / TWO53
    u2 = mpmath.mpf(int(k2)) / TWO53
    rad = mpmath.sqrt(-2 * mpmath.log(u1))
    ang = 2 * mpmath.pi * u2
    return rad * mpmath.cos(ang), rad * mpmath.sin(ang), rad


def momenta_ld(seed, n):
    """-> (v [..., n] in longdouble, rad [..., n]: the radius of each element's pair): the chain's momenta"""
    k1, k2 = momenta_bits(seed, n)
    a, b, rad = normal_pair_ld(k1, k2)
    v = np.stack([a, b], axis=-1).reshape(a.shape[:-1] + (2 * a.shape[-1],))[..., :n]
    r = np.stack([rad, rad], axis=-1).reshape(v.shape[:-1] + (2 * rad.shape[-1],))[..., :n]
    return v, r


def words_of(k):
    """-> (hi, lo) 32-bit words (uint32) whose u53 integer is k, low 11 bits zero: the inverse the edge tests feed the probe"""
    m = (np.asarray(k, dtype=np.uint64) - np.uint64(1)) << np.uint64(11)
    return (m >> _32).astype(np.uint32), (m & _MASK).astype(np.uint32)
