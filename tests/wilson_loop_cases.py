"""The numpy side of the Wilson-loop tests (tests/test_wilson_loops.py, tests/test_wilson_loops_gpu.py): the oracle in
np.longdouble by direct sums, a second oracle that walks every loop link by link, a float64 twin of the device algorithm
(fthmc_amd/csrc/loops.hip), the derived error bound, and the fields both test files use.

Conventions (include/fthmc_hip.h): x[B][2][L][L]; x0[i][j] points along i, x1[i][j] along j; the R x T loop with corner (i, j) has
    theta = sum_{a<R} x0[i+a][j] + sum_{c<T} x1[i+R][j+c] - sum_{a<R} x0[i+a][j+T] - sum_{c<T} x1[i][j+c]     (indices mod L)
and W[b][R-1][T-1] = mean over (i, j) of cos theta."""
import math

import numpy as np

U = 2.0 ** -53
# (B, L, Rmax, Tmax) of the device-table test: wrap in each direction, ragged and non-power-of-two L, several row blocks, more
# chains than one grid row of 128, Rmax != Tmax
SHAPES = ((3, 8, 8, 8), (2, 12, 12, 5), (2, 20, 7, 20), (2, 64, 64, 9), (2, 64, 9, 64), (1, 128, 5, 128), (130, 16, 4, 4))


def uniform_links(B, L, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-math.pi, math.pi, (B, 2, L, L))


def known_answer_field(L, k, B=1):
    """x0[i][j] = -(2 pi k / L) j, x1 = 0: W(R, T) = cos(2 pi k R T / L)"""
    x = np.zeros((B, 2, L, L))
    x[:, 0] = -(2.0 * math.pi * k / L) * np.arange(L)[None, None, :]
    return x


def known_answer(L, k, Rmax, Tmax):
    R, T = np.arange(1, Rmax + 1)[:, None], np.arange(1, Tmax + 1)[None, :]
    return np.cos(2.0 * math.pi * k * R * T / L)


def gauge_transform(x, alpha):
    """x_mu(n) -> x_mu(n) + alpha(n) - alpha(n + mu)"""
    y = np.array(x, dtype=np.float64, copy=True)
    y[:, 0] += alpha - np.roll(alpha, -1, axis=-2)
    y[:, 1] += alpha - np.roll(alpha, -1, axis=-1)
    return y


def loops_ref(x, Rmax, Tmax):
    """[B, Rmax, Tmax] in np.longdouble: the four sides as sums of rolled planes"""
    x = np.asarray(x, dtype=np.longdouble)
    B, _, L, _ = x.shape
    x0, x1 = x[:, 0], x[:, 1]
    W = np.zeros((B, Rmax, Tmax), dtype=np.longdouble)
    a0 = np.zeros_like(x0)
    for R in range(1, Rmax + 1):
        a0 = a0 + np.roll(x0, -(R - 1), axis=-2)                 # sum_{a<R} x0[i+a][j]
        a1 = np.zeros_like(x1)
        for T in range(1, Tmax + 1):
            a1 = a1 + np.roll(x1, -(T - 1), axis=-1)             # sum_{c<T} x1[i][j+c]
            theta = a0 + np.roll(a1, -R, axis=-2) - np.roll(a0, -T, axis=-1) - a1
            W[:, R - 1, T - 1] = np.cos(theta).reshape(B, -1).mean(axis=1)
    return W


def loops_walk(x, Rmax, Tmax):
    """the same table by walking every loop link by link around its perimeter (shares no indexing code with loops_ref)"""
    x = np.asarray(x, dtype=np.longdouble)
    B, _, L, _ = x.shape
    W = np.zeros((B, Rmax, Tmax), dtype=np.longdouble)
    for b in range(B):
        l0, l1 = x[b, 0], x[b, 1]
        for R in range(1, Rmax + 1):
            for T in range(1, Tmax + 1):
                tot = np.longdouble(0)
                for i in range(L):
                    for j in range(L):
                        p, q, th = i, j, np.longdouble(0)
                        for _ in range(R):
                            th += l0[p, q]; p = (p + 1) % L          # forward along i
                        for _ in range(T):
                            th += l1[p, q]; q = (q + 1) % L          # forward along j
                        for _ in range(R):
                            p = (p - 1) % L; th -= l0[p, q]          # back along i
                        for _ in range(T):
                            q = (q - 1) % L; th -= l1[p, q]          # back along j
                        assert (p, q) == (i, j)
                        tot += np.cos(th)
                W[b, R - 1, T - 1] = tot / (L * L)
    return W


def polyakov_correlator_ref(x, Rmax):
    """< P(i) P*(i + R) > averaged over i (and over nothing else: P does not depend on j) from the column phases, longdouble"""
    x = np.asarray(x, dtype=np.longdouble)
    ph = x[:, 1].sum(axis=-1)                                    # [B, L]: the angle of P(i)
    return np.stack([np.cos(np.roll(ph, -R, axis=-1) - ph).mean(axis=-1) for R in range(1, Rmax + 1)], axis=1)


# ---------------------------------------------------------------- the device algorithm in float64 numpy
def _two_sum_prefix(x0):
    """S[..., i, j] = sum_{a<i} x0[..., a, j], i = 0 .. L, the running sum as hi + lo (k_link_prefix)"""
    L = x0.shape[-2]
    S = np.zeros(x0.shape[:-2] + (L + 1, x0.shape[-1]))
    hi = np.zeros(x0.shape[:-2] + (x0.shape[-1],)); lo = np.zeros_like(hi)
    for i in range(L):
        v = x0[..., i, :]
        t = hi + v; bv = t - hi
        lo = lo + ((hi - (t - bv)) + (v - bv))
        hi = t
        S[..., i + 1, :] = hi + lo
    return S


def loops_twin64(x, Rmax, Tmax):
    """fthmc_amd/csrc/loops.hip in float64 numpy: compensated prefix sums, segment sums from two (three) of them, E and d by one
    sin / cos each, the walk G_{T+1} = G_T d(j + T), W_T = Re[G_T conj(E(j + T))] with the kernel's expressions; only the order of
    the final sum over sites (and the sincos implementation) differs from the device"""
    x = np.asarray(x, dtype=np.float64)
    B, _, L, _ = x.shape
    x0, x1 = x[:, 0], x[:, 1]
    S = _two_sum_prefix(x0)
    W = np.zeros((B, Rmax, Tmax))
    ii = np.arange(L)
    for R in range(1, Rmax + 1):
        e = ii + R
        nowrap = (S[:, np.minimum(e, L)] - S[:, ii])
        wrapped = (S[:, L][:, None, :] - S[:, ii]) + S[:, np.maximum(e - L, 0)]
        seg = np.where((e <= L)[None, :, None], nowrap, wrapped)
        Er, Ei = np.cos(seg), np.sin(seg)
        dang = x1[:, (ii + R) % L] - x1
        dr, di = np.cos(dang), np.sin(dang)
        gr, gi = Er * dr - Ei * di, Er * di + Ei * dr
        for T in range(1, Tmax + 1):
            e2r, e2i = np.roll(Er, -T, axis=-1), np.roll(Ei, -T, axis=-1)
            dnr, dni = np.roll(dr, -T, axis=-1), np.roll(di, -T, axis=-1)
            W[:, R - 1, T - 1] = (gr * e2r + gi * e2i).reshape(B, -1).sum(axis=1) / float(L * L)
            gr, gi = gr * dnr - gi * dni, gr * dni + gi * dnr
    return W


# ---------------------------------------------------------------- error bounds
def mu_of(x):
    return max(1.0, float(np.abs(np.asarray(x, dtype=np.float64)).max()) / math.pi)


def issue_bound(L, R, T, mu):
    """the ceiling no tolerance may exceed: worst-case recursive prefix sums of L angles plus products of R + T unit phases"""
    return U * (2.0 * math.pi * L * L + 8.0 * (R + T) + 16.0) * mu


def n_partials(L):
    """partials per (chain, R) the device adds in order (loops_geom, csrc/kernels.h)"""
    if L <= 1024:
        rows = min(L, max(1, 1024 // L))
        return -(-L // rows)
    return L * (-(-L // 1024))


def derived_bound(L, R, T, mu):
    """Worst-case |W_device - W_exact| of one entry for links of magnitude <= pi mu, u = 2^-53, for the arithmetic of loops.hip:
      * a stored prefix S[k] carries ONE rounding of a sum of magnitude <= k pi mu (the running sum is a two-sum pair);
        a segment sum is fl(S[i+R] - S[i]): prefix errors (i + R + i) pi mu u, the difference's rounding R pi mu u, together
        <= 2 L pi mu u; a wrapping one, fl(fl(S[L] - S[i]) + S[i+R-L]): <= (2 L + (i+R-L) + R) pi mu u <= 4 L pi mu u;
      * E = (cos, sin) of it, each component within 2.5 ulp <= 2.5 u (common.h ft_sincos): |dE| <= (4 pi L mu + 2.5 sqrt 2) u;
      * d = (cos, sin)(fl(x1[i+R][j] - x1[i][j])): the difference's rounding <= 2 pi mu u, |dd| <= (2 pi mu + 2.5 sqrt 2) u;
      * T complex products of unit-modulus numbers (G_1 = E d, G_{c+1} = G_c d), each within sqrt 5 u < 3 u relative;
      * Re[G conj(E')]: two operations, <= 2 u; the entry involves E twice (columns j and j + T) and d T times:
            per site  [2 (4 pi L mu + 3.54) + T (2 pi mu + 3.54 + 3) + 2] u
      * the mean over L^2 sites of magnitude <= 1: four sites per thread, a 6-level wave tree, four waves, n_partials(L)
        partials in order, one division: (14 + n_partials(L)) u
    and 0.1 % on top for the second-order terms.  O(L) ulps where a plain recursive prefix sum would give O(L^2)."""
    site = 2.0 * (4.0 * math.pi * L * mu + 3.54) + T * (2.0 * math.pi * mu + 6.54) + 2.0
    return U * (site + 14.0 + n_partials(L)) * 1.001


def tolerance(L, Rmax, Tmax, mu):
    """[Rmax, Tmax] of per-entry tolerances: the derived bound, which must lie below the issue's ceiling"""
    tol = np.array([[derived_bound(L, R, T, mu) for T in range(1, Tmax + 1)] for R in range(1, Rmax + 1)])
    cap = np.array([[issue_bound(L, R, T, mu) for T in range(1, Tmax + 1)] for R in range(1, Rmax + 1)])
    assert np.all(tol <= cap), (L, Rmax, Tmax, mu)
    return tol
