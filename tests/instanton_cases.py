"""The numpy side of the instanton-hit tests (tests/test_instanton.py, tests/test_instanton_gpu.py): a twin of fthmc_amd/csrc/topo.hip --
every formula of the device evaluated in np.longdouble (or, for the check of the bound itself, in float64), its draws through
tests/philox_ref.py -- with the error bounds derived below, the instanton configuration itself for the checks of the closed form,
and the fields and shapes both test files use.

Conventions (include/fthmc_hip.h): x[B][2][L][L], P(i,j) = x0[i][j] + x1[i+1][j] - x0[i][j+1] - x1[i][j], V = L^2, w = 2 pi / V.
    instanton of charge 1    A1[i][j] = w i,   A0[L-1][j] = -(2 pi / L) j,   A0[i][j] = 0 for i < L - 1:   every P moves by w,
                             the one at (L-1, L-1) by w - 2 pi
    sums                     C = sum cos P, Sn = sum sin P of the field a call received, added in the device's order (chain_sum)
    step h of a call         (u, s) = Philox block at counter (hit0 + h, 0, 4, 0): u = 1 - u53(words 0, 1), s = +1 where bit 0 of
                             word 2 is set, else -1;  theta = fl(fl(((2 k + s) mod 2 V) pi) / V);  sh = sin(fl(pi / V));
                             dS = s ((2 beta) sh) (C sin theta + Sn cos theta);  accepted iff u < exp(-dS);  then k += s
    the net charge k         x1[i][j] <- reg(x1[i][j] + fl(fl(2 pi ((k i) mod V)) / V)),  x0[L-1][j] <- reg(x0[L-1][j] - fl(fl(2 pi
                             ((k j) mod L)) / L));  a link whose reduced integer is 0 is copied
The twin is the exact-arithmetic reading of these formulas with the DEVICE's constants (pi as the double 3.141592653589793): what is
left between it and the device is rounding, which `hits` bounds (its docstring).

Not collected as a test (the name does not match test_*.py)."""
import functools
import math

import numpy as np

import local_update_cases as LC
import philox_ref as PR

LD = np.longdouble
U = LC.U
PI_D = LC.PI_D
SHAPES = LC.SHAPES
# (B, L, field amplitude, beta) of the device tests: LC.SHAPES at amplitude pi, a wide field (the sincos guard is not reached at 50:
# |P| <= 200; the reductions of large angles are), a smooth one at the beta of the headline workload as well
CASES = tuple((B, L, math.pi, 2.0) for B, L in SHAPES) + ((2, 20, 50.0, 2.0), (2, 20, 0.3, 2.0), (2, 20, 0.3, 6.0))
# (n_hit, hit0) of the device tests; the last: one hit at the last index of the counter word
HITS = ((1, 0), (5, 7), (64, 2 ** 32 - 64), (1, 2 ** 32 - 1))


def chain_threads(L):
    """csrc/kernels.h: the workgroup of a chain"""
    return 1024 if L * L >= 4096 else (512 if L * L >= 1024 else 256)


def fields(B, L, amp):
    x = LC.uniform_links(B, L, 1000 + L, amp)
    seeds = LC.chain_seeds(B, 3000 + L)
    x.setflags(write=False); seeds.setflags(write=False)
    return x, seeds


def plaquette_terms(x, dt=LD):
    """-> (P, roundoff weight): P in the device's order of operations ((x0 + x1[i+1]) - x0[j+1]) - x1, and |s1| + |s2| + |P| of its
    three partial sums: the three roundings of the device cost at most u times it"""
    x0, x1 = x[:, 0].astype(dt), x[:, 1].astype(dt)
    s1 = x0 + np.roll(x1, -1, axis=-2)
    s2 = s1 - np.roll(x0, -1, axis=-1)
    P = s2 - x1
    return P, (np.abs(s1) + np.abs(s2) + np.abs(P)).astype(np.float64)


def chain_sum(v, L):
    """the sum of v[B, V] over the sites in the device's order: thread t of the chain's workgroup adds sites t, t + nt, ... from 0.0,
    a wave adds its 64 lanes by the xor butterfly (offsets 32 .. 1), the waves' sums are added to 0.0 in order.  (Waves that hold
    no site add exact zeros and are left out.)  -> (sum [B], depth: the additions on the longest path)"""
    B, n = v.shape
    nt = chain_threads(L)
    nt_used = min(nt, (n + 63) // 64 * 64)
    m = (n + nt - 1) // nt
    pad = np.zeros((B, m * nt), dtype=v.dtype)
    pad[:, :n] = v
    rows = pad.reshape(B, m, nt)[:, :, :nt_used]
    acc = np.zeros((B, nt_used), dtype=v.dtype)
    for r in range(m):
        acc = acc + rows[:, r]
    w = acc.reshape(B, nt_used // 64, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, :, lane ^ o]
    tot = np.zeros(B, dtype=v.dtype)
    for i in range(nt_used // 64):
        tot = tot + w[:, i, 0]
    return tot, m + 6 + nt // 64


def sums(x, dt=LD, chunk=4096):
    """-> (C, Sn, dC, dSn) per chain: the two sums in `dt` and the bounds of the device's error of each (see `hits`)"""
    B, _, L, _ = x.shape
    out = [np.zeros(B, dtype=dt), np.zeros(B, dtype=dt), np.zeros(B), np.zeros(B)]
    for lo in range(0, B, chunk):
        P, wt = plaquette_terms(x[lo:lo + chunk], dt)
        P = P.reshape(P.shape[0], -1); dP = U * wt.reshape(P.shape)
        cs, sn = np.cos(P), np.sin(P)
        C, depth = chain_sum(cs, L)
        S, _ = chain_sum(sn, L)
        c64, s64 = np.abs(cs.astype(np.float64)), np.abs(sn.astype(np.float64))
        out[0][lo:lo + chunk], out[1][lo:lo + chunk] = C, S
        out[2][lo:lo + chunk] = (s64 * dP + 2.5 * U).sum(axis=1) + depth * U * c64.sum(axis=1)
        out[3][lo:lo + chunk] = (c64 * dP + 2.5 * U).sum(axis=1) + depth * U * s64.sum(axis=1)
    return tuple(out)


def mod(a, m):
    """the mathematical remainder in Python integers / int64 arrays (numpy's % is it already)"""
    return np.mod(a, m)


def delta_s(C, Sn, beta, k, s, L, dt=LD, dC=0.0, dSn=0.0):
    """dS of the step k -> k + s in the device's order of operations -> (dS, bound of the device's error of it).  k, s: int64 arrays"""
    V = L * L
    num = mod(2 * np.asarray(k, dtype=np.int64) + np.asarray(s, dtype=np.int64), 2 * V)
    if num.size > 4 * V:                             # many chains of a small lattice: theta takes 2 V values, each formed once
        tab = (np.arange(2 * V).astype(dt) * dt(PI_D)) / dt(V)
        th, st, ct = tab[num], np.sin(tab)[num], np.cos(tab)[num]
    else:
        th = (num.astype(dt) * dt(PI_D)) / dt(V)
        st, ct = np.sin(th), np.cos(th)
    sh = np.sin(dt(PI_D) / dt(V))
    pref = (dt(2) * np.asarray(beta, dtype=dt)) * sh
    a, b = np.asarray(C, dtype=dt) * st, np.asarray(Sn, dtype=dt) * ct
    t = a + b
    d = pref * t
    f = lambda v: np.abs(np.asarray(v).astype(np.float64))
    dth = 2 * U * f(th)
    dst, dct = f(ct) * dth + 2.5 * U, f(st) * dth + 2.5 * U
    dt_ = f(st) * dC + f(C) * dst + f(ct) * dSn + f(Sn) * dct + U * (f(a) + f(b)) + U * f(t)
    # sh: the quotient pi / V (u, relative), ft_sincos within 2.5 ulp of a result whose ulp is at most 2 u of it: 6 u; the products
    # (2 beta) sh and pref t one rounding each
    bound = f(pref) * dt_ + 8 * U * f(d)
    return np.where(np.asarray(s) > 0, d, -d), bound


def shift_x1(k, L, dt=LD, reduced=True):
    """the shift of x1[i][:] under the net charge k [B] -> ([B, L] in dt, the reduced integers [B, L])"""
    V = L * L
    ki = np.asarray(k, dtype=np.int64)[:, None] * np.arange(L, dtype=np.int64)[None, :]
    r = mod(ki, V)
    num = r if reduced else ki
    return (dt(2 * PI_D) * num.astype(dt)) / dt(V), r


def shift_seam(k, L, dt=LD, reduced=True):
    """the (positive) amount taken from x0[L-1][j] under the net charge k [B] -> ([B, L], the reduced integers)"""
    kj = np.asarray(k, dtype=np.int64)[:, None] * np.arange(L, dtype=np.int64)[None, :]
    r = mod(kj, L)
    num = r if reduced else kj
    return (dt(2 * PI_D) * num.astype(dt)) / dt(L), r


def apply_charge(x, k, dt=LD):
    """x + k A as the device forms it -> (new links [B, 2, L, L] in dt, moved [B, 2, L, L] bool, bound [B, 2, L, L]: the device's
    error of a moved link on the circle: the shift fl(fl(2 pi r) / n) is itself rounded twice, 2 u |shift|, BEFORE it is added --
    a term u (|x| + |shift|) alone would cover only the rounding of the sum, |y| <= |x| + |shift| -- so dy = 3 u |shift| + u |x|;
    then LC._reg_err; 0 for a copied link)"""
    B, _, L, _ = x.shape
    xn = x.astype(dt)
    moved = np.zeros(x.shape, dtype=bool)
    bound = np.zeros(x.shape)
    s1, r1 = shift_x1(k, L, dt)
    ss, rs = shift_seam(k, L, dt)
    y1 = xn[:, 1] + s1[:, :, None]
    ys = xn[:, 0, L - 1] - ss
    m1 = np.broadcast_to((r1 != 0)[:, :, None], (B, L, L))
    xn[:, 1] = np.where(m1, LC.regularize(y1, dt), xn[:, 1])
    xn[:, 0, L - 1] = np.where(rs != 0, LC.regularize(ys, dt), xn[:, 0, L - 1])
    moved[:, 1] = m1
    moved[:, 0, L - 1] = rs != 0
    f = lambda v: np.abs(np.asarray(v).astype(np.float64))
    b1 = LC._reg_err(y1.astype(np.float64), 3 * U * f(s1)[:, :, None] + U * f(x[:, 1]))
    bs = LC._reg_err(ys.astype(np.float64), 3 * U * f(ss) + U * f(x[:, 0, L - 1]))
    bound[:, 1] = np.where(m1, 1.01 * b1, 0.0)
    bound[:, 0, L - 1] = np.where(rs != 0, 1.01 * bs, 0.0)
    return xn, moved, bound


def draws(seeds, n_hit, hit0):
    """-> (u [B, n_hit] float64, exact; s [B, n_hit] int64)"""
    k0, k1 = PR._key(seeds)
    h = (np.uint64(hit0) + np.arange(n_hit, dtype=np.uint64))[None, :]
    w = PR.philox4x32_10((h, 0, 4, 0), (k0[:, None], k1[:, None]))
    u = PR.accept_u(PR.u53(w[0], w[1]))
    s = np.where((w[2] & np.uint64(1)) == 1, 1, -1).astype(np.int64)
    return u, s


def hits(x, beta, seeds, n_hit, hit0=0, dt=LD, pre=None):
    """The whole call of the device for every chain of x [B, 2, L, L] (float64): beta a number or [B] -> dict with
        C, Sn [B] in dt;  dC, dSn [B]: their bounds
        s, u, dS, accepted [B, n_hit]: the steps;  dS_bound [B, n_hit]
        k, nacc [B] int64
        x [B, 2, L, L] in dt, moved, bound: apply_charge of the k the steps end with
        margin [B]: the smallest |u - exp(-dS)| of the chain's decisions;  ambiguous [B]: a decision closer than its bound
    The derived bound (against a device that computes in fp64 with correctly rounded + - * /, ft_sincos within 2.5 u absolute, the
    library's exp within 2 u relative, u = 2^-53; first order, 1 % on top for the second):
      * P: three roundings, each at most u times its partial sum: dP = u (|s1| + |s2| + |P|);
      * cos P: |sin P| dP + 2.5 u, sin P: |cos P| dP + 2.5 u;
      * the sums: every term's own error, plus depth u sum |term| for the additions (depth: the longest path of chain_sum: a
        thread's sites, six butterfly levels, the waves);
      * theta: two roundings, 2 u theta; its sine and cosine as above; sh = sin(pi / V) within 6 u of itself;
      * dS = ((2 beta) sh) (C sin theta + Sn cos theta): the partial derivatives times the bounds above, u per product and sum;
      * exp(-dS): e (dS_bound + 2 u); a decision is safe when |u - e| exceeds 1.01 times that (u itself is exact);
      * a moved link: apply_charge."""
    x = np.asarray(x, dtype=np.float64)
    B, _, L, _ = x.shape
    beta_b = np.broadcast_to(np.asarray(beta, dtype=np.float64).reshape(-1), (B,))
    C, Sn, dC, dSn = sums(x, dt) if pre is None else pre              # pre: sums(x, dt) formed earlier (case)
    k = np.zeros(B, dtype=np.int64)
    nacc = np.zeros(B, dtype=np.int64)
    margin = np.full(B, np.inf)
    ambiguous = np.zeros(B, dtype=bool)
    n_hit = int(n_hit)
    steps = {key: np.zeros((B, n_hit), dtype=t) for key, t in (('s', np.int64), ('u', np.float64), ('dS', dt), ('accepted', bool), ('dS_bound', np.float64))}
    if n_hit:
        u, s = draws(seeds, n_hit, hit0)
        for h in range(n_hit):
            dS, bd = delta_s(C, Sn, beta_b, k, s[:, h], L, dt, dC, dSn)
            with np.errstate(over='ignore'):
                e = np.exp(-dS)
            acc = u[:, h].astype(dt) < e
            e64 = np.minimum(e.astype(np.float64), 1e300)
            mg = np.abs(u[:, h] - e64)
            margin = np.minimum(margin, mg)
            ambiguous |= mg <= 1.01 * e64 * (bd + 2 * U)
            k = k + np.where(acc, s[:, h], 0)
            nacc = nacc + acc
            for key, val in (('s', s[:, h]), ('u', u[:, h]), ('dS', dS), ('accepted', acc), ('dS_bound', bd)):
                steps[key][:, h] = val
    xn, moved, bound = apply_charge(x, k, dt)
    out = dict(C=C, Sn=Sn, dC=1.01 * dC, dSn=1.01 * dSn, k=k, nacc=nacc, x=xn, moved=moved, bound=bound, margin=margin, ambiguous=ambiguous)
    out.update(steps)
    return out


@functools.lru_cache(maxsize=None)
def case(B, L, amp, beta, n_hit, hit0):
    """(links, seeds, the twin's call) of a device case: computed once, shared by every test that needs it, never written.
    tests/test_instanton.py checks on the CPU that the twin leaves no chain of these out."""
    x, seeds = fields(B, L, amp)
    return x, seeds, hits(x, beta, seeds, n_hit, hit0, pre=_field_sums(B, L, amp))


@functools.lru_cache(maxsize=None)
def _field_sums(B, L, amp):
    """sums() of a case's field: one reduction for all of its (n_hit, hit0), as on the device"""
    return sums(fields(B, L, amp)[0])


# ---------------------------------------------------------------- the instanton itself, for the checks of the closed form
def instanton(L, dt=LD):
    """A [2, L, L] of charge 1 in dt, unreduced"""
    A = np.zeros((2, L, L), dtype=dt)
    A[1] = (dt(2 * PI_D) / dt(L * L)) * np.arange(L, dtype=dt)[:, None]
    A[0, L - 1] = -(dt(2 * PI_D) / dt(L)) * np.arange(L, dtype=dt)
    return A


def action_sum(x):
    """sum cos P per chain, np.longdouble, of a field of any float type"""
    x = np.asarray(x, dtype=LD)
    P = x[:, 0] + np.roll(x[:, 1], -1, axis=-2) - np.roll(x[:, 0], -1, axis=-1) - x[:, 1]
    return np.cos(P).reshape(x.shape[0], -1).sum(axis=1)


def charge(x):
    """Q = sum wrap(P) / 2 pi per chain in np.longdouble (the circle of circumference 2 FT_PI) -> (rounded int64, distance from it)"""
    x = np.asarray(x, dtype=LD)
    P = x[:, 0] + np.roll(x[:, 1], -1, axis=-2) - np.roll(x[:, 0], -1, axis=-1) - x[:, 1]
    w = P - LD(2 * PI_D) * np.floor((P + LD(PI_D)) / LD(2 * PI_D))
    q = w.reshape(x.shape[0], -1).sum(axis=1) / LD(2 * PI_D)
    qi = np.rint(q)
    return qi.astype(np.int64), np.abs(q - qi).astype(np.float64)


def path_delta_s(C, Sn, beta, k, L, dt=LD, dC=0.0, dSn=0.0):
    """the closed form summed over the |k| steps 0 -> k, one unit at a time -> (dS [B], bound [B])"""
    s = 1 if k > 0 else -1
    tot, bd = np.zeros(np.shape(C), dtype=dt), np.zeros(np.shape(C))
    for j in range(abs(int(k))):
        kk = np.full(np.shape(C), s * j, dtype=np.int64)
        d, b = delta_s(C, Sn, beta, kk, np.full(np.shape(C), s, dtype=np.int64), L, dt, dC, dSn)
        tot, bd = tot + d, bd + b
    return tot, bd
