"""The numpy side of the local-update tests (tests/test_local_update.py, tests/test_local_update_gpu.py): a twin of ONE class update of
fthmc_amd/csrc/local.hip -- every formula of the device evaluated in np.longdouble (or, for the check of the bound itself, in
float64), its draws through tests/philox_ref.py -- with the per-link error bound derived below, a sampler made of it, and the fields
and shapes both test files use.

Conventions (include/fthmc_hip.h): x[B][2][L][L], P(i,j) = x0[i][j] + x1[i+1][j] - x0[i][j+1] - x1[i][j]; a link's conditional weight is
exp(kappa cos(x - phi)), kappa = beta |A|, phi = -arg A, A = exp(i a) + exp(-i b) = 2 cos h exp(i (a - b) / 2), h = (a + b) / 2:
    x0[i][j]:  a = x1[i+1][j] - x0[i][j+1] - x1[i][j],        b = x0[i][j-1] + x1[i+1][j-1] - x1[i][j-1]
    x1[i][j]:  a = -(x0[i][j] + x1[i+1][j] - x0[i][j+1]),     b = -(x0[i-1][j] - x0[i-1][j+1] - x1[i-1][j])
    kappa = 2 beta |cos h|,   phi = (b - a) / 2 (+ pi where cos h < 0)
    overrelaxation  x <- reg((b - a) - x)                      reg(f) = 2 pi (g - floor(g) - 1/2), g = (f - pi) / 2 pi
    heatbath        tau = 1 + sqrt(1 + 4 kappa^2), rho = 2 kappa / (tau + sqrt(2 tau)), r = (1 + rho^2) / (2 rho); per attempt t < 64:
                    z = cos(pi u1), f = clamp((1 + r z) / (r + z)), c = kappa (r - f); accept when c (2 - c) - u2 > 0 or
                    log(c / u2) + 1 - c >= 0; then x <- reg(phi +- acos f).  kappa < 2^-60: f = z, accepted (the uniform limit).
                    (u1, u2, sign) = Philox block at counter (i L + j, sweep, 3, mu << 8 | t): words (0, 1), (2, 3), bit 0 of word 1
The twin is the exact-arithmetic reading of these formulas with the DEVICE's constants (pi as the double 3.141592653589793): what is
left between it and the device is rounding, which `derived_bound` (in class_update) bounds link by link.

Not collected as a test (the name does not match test_*.py)."""
import functools
import math

import numpy as np

import philox_ref as PR

LD = np.longdouble
U = 2.0 ** -53
PI_D = math.pi                       # FT_PI of csrc/common.h
KAPPA_MIN = 2.0 ** -60
MAX_ATTEMPTS = 64
CLASSES = ((0, 0), (0, 1), (1, 0), (1, 1))      # (mu, parity), the order of a sweep; class k is bit k of the mask
MARGIN_MIN = 1e-10                   # a chain with a closer accept decision is left out of a per-link comparison
# (B, L) of the device tests: a two-column class whose neighbours both wrap, ragged sizes, the last resident shape and the first
# class-kernel-only one, more chains than a grid row of 128, more chains than a 65 535 grid dimension
SHAPES = ((3, 4), (3, 8), (2, 12), (2, 20), (2, 64), (1, 68), (1, 128), (130, 16), (66000, 4))


def uniform_links(B, L, seed, amp=math.pi):
    rng = np.random.default_rng(seed)
    return rng.uniform(-amp, amp, (B, 2, L, L))


def chain_seeds(B, seed):
    """B int64 seeds (63 bits, as fthmc_chain_seeds hands them out)"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 2 ** 63 - 1, size=B, dtype=np.int64)


BETA = 2.0           # of the per-link comparisons
SWEEP = 3            # their heatbath-sweep index
CASES = tuple((B, L, math.pi) for B, L in SHAPES) + ((2, 20, 50.0),)      # (B, L, field amplitude)


@functools.lru_cache(maxsize=None)
def case(B, L, kind, amp=math.pi):
    """(links, seeds, the twin's four class updates at BETA, SWEEP) of a shape: computed once, shared by every test that needs it,
    never written.  tests/test_local_update.py checks on the CPU that the twin leaves no chain of these out."""
    x = uniform_links(B, L, 1000 + L, amp)
    seeds = chain_seeds(B, 2000 + L)
    x.setflags(write=False); seeds.setflags(write=False)
    return x, seeds, [class_update(x, mu, p, kind, BETA, seeds, SWEEP) for mu, p in CLASSES]


def class_links(L, mu, p):
    """-> (ii, jj), each [L^2 / 2]: the links of class (mu, p)"""
    i, j = np.meshgrid(np.arange(L), np.arange(L), indexing='ij')
    sel = ((j if mu == 0 else i) & 1) == p
    return i[sel], j[sel]


def regularize(f, dt=LD):
    g = (f - dt(PI_D)) / dt(2 * PI_D)
    return dt(2 * PI_D) * (g - np.floor(g) - dt(0.5))


def circ_dist(a, b):
    """distance of two angles on the circle of circumference 2 FT_PI, float64"""
    d = np.abs(np.asarray(a, dtype=LD) - np.asarray(b, dtype=LD)) % LD(2 * PI_D)
    return np.minimum(d, LD(2 * PI_D) - d).astype(np.float64)


def _reg_err(y, dy):
    """|reg_device(y~) - reg_exact(y)| on the circle for |y~ - y| <= dy: g = (y - pi) / 2 pi costs u |y - pi| (the subtraction) and
    u |g| (the division) besides the input; g - floor(g) is exact for g >= 0 and rounds once (<= u) below; - 1/2 rounds at most once
    (<= u); the product with 2 pi (<= pi in magnitude) once: u pi.  Together dy + u (2 |y - pi| + 4 pi + pi) <= dy + u (2 |y| + 22)."""
    return dy + U * (2.0 * np.abs(y) + 22.0)


def staples(x, mu, ii, jj, dt=LD):
    """-> (a, b, ta, tb): the staple angles of the links (mu, ii, jj) of every chain, in the device's order of operations, and the sums
    of the magnitudes of their three terms"""
    L = x.shape[-1]
    x0, x1 = x[:, 0].astype(dt), x[:, 1].astype(dt)
    ip, im, jp, jm = (ii + 1) % L, (ii - 1) % L, (jj + 1) % L, (jj - 1) % L
    if mu == 0:
        v = (x1[:, ip, jj], x0[:, ii, jp], x1[:, ii, jj], x0[:, ii, jm], x1[:, ip, jm], x1[:, ii, jm])
        a, b = (v[0] - v[1]) - v[2], (v[3] + v[4]) - v[5]
    else:
        v = (x0[:, ii, jj], x1[:, ip, jj], x0[:, ii, jp], x0[:, im, jj], x0[:, im, jp], x1[:, im, jj])
        a, b = -((v[0] + v[1]) - v[2]), -((v[3] - v[4]) - v[5])
    ta = (np.abs(v[0]) + np.abs(v[1]) + np.abs(v[2])).astype(np.float64)
    tb = (np.abs(v[3]) + np.abs(v[4]) + np.abs(v[5])).astype(np.float64)
    return a, b, ta, tb


def vonmises_draw(kappa, phi, seeds, site, mu, sweep, dt=LD, dkappa=None):
    """The heatbath draw of every entry of `kappa` / `phi` ([B, n]; seeds [B], site [n]) -> dict(theta = phi +- acos f BEFORE the
    regularisation, attempts (0: never accepted), margin = the smallest |margin| of the accept decisions taken, df = the bound on
    the device's error of acos f (see class_update), accepted)"""
    kappa = np.asarray(kappa, dtype=dt)
    B, n = kappa.shape
    k0, k1 = PR._key(seeds)
    k0 = np.broadcast_to(k0[:, None], (B, n)); k1 = np.broadcast_to(k1[:, None], (B, n))
    site = np.broadcast_to(np.asarray(site, dtype=np.uint64)[None, :], (B, n))
    flat = ~(kappa >= dt(KAPPA_MIN))
    ks = np.where(flat, dt(1), kappa)
    tau = dt(1) + np.sqrt(dt(1) + dt(4) * ks * ks)
    rho = dt(2) * ks / (tau + np.sqrt(dt(2) * tau))
    r = (dt(1) + rho * rho) / (dt(2) * rho)
    # relative error of the device's r: kappa's own (dkappa / kappa: the relative error of cos h -- where 1 / |A| enters), rho's six
    # roundings (4 kappa^2, + 1, sqrt, + 1 give tau within 4 u; sqrt(2 tau) within 3 u; the sum 5 u; the quotient 6 u; rho(kappa) has
    # condition number <= 1), r's three (rho^2, 1 +, the quotient; r(rho) has condition number |rho^2 - 1| / (rho^2 + 1) <= 1)
    relk = np.zeros((B, n)) if dkappa is None else (np.asarray(dkappa, dtype=np.float64) / np.maximum(ks.astype(np.float64), 1e-300))
    dr = r.astype(np.float64) * (relk + 9.0 * U)
    theta = np.full((B, n), np.nan, dtype=dt)
    dtheta = np.zeros((B, n))
    attempts = np.zeros((B, n), dtype=np.int64)
    margin = np.full((B, n), np.inf)
    todo = np.ones((B, n), dtype=bool)
    for t in range(MAX_ATTEMPTS):
        idx = np.nonzero(todo)
        if idx[0].size == 0:
            break
        w = PR.philox4x32_10((site[idx], sweep, 3, (mu << 8) | t), (k0[idx], k1[idx]))
        u1 = PR.u53(w[0], w[1]).astype(dt) * dt(2.0) ** -53
        u2 = PR.u53(w[2], w[3]).astype(dt) * dt(2.0) ** -53
        minus = (w[1] & np.uint64(1)) == 1
        arg = dt(PI_D) * u1
        z = np.cos(arg)
        rr, kk, fl = r[idx], kappa[idx], flat[idx]
        den = rr + z
        with np.errstate(divide='ignore', invalid='ignore'):
            f = np.where(fl, z, np.clip((dt(1) + rr * z) / den, dt(-1), dt(1)))
            c = kk * (rr - f)
            m1 = c * (dt(2) - c) - u2
            m2 = np.log(c / u2) + dt(1) - c
        m2 = np.where(np.isnan(m2), -np.inf, m2)
        take = fl | (m1 > 0) | (m2 >= 0)
        mg = np.where(fl, np.inf, np.where(m1 > 0, np.abs(m1), np.minimum(np.abs(m1), np.abs(m2)))).astype(np.float64)
        margin[idx] = np.minimum(margin[idx], mg)
        # the device's error of f, first order, the inputs through the exact partial derivatives df/dr = (z^2 - 1) / (r + z)^2,
        # df/dz = (r^2 - 1) / (r + z)^2: dz = u pi |sin| (the rounding of pi u1) + 2.5 u (ft_sincos); then the roundings of r z and
        # 1 + r z, each relative to (r + z), and of the sum r + z and the quotient, u |f| each.  The uniform limit has f = z.
        z64, r64, f64, den64 = z.astype(np.float64), rr.astype(np.float64), f.astype(np.float64), np.abs(den.astype(np.float64))
        dz = U * (math.pi * np.abs(np.sin(arg.astype(np.float64))) + 2.5)
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            df = (np.abs(z64 * z64 - 1) * dr[idx] + np.abs(r64 * r64 - 1) * dz) / den64 ** 2 + U * (np.abs(r64 * z64) + np.abs(1 + r64 * z64)) / den64 \
                + 2 * U * np.abs(f64)
        df = np.where(fl, dz, df)
        th = np.arccos(f)
        # acos: by the mean value theorem dth <= df / sqrt((1 - |f| - df)(1 + |f|)) while the interval stays inside (-1, 1) -- the factor
        # 1 / |sin delta|; at an end, |acos f - acos f'| <= acos(1 - (1 - |f|) - df) <= 1.02 sqrt(2 (1 - |f| + df)); plus 4 u th for the
        # library's acos itself
        gap = 1.0 - np.abs(f64)
        with np.errstate(divide='ignore', invalid='ignore'):
            mvt = df / np.sqrt(np.maximum(gap - df, 1e-300) * (1.0 + np.abs(f64)))
        dth = np.where(gap > 4 * df, mvt, 1.02 * np.sqrt(2 * (gap + df)) + 1.02 * np.sqrt(2 * gap)) + 4 * U * th.astype(np.float64)
        dth = np.where(np.isfinite(dth), dth, math.pi)
        sel = tuple(k[take] for k in idx)
        theta[sel] = np.where(minus[take], -th[take], th[take])
        dtheta[sel] = dth[take]
        attempts[sel] = t + 1
        todo[sel] = False
    return dict(theta=theta, attempts=attempts, margin=margin, dtheta=dtheta, accepted=~todo, r=r, flat=flat)


def class_update(x, mu, p, kind, beta, seeds=None, sweep=0, dt=LD):
    """One class of one sweep: kind 'or' | 'hb'; beta a number or [B]; x [B, 2, L, L] float64.  -> dict with
        x          the new field [B, 2, L, L] in `dt` (every link outside the class as it came)
        ii, jj     the class's links, [L^2 / 2]
        new, kappa, attempts, margin, bound, ambiguous   per link [B, L^2 / 2]
    derived_bound (`bound`, on the circle, against a device that computes in fp64 with correctly rounded + - * / sqrt, ft_sincos
    within 2.5 u and the library's acos within 4 u of the angle, u = 2^-53; first order, 1 % on top for the second):
      * a, b: two roundings each, <= u (|t1| + |t2| + |t3|) each: da = 2 u ta, db = 2 u tb;
      * OR: y = (b - a) - x: dy = da + db + u |b - a| + u |y|, then _reg_err;
      * HB: h = (a + b) / 2: dh = (da + db) / 2 + u |h|;  cos h: dch = |sin h| dh + 2.5 u;  kappa = 2 beta |cos h|: dkappa = 2 beta dch
        + u kappa, i.e. RELATIVE dch / |cos h| = 2 dch / |A|: the first ill-conditioned factor, which reaches the link through r
        (vonmises_draw);  phi = (b - a) / 2 (+ pi): dphi = (da + db) / 2 + u |b - a| / 2 (+ u |phi|);  where |cos h| <= dch the
        device may see the other sign of cos h, i.e. phi + pi: the link is `ambiguous` and its bound is pi (|A| <= 2 dch there, the
        distribution is uniform to 1e-15);  acos f with its factor 1 / |sin delta| (vonmises_draw);  y = phi +- acos f: dy = dphi +
        dth + u |y|, then _reg_err.
    A link whose attempts ran out keeps its value: bound 0."""
    x = np.asarray(x, dtype=np.float64)
    B, _, L, _ = x.shape
    ii, jj = class_links(L, mu, p)
    a, b, ta, tb = staples(x, mu, ii, jj, dt)
    own = x[:, mu, ii, jj].astype(dt)
    da, db = 2 * U * ta, 2 * U * tb
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    out = dict(ii=ii, jj=jj)
    if kind == 'or':
        y = (b - a) - own
        dy = da + db + U * np.abs(b64 - a64) + U * np.abs(y.astype(np.float64))
        new = regularize(y, dt)
        out.update(kappa=np.zeros((B, ii.size)), attempts=np.zeros((B, ii.size), dtype=np.int64), margin=np.full((B, ii.size), np.inf),
                   bound=1.01 * _reg_err(y.astype(np.float64), dy), ambiguous=np.zeros((B, ii.size), dtype=bool))
    else:
        beta_b = np.broadcast_to(np.asarray(beta, dtype=np.float64).reshape(-1, 1), (B, 1))
        h = dt(0.5) * (a + b)
        ch = np.cos(h)
        h64, ch64 = h.astype(np.float64), ch.astype(np.float64)
        dh = 0.5 * (da + db) + U * np.abs(h64)
        dch = np.abs(np.sin(h64)) * dh + 2.5 * U
        kappa = dt(2) * beta_b.astype(dt) * np.abs(ch)
        dkappa = 2 * beta_b * dch + U * kappa.astype(np.float64)
        phi = dt(0.5) * (b - a)
        phi = np.where(ch < 0, phi + dt(PI_D), phi)
        dphi = 0.5 * (da + db) + 0.5 * U * np.abs(b64 - a64) + np.where(ch64 < 0, U * np.abs(phi.astype(np.float64)), 0.0)
        ambiguous = np.abs(ch64) <= dch
        d = vonmises_draw(kappa, phi, seeds, ii.astype(np.uint64) * np.uint64(L) + jj.astype(np.uint64), mu, sweep, dt, dkappa)
        y = phi + np.where(d['accepted'], d['theta'], dt(0))
        dy = dphi + d['dtheta'] + U * np.abs(y.astype(np.float64))
        new = np.where(d['accepted'], regularize(y, dt), own)
        bound = np.where(d['accepted'], 1.01 * _reg_err(y.astype(np.float64), dy), 0.0)
        bound = np.where(ambiguous & d['accepted'], math.pi, np.minimum(bound, math.pi))
        out.update(kappa=kappa.astype(np.float64), attempts=d['attempts'], margin=d['margin'], bound=bound, ambiguous=ambiguous)
    xn = x.astype(dt)
    xn[:, mu, ii, jj] = new
    out.update(x=xn, new=new)
    return out


def sweep(x, beta, seeds, sweep_index, n_or=0, classes=0xF, dt=np.float64):
    """one compound sweep -- a heatbath sweep (index `sweep_index` of the stream) and n_or overrelaxation sweeps -- -> the new field"""
    for kind in ['hb'] + ['or'] * n_or:
        for k, (mu, p) in enumerate(CLASSES):
            if (classes >> k) & 1:
                x = class_update(x, mu, p, kind, beta, seeds, sweep_index, dt)['x'].astype(np.float64)
    return x


def plaquettes(x):
    x0, x1 = x[:, 0], x[:, 1]
    return x0 + np.roll(x1, -1, axis=-2) - np.roll(x0, -1, axis=-1) - x1


def action_sum(x):
    """sum over the lattice of cos P per chain, np.longdouble"""
    return np.cos(plaquettes(np.asarray(x, dtype=LD))).reshape(x.shape[0], -1).sum(axis=1)


def bessel_ratio(kappa):
    """I_1(kappa) / I_0(kappa)"""
    import mpmath as mp
    return float(mp.besseli(1, kappa) / mp.besseli(0, kappa)) if kappa > 0 else 0.0
