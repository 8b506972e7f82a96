"""The numpy twin of boundary-condition tempering (csrc/defect.hip) and the cases the CPU and GPU tests share.

Every definition of include/fthmc_hip.h ("Boundary-condition tempering") is stated once and evaluated in the dtype it is given:
float64 (what the device computes in) or np.longdouble (the reference of the comparisons) -- the defect's mask, C, Dsum and the integer
charge, S_d, the force, H, a whole trajectory of any schedule (the schedule comes from the library's fthmc_integrator_schedule binding,
ops.integrator_schedule), the translation and the swap -- and a float64 sampler of the whole algorithm.

The one thing that cannot be compared to round-off is the accept: the twin keeps |u - exp(-dH)| per chain, and a chain is LEFT OUT when
it is below U_MARGIN exp(-dH); on the committed inputs no chain is (tests/test_defect.py asserts it with the twin alone)."""
import functools
import math

import numpy as np

from meta_cases import DT, LD, U_MARGIN, _pi, draws, f64, links, plaq, regularize, rel_err, schedule  # noqa: F401  (shared with the tests)


# ---------------------------------------------------------------- the definitions
def mask(L, defect):
    """[L][L] bool: the plaquettes ((i0 + a) mod L, j0), 0 <= a < Ld"""
    i0, j0, Ld = defect
    m = np.zeros((L, L), dtype=bool)
    m[(i0 + np.arange(Ld)) % L, j0] = True
    return m


def wrap(p, dt):
    two_pi = 2 * _pi(dt)
    return (p + _pi(dt)) % two_pi - _pi(dt)


def sums(x, defect, dt):
    """-> (C = sum cos P, Dsum = its part on the defect, Q = the integer charge) per chain"""
    P = plaq(x.astype(dt))
    cs = np.cos(P)
    Q = np.rint((wrap(P, dt).sum(axis=(1, 2)) / (2 * _pi(dt))).astype(np.float64))
    return cs.sum(axis=(1, 2)), (cs * mask(x.shape[-1], defect)).sum(axis=(1, 2)), Q


def action(x, beta, g, defect, dt):
    """-> (S_d = (-beta) C + (beta - g_b) Dsum, C, Dsum, Q)"""
    C, D, Q = sums(x, defect, dt)
    return -dt(beta) * C + (dt(beta) - np.asarray(g).astype(dt)) * D, C, D, Q


def weights(L, beta, g, defect, dt):
    """w[B][L][L]: g_b on the defect, beta elsewhere"""
    return np.where(mask(L, defect)[None], np.asarray(g).astype(dt)[:, None, None], dt(beta))


def force(x, beta, g, defect, dt):
    """F = dS_d / dx: gP = w sin P, f0 = gP(s) - gP(s_{j-1}), f1 = gP(s_{i-1}) - gP(s)"""
    gp = weights(x.shape[-1], beta, g, defect, dt) * np.sin(plaq(x.astype(dt)))
    return np.stack([gp - np.roll(gp, 1, 2), np.roll(gp, 1, 1) - gp], axis=1)


def hamiltonian(x, v, beta, g, defect, dt):
    S, C, D, Q = action(x, beta, g, defect, dt)
    return S + dt(0.5) * (v.astype(dt) ** 2).sum(axis=(1, 2, 3)), C, D, Q


def trajectory(x, v, u, beta, g, defect, dt_md, nstep, integrator, dt=LD, sched=None):
    """One trajectory of every chain -> dict(x_new, dH, acc, H0, H1, csum, dsum, Q, x_prop, u_margin, left_out)"""
    b0, stages = sched if sched is not None else schedule(integrator, float(dt_md), int(nstep))
    x0, y, p = x.astype(dt), x.astype(dt), v.astype(dt)
    h0, c0, d0, q0 = hamiltonian(x0, p, beta, g, defect, dt)
    y = y + dt(b0) * p
    ye = y
    for kind, a, b in stages:
        F = force(ye, beta, g, defect, dt)
        if kind == 'shift':
            ye = y - dt(a) * F
        else:
            p = p - dt(a) * F
            y = y + dt(b) * p
            ye = y
    y = regularize(y, dt)
    h1, c1, d1, q1 = hamiltonian(y, p, beta, g, defect, dt)
    dH = h1 - h0
    e = np.exp(-dH)
    uu = np.asarray(u, dtype=np.float64).astype(dt)
    acc = uu < e
    u_margin = np.abs(uu - e).astype(np.float64)
    left_out = u_margin < U_MARGIN * e.astype(np.float64)
    return {'x_new': np.where(acc[:, None, None, None], y, x0), 'dH': dH, 'acc': acc, 'H0': h0, 'H1': h1, 'csum': np.where(acc, c1, c0),
            'dsum': np.where(acc, d1, d0), 'Q': np.where(acc, q1, q0), 'x_prop': y, 'u_margin': u_margin, 'left_out': left_out}


def translate(x, rung, top, shift):
    """x_out[b][mu][(i + s0) mod L][(j + s1) mod L] = x[b][mu][i][j] on rung `top`, a copy elsewhere"""
    out = np.array(x, copy=True)
    for b in np.nonzero(np.asarray(rung) == top)[0]:
        out[b] = np.roll(x[b], (int(shift[b][0]), int(shift[b][1])), axis=(1, 2))
    return out


def swap(gs, dsum, u, g_b, rung, chain_of, parity):
    """One round of fthmc_replica_swap given betas := gs, C := dsum, beta_b := g_b, in place -> swap_acc [M, K - 1] (1, 0, -1: not tried)"""
    K = len(gs)
    M = len(g_b) // K
    acc = -np.ones((M, K - 1))
    for m in range(M):
        for k in range(parity, K - 1, 2):
            a, c = m * K + chain_of[m * K + k], m * K + chain_of[m * K + k + 1]
            ok = u[m][k] < np.exp((gs[k] - gs[k + 1]) * (dsum[c] - dsum[a]))
            acc[m, k] = 1.0 if ok else 0.0
            if ok:
                rung[a], rung[c] = k + 1, k
                g_b[a], g_b[c] = gs[k + 1], gs[k]
                chain_of[m * K + k], chain_of[m * K + k + 1] = chain_of[m * K + k + 1], chain_of[m * K + k]
    return acc


# ---------------------------------------------------------------- the cases
SHAPES_ONE_LAUNCH = ((3, 4), (2, 8), (5, 12), (2, 20), (3, 32), (2, 36), (2, 64))   # path 1 and path 2; 32: one site per thread, 36: ragged
SHAPES_SEQUENCED = ((2, 68), (1, 128))                                               # path 2 only
SHAPES = SHAPES_ONE_LAUNCH + SHAPES_SEQUENCED
AMPS = (math.pi, 0.3)
BETAS = (2.0, 6.0)
NSTEPS = (1, 3)
INTEGRATORS = ('leapfrog', 'omelyan', 'force_gradient')
DEFECTS = ('none', 'one', 'full', 'wrap', 'col0')


def defect_of(kind, L):
    """none: Ld = 0; one: Ld = 1; full: Ld = L; wrap: a row that wraps (i0 = L - 2, Ld = 4) at j0 = L - 1; col0: j0 = 0"""
    return {'none': (1, 2, 0), 'one': (1, 2, 1), 'full': (0, 1, L), 'wrap': (L - 2, L - 1, 4), 'col0': (3, 0, 3)}[kind]


def couplings(B, beta, k):
    """g_b per chain, mixed out of {0, beta / 3, beta}"""
    return np.array([(0.0, beta / 3.0, beta)[(b + k) % 3] for b in range(B)])


def _cases():
    """every shape with every defect; amplitude, beta, nstep and integrator rotate (as meta_cases._cases rotates them) so that each
    value meets each shape class and each defect"""
    out = []
    for dk in DEFECTS:
        k = 0
        for B, L in SHAPES:
            out.append((B, L, AMPS[k % 2], BETAS[(k // 2) % 2], NSTEPS[(k // 4) % 2], INTEGRATORS[k % 3], dk))
            k += 1
    return tuple(out)


CASES = _cases()          # (B, L, amp, beta, nstep, integrator, defect kind)


def case_id(c):
    B, L, amp, beta, nstep, integ, dk = c
    return f'B{B}-L{L}-a{amp:.1f}-b{beta:g}-n{nstep}-{integ}-{dk}'


def case_seed(c):
    B, L, amp, beta, nstep, integ, dk = c
    return 9000 + 97 * L + 13 * B + 5 * DEFECTS.index(dk)


@functools.lru_cache(maxsize=None)
def case(c):
    """-> (x, v, u, g, defect, longdouble twin's trajectory) of case c; computed once and shared (treat as read-only)"""
    B, L, amp, beta, nstep, integ, dk = c
    seed = case_seed(c)
    x = links(B, L, seed, amp)
    v, u = draws(B, L, seed + 1)
    g, df = couplings(B, beta, DEFECTS.index(dk)), defect_of(dk, L)
    return x, v, u, g, df, trajectory(x, v, u, beta, g, df, DT, nstep, integ, dt=LD)


# ---------------------------------------------------------------- the twin as a sampler
def sampler(L, beta, cs, M, ntraj, defect, seed=11, dt_md=0.1, nstep=10, do_translate=True):
    """float64 leapfrog PTBC from a cold start: M ladders over cs, a swap round (parities alternating) after every trajectory and a
    random translation of the top rung behind it -> dict(Q [ntraj, M] of rung K - 1, dq, acc, swap_acc [K - 1], dplaq [ntraj, K, M])"""
    rng = np.random.default_rng(seed)
    K = len(cs)
    B = M * K
    gs = beta * np.asarray(cs, dtype=np.float64)
    g_b, rung, chain_of = np.tile(gs, M), np.tile(np.arange(K), M), np.tile(np.arange(K), M)
    x = np.zeros((B, 2, L, L))
    sched = (0.5 * dt_md, [('kick', dt_md, dt_md)] * (nstep - 1) + [('kick', dt_md, 0.5 * dt_md)])
    Ld = defect[2]
    Q, dq, acc, dplaq = [], [], [], []
    tried, won = np.zeros(K - 1), np.zeros(K - 1)
    qold = np.zeros(M)
    for t in range(ntraj):
        r = trajectory(x, rng.standard_normal(x.shape), rng.uniform(size=B), beta, g_b, defect, dt_md, nstep, 'leapfrog', dt=np.float64, sched=sched)
        x = r['x_new']
        order = np.argsort(rung.reshape(M, K), axis=1) + (np.arange(M) * K)[:, None]          # [M, K] -> chain on rung k
        dplaq.append((r['dsum'][order] / max(Ld, 1)).T)
        sa = swap(gs, r['dsum'], rng.uniform(size=(M, K - 1)), g_b, rung, chain_of, t % 2)
        tried += (sa >= 0).sum(axis=0); won += (sa > 0.5).sum(axis=0)
        top = np.nonzero(rung == K - 1)[0]                                                   # one per ladder, in ladder order
        q = r['Q'][top]
        Q.append(q); dq.append(np.abs(q - qold).mean()); acc.append(r['acc'].mean())
        qold = q
        if do_translate:
            x = translate(x, rung, K - 1, np.floor(rng.uniform(size=(B, 2)) * L).astype(np.int64))
    return {'Q': np.array(Q), 'dq': float(np.mean(dq)), 'acc': float(np.mean(acc)), 'swap_acc': won / np.maximum(tried, 1),
            'dplaq': np.array(dplaq)}
