"""The numpy side of the hard-input metadynamics tests (tests/test_meta_hard.py, tests/test_z_meta_hard_gpu.py): the shapes at which
the launch geometry of fthmc_amd/csrc/meta.hip and of the biased plain sequence (hmc_trajectory_call, csrc/api.hip) changes, stencil_cases' hard inputs, a long
double reference of every operation that carries its own per-site / per-chain error bound, a float64 twin in the kernels' operation
and summation order, and the named mutants of the twin.  Built on meta_cases (Table: rows, geometry, deposit; the definitions and
trajectory(), against which the reference here is cross-checked on the CPU), stencil_cases (the per-operation bound forms, SLACK, the
site-by-site propagation) and batch_kernel_cases (sum_roundings, action_bounds, kinetic_cap through stencil_cases.r_energy).

Shapes (beta = 2.5, dt = 0.05, nstep 1 and 2, the three integrators rotating; see SHAPES and test_meta_hard.py, which computes what
each reaches from the launchers' arithmetic):
  rows   B 6   L 8   G 2, 3        1 < G < B: b / (B / G), b % G and "row 0 or row b" all differ
  batch  B 258 L 4   G 1, 3, 258   chains 256, 257 in k_meta_energy's second workgroup, its b >= B guard, row 2 at G = 3
  L36    B 2   L 36  G 2           512 threads: 2 passes + 272 sites; one-launch kernel: 1 pass + 272
  L60    B 2   L 60  G 1           512 threads: 7 passes + 16; one-launch kernel: 3 passes + 528
  L132   B 2   L 132 G 2           1040 sites in k_meta_gp's second pass; 1024 threads: 17 passes + 16 (sequenced path, nstep 1)
Tables: meta_cases.table('rough') for every shape, 'quad' for rows and L60.  Inputs: stencil_cases.inputs (links +-pi, chain 0 with
pinned links at +-(pi - 1e-9), the last chain shifted by +-30, momenta x 3); the uniforms of the accept are drawn from seed + 17
(chain 0 draws 0 where the draw would accept no chain: traj_reference, which records it as `forced`).

Placement cases (force and action; B = 6, L = 8, G = 6, uniform +-pi links, rough rows): the six chains sit, in order, on the positive
wall, on the negative wall, in interval 0, in interval nb - 2, 1e-6 (in t) below a node and 1e-6 above the same node.  Chain 4 is a
drawn field and qmax is COMPUTED from its long double Q_m so that its t is k - 1e-6; chain 5 is chain 4 with the one link of largest
dQ_m / dx turned until t is k + 1e-6; chains 0 .. 3 are the first fields of a seeded pool that fall where they should under that
geometry.  The same against nb = 2 (one interval: node 1 separates the table from the wall, so chain 5 is a wall chain with
d = 2e-6 qmax).  The zero field with nb = 41, qmax = 2: Q_m = 0, the float64 twin says which node t lands on (20, f = 0), vbias is that
node's height and F = +0.0 in every bit (gP is one number at every site).

Constants of the statement: FT_TWO_PI and delta = fl(fl(2 qmax) / (nb - 1)) are the DOUBLES the device holds (as stencil_cases takes
FT_PI in regularize): the reference divides by exactly these, so that no bound has to carry the representation error of a constant.
meta_cases' long double twin divides by the long double pi and the unrounded delta; the two differ by <= 0.6 u relative in Q_m, t
and c, which test_meta_hard.py checks.

Bounds, u = 2^-53, first order, arrays per site or per chain computed from the inputs' magnitudes, never from a device run; e(.) is
the bound an operand carries.  stencil_cases' forms for plaq, sin (and cos: ft_sincos is within 2.5 ulp <= 5 u for both), force,
kick, shift, drift, regularize and H = S + K / 2.  New here:
  Q_m   q = (sum_s sin P_s) / 2 pi     e(q) = (sum_s e(sin P_s) + R u sum_s |sin P_s|) / 2 pi + u |q|
        R counts the roundings on the way of one term through the sum: batch_kernel_cases.sum_roundings(n, chain_threads(L)) for the
        workgroup sums of k_meta_sums / k_meta_force / k_meta_action; in the one-launch kernel (L <= 64) ceil(n / 1024) - 1 in the
        thread, four DPP levels and three row additions in the wave, 15 additions over the 16 waves (the first onto 0.0 is exact):
        ceil(n / 1024) + 21.  R is the larger of the two; the quotient rounds once (u |q|).
  lookup inside the table   t = (q + qmax) / delta     e(t) = e(q) / delta + 2 u |t|     (the sum, the quotient)
        V = v0 + f dv, f = t - floor(t) (exact), dv = v1 - v0     e(V) = |dv| e(t) + 2 u (|v0| + |f dv|) + u |dv|
                                                                  (the product and the sum; dv's rounding reaches V times f <= 1)
        c = dv / (delta 2 pi)     e(c) = 3 u |c|     (dv, the product delta 2 pi, the quotient: one rounding each -- c is ONE quotient
                                                      of a table difference and does not see e(q) as long as the interval is the
                                                      reference's)
  on the wall   d = |q| - qmax     e(d) = e(q) + u |d|
        V = edge + ((wall / 2) d) d     e(V) = wall |d| e(d) + 3 u wall d^2 / 2 + u |V_edge|     (two products; the sum's rounding is
                                        u |V| <= u |V_edge| + u wall d^2 / 2)
        c = +-(wall d) / 2 pi           e(c) = wall e(d) / 2 pi + 3 u |c|                        (2 roundings; 3 kept)
  gP = beta sin P + c cos P     beta e(sin) + |c| e(cos) + e(c) |cos P| + 2 u (|beta sin P| + |c cos P|)
                                (each product, and the sum charged to both terms; one rounding less if contracted)
  H_b = H + V and S_b = S + V   e(H) + e(V) + u |H_b|
Through an MD the bounds go site by site through the stencil as in stencil_cases.r_md; the one new coupling is that e(c) of a stage on
the wall takes e(q), which sums e(sin P) -- e(x) of every link of the chain.
V' jumps at the nodes, so the interval (or the wall side) of every lookup is the reference's, and a chain is compared only where
that is decided on the inputs: min |t - round(t)| > 8 e(t) inside, |d| > 8 e(d) on the wall (8: the device's t may be e(t) from the
reference's, the twin's another e(t); 8 leaves a factor 4 for what first order leaves out).  An accept is compared where
|u - exp(-dH)| > exp(-dH) (2 e(dH) + 4 u): exp(-dH) moves by exp(-dH) e(dH) with dH, the device's exp is within 2 u, the comparison
with the factor 2 in hand.  Both are conditions on the inputs; where a draw misses one the seed is redrawn by
integrator_cases.decided_case's rule (seed + 1000, at most 3 times), and on the committed seeds NO chain and NO lookup is left out
(test_meta_hard.py asserts it with the reference alone).
Every bound is widened by stencil_cases.SLACK = 1 + 2^-8 for the reference's own rounding (2^-11 u per operation)."""
import collections
import functools
import math

import numpy as np

import batch_kernel_cases as BC
import integrator_cases as IC
import meta_cases as MC
import stencil_cases as SC

U, LD, SLACK = SC.U, SC.LD, SC.SLACK
TWO_PI = SC.TWO_PI
BETA, DT = SC.BETA, SC.DT
NSTEPS = (1, 2)
INTEGRATORS = IC.NAMES
GP_STRIDE = 64 * 256                 # launch_meta_gp: at most 64 workgroups of 256 threads, one site each per pass
ENERGY_BLOCK = 256                   # launch_meta_energy: chains per workgroup
ONE_LAUNCH_NT, ONE_LAUNCH_MAXL = 1024, 64          # k_meta_trajectory (MT_NT, MT_MAXL)
MARGIN = 8.0
ld, f64, mag = SC.ld, SC.f64, SC.mag

chain_threads = BC.nt_action         # kernels.h chain_threads(L): 1024 from 4096 sites, 512 from 1024, else 256

Case = collections.namedtuple('Case', 'shape seed B L G table nstep integrator paths')

# id -> (B, L, Gs, table kinds, paths)
SHAPES = collections.OrderedDict([
    ('rows', (6, 8, (2, 3), ('rough', 'quad'), (1, 2))),
    ('batch', (258, 4, (1, 3, 258), ('rough',), (1, 2))),
    ('L36', (2, 36, (2,), ('rough',), (1, 2))),
    ('L60', (2, 60, (1,), ('rough', 'quad'), (1, 2))),
    ('L132', (2, 132, (2,), ('rough',), (2,))),
])


def _cases():
    out, k = [], 0
    for sid, (B, L, Gs, kinds, paths) in SHAPES.items():
        for G in Gs:
            for tk in kinds:
                if sid == 'L132':                    # nstep 1 only: leapfrog (one stage) and force-gradient (kick, shift, kicks)
                    runs = [(1, 'leapfrog'), (1, 'force_gradient')]
                else:
                    runs = []
                    for n in NSTEPS:
                        runs.append((n, INTEGRATORS[k % 3]))
                        k += 1
                for n, integ in runs:
                    out.append(Case(sid, 41000 + 10 * L + B + G, B, L, G, tk, n, integ, paths))
    return tuple(out)


CASES = _cases()
FIELD_CASES = tuple({(c.shape, c.G, c.table): c for c in CASES}.values())      # force and action see no nstep and no integrator


def case_id(c):
    return f'{c.shape}-G{c.G}-{c.table}-n{c.nstep}-{c.integrator}'


def field_id(c):
    return f'{c.shape}-G{c.G}-{c.table}'


def sum_count(L):
    """R of e(q): the roundings one term meets in the chain sum, the larger of the workgroup sum's and the one-launch kernel's"""
    n = L * L
    r = BC.sum_roundings(n, chain_threads(L))
    if L <= ONE_LAUNCH_MAXL:
        r = max(r, -(-n // ONE_LAUNCH_NT) + 21)
    return r


def delta_of(tab):
    """the device's delta: (2.0 * qmax) / (double)(nb - 1), a double"""
    return np.float64(2.0 * tab.qmax) / np.float64(tab.nb - 1)


# ---------------------------------------------------------------- the long double reference with its bounds
def r_sincos(x, ex):
    P, eP = SC.r_plaq(x, ex)
    s, c = np.sin(P), np.cos(P)
    return s, eP + 5 * U * mag(s), c, eP + 5 * U * mag(c)


def r_charge(s, es):
    B, L = s.shape[0], s.shape[-1]
    q = s.reshape(B, -1).sum(axis=1) / LD(TWO_PI)
    eq = (es.reshape(B, -1).sum(axis=1) + sum_count(L) * U * mag(s).reshape(B, -1).sum(axis=1)) / TWO_PI + U * mag(q)
    return q, eq


Look = collections.namedtuple('Look', 'V eV c ec inside i t et d ed decided')


def r_lookup(tab, q, eq):
    """V(q), c = V'(q) / 2 pi per chain with their bounds, the interval / wall side, and whether that is decided on the inputs"""
    B = len(q)
    r = tab.rows(B)
    delta = delta_of(tab)
    qmax, wall = tab.qmax, tab.wall
    t = (q + LD(qmax)) / LD(delta)
    et = eq / delta + 2 * U * mag(t)
    fl = np.floor(t)
    inside = (t >= 0) & (fl <= tab.nb - 2)
    i = np.where(inside, fl, 0).astype(np.int64)
    v0, v1 = ld(tab.V[r, i]), ld(tab.V[r, np.minimum(i + 1, tab.nb - 1)])
    dv, f = v1 - v0, t - fl
    Vin = v0 + f * dv
    eVin = mag(dv) * et + 2 * U * (mag(v0) + mag(f * dv)) + U * mag(dv)
    cin = dv / (LD(delta) * LD(TWO_PI))
    ecin = 3 * U * mag(cin)
    d = np.abs(q) - LD(qmax)
    ed = eq + U * mag(d)
    edge = ld(np.where(f64(q) < 0, tab.V[r, 0], tab.V[r, -1]))
    Vw = edge + ((LD(0.5) * LD(wall)) * d) * d
    eVw = wall * mag(d) * ed + 3 * U * wall * mag(d) ** 2 / 2 + U * mag(edge)
    cw = np.where(q < 0, -(LD(wall) * d), LD(wall) * d) / LD(TWO_PI)
    ecw = wall * ed / TWO_PI + 3 * U * mag(cw)
    decided = np.where(inside, f64(np.abs(t - np.rint(t))) > MARGIN * et, mag(d) > MARGIN * ed)
    return Look(np.where(inside, Vin, Vw), np.where(inside, eVin, eVw), np.where(inside, cin, cw), np.where(inside, ecin, ecw),
                inside, i, t, et, d, ed, decided)


def r_gp(x, ex, beta, tab):
    """-> ((gP, e), (q, e), Look)"""
    s, es, c, ec = r_sincos(x, ex)
    q, eq = r_charge(s, es)
    lk = r_lookup(tab, q, eq)
    C, eC = lk.c[:, None, None], lk.ec[:, None, None]
    g = LD(beta) * s + C * c
    eg = beta * es + mag(C) * ec + eC * mag(c) + 2 * U * (mag(LD(beta) * s) + mag(C * c))
    return (g, eg), (q, eq), lk


def r_force(x, ex, beta, tab):
    G, Q, lk = r_gp(x, ex, beta, tab)
    return SC.r_force_of(*G), Q, lk


def r_action(x, ex, beta, tab):
    """-> dict S, qm, vbias -> (value, bound) and the Look.  S: stencil_cases.r_energy with no momenta (its kinetic terms vanish)"""
    z = np.zeros(x.shape)
    (H, S, K), bS = SC.r_energy(x, ex, ld(z), z, beta)
    s, es, _, _ = r_sincos(x, ex)
    q, eq = r_charge(s, es)
    lk = r_lookup(tab, q, eq)
    Sb = S + lk.V
    return {'S': (Sb, bS + lk.eV + U * mag(Sb)), 'qm': (q, eq), 'vbias': (lk.V, lk.eV)}, lk


def r_energy(x, ex, v, ev, beta, tab):
    """-> ((H_b, e), (q, e), (V, e), Look)"""
    (H, S, K), bH = SC.r_energy(x, ex, v, ev, beta)
    s, es, _, _ = r_sincos(x, ex)
    q, eq = r_charge(s, es)
    lk = r_lookup(tab, q, eq)
    Hb = H + lk.V
    return (Hb, bH + lk.eV + U * mag(Hb)), (q, eq), (lk.V, lk.eV), lk


def hold(pair):
    return pair[0], pair[1] * SLACK


@functools.lru_cache(maxsize=None)
def table_of(c):
    return MC.table(c.table, c.G)


@functools.lru_cache(maxsize=None)
def field_reference(c):
    """force and action of the case's start field -> dict(x, tab, F, S, qm, vbias: held (value, bound) pairs; decided: per chain)"""
    x, _ = SC.inputs(c.seed, c.B, c.L)
    return _field_reference(x, table_of(c))


def _field_reference(x, tab):
    X = SC.exact(x)
    F, Q, lk = r_force(*X, BETA, tab)
    A, lk2 = r_action(*X, BETA, tab)
    out = {'x': x, 'tab': tab, 'F': hold(F), 'decided': lk.decided & lk2.decided, 'look': lk}
    out.update({k: hold(v) for k, v in A.items()})
    return out


Traj = collections.namedtuple('Traj', 'seed redraws x v u tab H0 H1 dH xr qm vbias acc lookups_decided accept_decided stages forced xp')


def _traj(c, seed):
    x, v = SC.inputs(seed, c.B, c.L)
    u = np.random.default_rng(seed + 17).uniform(size=c.B)
    tab = table_of(c)
    z = np.zeros(x.shape)
    H0, Q0, V0, lk = r_energy(ld(x), z, ld(v), z, BETA, tab)
    decided = lk.decided.copy()
    b0, stages = IC.schedule(c.integrator, DT, c.nstep)
    X = SC.r_axpy(*SC.exact(x), *SC.exact(v), b0)
    Pm = SC.exact(v)
    at = X
    for kind, a, b in stages:
        F, _, lk = r_force(at[0], at[1], BETA, tab)
        decided &= lk.decided
        if kind == 'shift':
            at = SC.r_axpy(*X, *F, -a)
        else:
            Pm = SC.r_kick(*Pm, *F, a)
            X = SC.r_axpy(*X, *Pm, b)
            at = X
    xr = SC.r_regularize(*X)
    H1, Q1, V1, lk = r_energy(xr[0], xr[1], Pm[0], Pm[1], BETA, tab)
    decided &= lk.decided
    dH = H1[0] - H0[0]
    bdH = H0[1] + H1[1] + U * mag(dH)
    e = np.exp(-dH)
    forced = bool(not (ld(u) < e).any() and f64(dH)[0] < SC.DH_MAX)
    if forced:                                                  # no chain of the draw accepted: chain 0 draws u = 0 (see traj_reference)
        u[0] = SC.U_ACCEPT
    acc = ld(u) < e
    accept_decided = f64(np.abs(ld(u) - e)) > f64(e) * (2 * bdH * SLACK + 4 * U)
    sel = lambda a1, a0: (np.where(acc, a1[0], a0[0]), np.where(acc, a1[1], a0[1]))
    a4 = acc[:, None, None, None]
    xn = (np.where(a4, xr[0], ld(x)), np.where(a4, xr[1], 0.0))
    return Traj(seed, 0, x, v, u, tab, hold(H0), hold(H1), hold((dH, bdH)), hold(xn), hold(sel(Q1, Q0)), hold(sel(V1, V0)), f64(acc) > 0.5,
                decided, accept_decided, len(stages), forced, hold(xr))


@functools.lru_cache(maxsize=None)
def traj_reference(c):
    """The case's trajectory in long double with its bounds; the seed is redrawn (seed + 1000, at most 3 times) until every lookup and
    every accept of every chain is decided on the reference's numbers.  x_new: the selected field -- the regularized end point with its
    bound where accepted, x with bound 0 where rejected (compared as an angle: a link next to the branch of regularize may come back
    2 pi away).  The uniforms are drawn; where the draw would accept no chain, chain 0 draws u = 0 instead -- accepted whatever
    dH < 700 (stencil_cases.U_ACCEPT), so that x_new is held per link wherever an accept is possible.  It is not in
    L132-leapfrog: one leapfrog step from the wall at |Q_m| = 6.6 and 23 gains dH = 1.2e4 and 3.4e5, exp(-dH) = 0 on the device; that
    case holds H0, H1, dH, qm and vbias, and L132-force_gradient (chain 0 accepted) the links beyond k_meta_gp's first pass."""
    for k in range(4):
        T = _traj(c, c.seed + 1000 * k)
        if T.lookups_decided.all() and T.accept_decided.all():
            return T._replace(redraws=k)
    raise AssertionError(f'{case_id(c)}: no draw with every lookup and accept decided in 3 redraws')


# ---------------------------------------------------------------- placement
Placement = collections.namedtuple('Placement', 'x tab k roles')
ROLES = ('wall+', 'wall-', 'interval0', 'interval_last', 'below_node', 'above_node')
NODE_OFFSET = 1e-6


def _qm_ld(x):
    return np.sin(SC.r_plaq(ld(x), np.zeros(x.shape))[0]).reshape(len(x), -1).sum(axis=1) / LD(TWO_PI)


@functools.lru_cache(maxsize=None)
def placement(nb, seed=43000):
    L, wall = 8, 10.0
    rng = np.random.default_rng(seed)
    pool = rng.uniform(-math.pi, math.pi, (4096, 2, L, L))
    qp = _qm_ld(pool)
    q64 = f64(qp)
    i4 = int(np.argmax((np.abs(q64) > 0.2) & (np.abs(q64) < 0.6)))
    q4 = qp[i4]
    k = int(np.rint((f64(q4) / 1.0 + 1.0) * (nb - 1) / 2.0)) if nb > 2 else (1 if q4 > 0 else 0)
    qmax = float(q4 / (2 * (LD(k) - LD(NODE_OFFSET)) / LD(nb - 1) - 1))
    assert qmax > 0
    tab = MC.Table(np.cumsum(rng.uniform(-3.0, 3.0, size=(6, nb)), axis=1), qmax, wall)
    delta = delta_of(tab)
    tp = f64((qp + LD(qmax)) / LD(delta))
    first = lambda m: int(np.argmax(m)) if m.any() else None
    lo, hi = ((0.1, 0.9), (nb - 2 + 0.1, nb - 2 + 0.9)) if nb > 2 else ((0.1, 0.45), (0.55, 0.9))
    idx = [first(q64 > qmax + 0.1), first(q64 < -qmax - 0.1), first((tp > lo[0]) & (tp < lo[1])), first((tp > hi[0]) & (tp < hi[1])), i4]
    assert None not in idx and len(set(idx)) == 5, idx
    x = np.concatenate([pool[idx], pool[i4:i4 + 1]], axis=0).copy()
    # chain 5: chain 4 with the link of largest |dQ_m / dx| turned until t = k + NODE_OFFSET (secant steps on the long double Q_m of the
    # float64 field)
    P = SC.r_plaq(ld(x[5:6]), np.zeros((1, 2, L, L)))[0][0]
    cs = f64(np.cos(P))
    dq0 = (cs - np.roll(cs, 1, 1)) / TWO_PI                   # x0[i][j] enters P(i, j) with + and P(i, j - 1) with -
    at = np.unravel_index(int(np.argmax(np.abs(dq0))), dq0.shape)
    target = (LD(k) + LD(NODE_OFFSET)) * LD(delta) - LD(qmax)
    base = x[5, 0][at]
    th0, th1 = 0.0, float((target - q4) / LD(dq0[at]))

    def miss(th):
        y = x[5:6].copy()
        y[0, 0][at] = base + th
        return float(_qm_ld(y)[0] - target)
    m0, m1 = miss(th0), miss(th1)
    for _ in range(8):
        if m1 == m0:
            break
        th0, th1, m0 = th1, th1 - m1 * (th1 - th0) / (m1 - m0), m1
        m1 = miss(th1)
    x[5, 0][at] = base + th1
    x.setflags(write=False)
    return Placement(x, tab, k, ROLES)


@functools.lru_cache(maxsize=None)
def placement_reference(nb):
    p = placement(nb)
    return _field_reference(p.x, p.tab)


def zero_field():
    """x = 0 against a rough table of nb = 41 on |q| <= 2, one row per chain -> (x, tab, node): the float64 twin's t is the node"""
    x = np.zeros((6, 2, 8, 8))
    tab = MC.Table(np.cumsum(np.random.default_rng(43500).uniform(-3.0, 3.0, size=(6, 41)), axis=1), 2.0, 10.0)
    t = (np.float64(0.0) + np.float64(tab.qmax)) / delta_of(tab)
    assert t == np.floor(t)
    return x, tab, int(t)


PLACEMENTS = (41, 2)


# ---------------------------------------------------------------- the float64 twin, in the kernels' operation and summation order
MUTANTS = ('row_mod', 'row_zero', 'next_interval', 'wall_sign', 'edge_far', 'stale_qm', 'sums_first_pass', 'drop_wave', 'gp_one_pass',
           'energy_second_block', 'select_proposed', 'slope_3e8')


def t_sums(x, mutant=None):
    """k_meta_sums / mt_chain_sums + ft_block_sum: (sum sin P, sum cos P) per chain, a workgroup of chain_threads(L).
      sums_first_pass   the strided loop stops after its first pass: sites >= chain_threads(L) are dropped
      drop_wave         wave 1's partial is left out of the workgroup sum"""
    B, L = x.shape[0], x.shape[-1]
    nt = chain_threads(L)
    P = SC.t_plaq(x)
    sn, cs = np.sin(P).reshape(B, -1), np.cos(P).reshape(B, -1)
    passes = 1 if mutant == 'sums_first_pass' else None
    dw = 1 if mutant == 'drop_wave' else None
    q = np.array([BC.block_sum(BC.strided_partials(t, nt, passes=passes), dw) for t in sn])
    c = np.array([BC.block_sum(BC.strided_partials(t, nt, passes=passes), dw) for t in cs])
    return q, c, sn.reshape(P.shape), cs.reshape(P.shape)


def t_lookup(tab, q, mutant=None):
    """mt_lookup in float64 -> (V, c).
      row_mod        chain b reads row b % G                  row_zero      every chain reads row 0
      next_interval  the slope of interval i + 1              wall_sign     no sign flip on the negative wall
      edge_far       the wall measured from the far end node (its height, and d = |q| + qmax)
      slope_3e8      c (1 + 3e-8)"""
    B = len(q)
    r = tab.rows(B)
    if mutant == 'row_mod':
        r = np.arange(B) % tab.G
    elif mutant == 'row_zero':
        r = np.zeros(B, dtype=np.int64)
    V, nb, qmax, wall = tab.V, tab.nb, np.float64(tab.qmax), np.float64(tab.wall)
    delta = delta_of(tab)
    t = (q + qmax) / delta
    fl = np.floor(t)
    inside = (t >= 0.0) & (fl <= nb - 2)
    i = np.where(inside, fl, 0).astype(np.int64)
    v0 = V[r, i]
    dv = V[r, i + 1] - v0
    f = t - fl
    Vin = v0 + f * dv
    j = np.minimum(i + 1, nb - 2) if mutant == 'next_interval' else i
    cin = (V[r, j + 1] - V[r, j]) / (delta * TWO_PI)
    neg = q < 0.0
    if mutant == 'edge_far':
        d, edge = np.abs(q) + qmax, np.where(neg, V[r, nb - 1], V[r, 0])
    else:
        d, edge = np.abs(q) - qmax, np.where(neg, V[r, 0], V[r, nb - 1])
    Vw = edge + ((0.5 * wall) * d) * d
    cw = np.where(neg & (mutant != 'wall_sign'), -(wall * d), wall * d) / TWO_PI
    c = np.where(inside, cin, cw)
    if mutant == 'slope_3e8':
        c = c * (1.0 + 3e-8)
    return np.where(inside, Vin, Vw), c


def t_bias(tab, ssum, mutant=None):
    q = ssum / TWO_PI
    V, c = t_lookup(tab, q, mutant)
    return q, V, c


def t_gp(x, beta, tab, mutant=None, before=None):
    """k_meta_sums + k_meta_gp -> (gP, Q_m).  before = (gP, Q_m) of the stage before (None: nothing was computed yet):
      stale_qm      c from the Q_m of the stage before
      gp_one_pass   k_meta_gp's first pass only: sites >= 64 x 256 keep the stage before's gP (t_trajectory: before the first stage
                    the plane holds gP of the start field, a finite stale plane; NaN only where no plane is handed in)"""
    B, L = x.shape[0], x.shape[-1]
    ssum, _, sn, cs = t_sums(x, mutant)
    q, V, c = t_bias(tab, ssum, mutant)
    if mutant == 'stale_qm' and before is not None:
        _, c = t_lookup(tab, before[1], mutant)
    g = beta * sn + c[:, None, None] * cs
    if mutant == 'gp_one_pass' and L * L > GP_STRIDE:
        g = g.reshape(B, -1).copy()
        g[:, GP_STRIDE:] = np.nan if before is None else before[0].reshape(B, -1)[:, GP_STRIDE:]
        g = g.reshape(B, L, L)
    return g, q


def t_force(x, beta, tab, mutant=None):
    """k_meta_force: the chain's sum, then the two differences of gP per site"""
    return SC.t_adj(t_gp(x, beta, tab, mutant)[0])


def t_action(x, beta, tab, mutant=None):
    """k_meta_action -> (S_b, Q_m, V)"""
    ssum, csum, _, _ = t_sums(x, mutant)
    q, V, c = t_bias(tab, ssum, mutant)
    return (-beta) * csum + V, q, V


def t_energy(x, v, beta, tab, mutant=None):
    """the biased plain sequence's energy: the plain H = S + K / 2 (stencil_cases.t_energy), then k_meta_energy: H + V, (Q_m, V).
      energy_second_block   chains >= 256 (the second workgroup of k_meta_energy) keep H without V"""
    h = SC.t_energy(x, v, beta)
    q, V, _ = t_bias(tab, t_sums(x, mutant)[0], mutant)
    hb = h + V
    if mutant == 'energy_second_block':
        hb[ENERGY_BLOCK:] = h[ENERGY_BLOCK:]
    return hb, q, V


def t_trajectory(x, v, u, beta, name, dt, nstep, tab, mutant=None):
    """the biased plain sequence (hmc_trajectory_call with its bias), launch by launch -> dict(H0, H1, dH, acc, x_new, qm, vbias; x_prop: the regularized end point of every
    chain, which the device hands out only where it accepts).
      select_proposed   qm / vbias of the proposed end point, whatever the accept"""
    b0, stages = IC.schedule(name, dt, nstep)
    H0, q0, V0 = t_energy(x, v, beta, tab, mutant)
    y = x + b0 * v
    p, at = v, y
    before = (None, q0) if mutant == 'stale_qm' else None
    if mutant == 'gp_one_pass':                          # the plane as an evaluation at the start field left it: finite, and stale
        before = (t_gp(x, beta, tab)[0], q0)
    for kind, a, b in stages:
        g, q = t_gp(at, beta, tab, mutant, before)
        before = (g, q)
        if kind == 'shift':
            at = SC.t_shift(g, y, a)
        else:
            p, y = SC.t_kick(g, p, y, a, b)
            at = y
    xr = SC.t_regularize(y)
    H1, q1, V1 = t_energy(xr, p, beta, tab, mutant)
    dH = H1 - H0
    with np.errstate(over='ignore', invalid='ignore'):
        acc = u < np.exp(-dH)
    keep = np.ones_like(acc) if mutant == 'select_proposed' else acc
    return {'H0': H0, 'H1': H1, 'dH': dH, 'acc': acc, 'x_new': np.where(acc[:, None, None, None], xr, x), 'qm': np.where(keep, q1, q0),
            'vbias': np.where(keep, V1, V0), 'x_prop': xr}


# ---------------------------------------------------------------- comparing
def angle_err(got, val):
    d = ld(got) - val
    return f64(np.abs(d - LD(TWO_PI) * np.rint(d / LD(TWO_PI))))


def worst(got, ref, angle=False):
    """-> (batch_kernel_cases.frac of |got - value| against the bound, the index where that fraction sits: the first nan's if it is nan)"""
    val, bound = ref
    err = angle_err(got, val) if angle else f64(np.abs(ld(got) - val))
    bound = np.broadcast_to(bound, err.shape)
    w = BC.frac(err, bound)
    if w != w:
        return w, tuple(int(k) for k in np.argwhere(np.isnan(err))[0])
    if w == 0.0:
        return w, (0,) * err.ndim
    with np.errstate(invalid='ignore', divide='ignore'):
        at = np.argwhere((err != 0.0) & (err / bound == w))[0]
    return w, tuple(int(k) for k in at)


FIELD_OUTPUTS = ('F', 'S', 'qm', 'vbias')
TRAJ_OUTPUTS = ('x_new', 'H0', 'H1', 'dH', 'qm', 'vbias')


def field_fracs(got, ref):
    """got: dict F, S, qm, vbias -> dict output -> (fraction, where)"""
    return {k: worst(got[k], ref[k]) for k in FIELD_OUTPUTS}


def traj_fracs(got, T):
    """-> (dict output -> (fraction, where), the accept flags are the reference's); x_prop (the twin's: the proposed end point of
    every chain, accepted or not, per link) where `got` has it"""
    f = {k: worst(got[k], getattr(T, 'xr' if k == 'x_new' else k), angle=k == 'x_new') for k in TRAJ_OUTPUTS}
    if 'x_prop' in got:
        f['x_prop'] = worst(got['x_prop'], T.xp, angle=True)
    return f, bool(np.array_equal(np.asarray(got['acc']) > 0.5, T.acc))


def worst_of(f):
    """(fraction, output, where) of the worst entry of a fracs dict; a nan wins"""
    k = max(f, key=lambda k: math.inf if f[k][0] != f[k][0] else f[k][0])
    return f[k][0], k, f[k][1]


def field_twin(x, tab, mutant=None):
    S, q, V = t_action(x, BETA, tab, mutant)
    return {'F': t_force(x, BETA, tab, mutant), 'S': S, 'qm': q, 'vbias': V}


def traj_twin(c, mutant=None):
    T = traj_reference(c)
    return t_trajectory(T.x, T.v, T.u, BETA, c.integrator, DT, c.nstep, T.tab, mutant)
