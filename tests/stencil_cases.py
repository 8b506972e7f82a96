"""The numpy side of the plain Wilson stencil tests (tests/test_stencils.py, tests/test_stencils_gpu.py): seeded hard inputs, a
numpy longdouble reference of every single operation of fthmc_amd/csrc/wilson.hip's stencil and trajectory kernels that carries its
own per-site error bound, a float64 twin in the kernels' operation order, and the named mutants of the twin.

Inputs (inputs()): links uniform in +-pi with second_order_cases.pin_links on chain 0 (links at +-(pi - 1e-9): the regularize / wrap
branch), the LAST chain with links of magnitude 27 .. 33 (a field that was never regularized; plaquette angles up to 132, inside
ft_sincos's stated |x| <= 1e5), momenta normal x 3.  Scalar beta = 2.5; per-chain beta (1.0, 2.5, 6.0).

Bounds, u = 2^-53, first order, every one a per-site array computed from the inputs' magnitudes (never from a device run); e(.) is
the bound carried by an operand, so the bounds of a multi-stage MD are the one-stage bounds propagated site by site through the
stencil (see r_md for how that relates to a Lipschitz factor):
  drift    y = x + a p                   e(x) + |a| e(p) + 2 u (|x| + |a p|)            (product and sum; one rounding if contracted)
  plaq     P = ((a - b) - c) + d         3 u (|a| + |b| + |c| + |d|) + e(a) + e(b) + e(c) + e(d)
  sin      s = sin P                     e(P) + 5 u |s|      (|sin'| <= 1; ft_sincos is within 2.5 ulp <= 5 u |s|: common.h, held by
                                                              tests/test_device_math_gpu.py)
  seed     g = beta s                    beta e(s) + u |g|
  force    f0 = g(s) - g(s - j), f1 = g(s - i) - g(s)        the two e(g) + u |f|
  kick     p' = p - dt f                 e(p) + |dt| e(f) + u (|dt f| + |p'|)
  shift    xs = x - c f                  the drift's form
  regularize  2 pi (f_ - floor(f_) - 1/2), f_ = (x - pi) / 2 pi        e(x) + 2 u (|x| + pi) + 2 pi u + u |r|   (difference, quotient; the floor
                                         is exact; f_ - floor(f_) lands in [0, 1) and rounds by up to 2^-54 where f_ < 0 carries
                                         a finer spacing, - 1/2 by up to 2^-55: 2 pi u covers both times 2 pi; the product)
  wrap     remainder(x + pi, 2 pi) - pi  e(x) + 2 u (|x| + 2 pi)       (x + pi, + 2 pi for a negative remainder, - pi)
  H = S + K / 2                          batch_kernel_cases.action_bounds and kinetic_cap (see r_energy)
regularize and wrap jump by 2 pi at their branch: the reference's distance to it (margin) is reported and asserted on the CPU.
Every bound is widened by SLACK = 1 + 2^-8 for the reference's own rounding: longdouble carries 2^-64 = 2^-11 u per operation, a
reference value is at most a few dozen of them from exact, and the second-order terms (u^2) are far below that."""
import collections
import functools
import math

import numpy as np

import batch_kernel_cases as BC
import integrator_cases as IC
from second_order_cases import pin_links

U = BC.U
LD = np.longdouble
SLACK = 1.0 + 2.0 ** -8
PI, TWO_PI = math.pi, 2.0 * math.pi           # FT_PI, FT_TWO_PI of common.h: the same doubles
BIG = 30.0
BETA, PB_BETAS = 2.5, (1.0, 2.5, 6.0)
DT = 0.05
TS = 16                                       # k_force's tile
STRIDE_SITES = 64 * 256                       # the grid cap of k_kick_from_gp / k_shift_from_gp / k_plaq: sites per pass
INTEGRATORS = IC.NAMES
U_ACCEPT, U_REJECT = 0.0, 1.0 - 2.0 ** -53    # accept whatever dH < 700; reject whatever dH > 2^-53
DH_MAX = 700.0                                # exp(-dH) > 0 on the device below this

Case = collections.namedtuple('Case', 'id seed B L beta dt a integrator')


def _case(L, integrator='leapfrog', pb=False, tag=''):
    B = 2 if L in (16, 48, 128, 132, 60) else 3
    beta = PB_BETAS[:B] if pb else BETA
    return Case(f'L{L}{tag}', 31000 + L, B, L, beta, DT, 0.5 * DT, integrator)


# lattice -> the kernels it selects: 4, 12, 16 tile kernels with the slow wrap (16 one exact tile); 20, 36 ragged, fast wrap; 48 three
# exact tiles; 68 ragged past a row-strip size; 132 ragged and past one pass of the grid-stride kernels; 64, 128 row strips
STENCIL_L = (4, 12, 16, 20, 36, 48, 68, 132, 64, 128)
MD_L = (4, 20, 68, 132, 64, 128)
ONE_LAUNCH_L = (4, 8, 36, 60, 64)
MULTI_LAUNCH_L = (8, 36, 68, 132)             # 8, 36: with the VALU variant, which has no one-launch kernel
PB_L = (20, 68, 128)
ROW_L = (64, 128)
LEAP_NSTEP, MD_NSTEP, TRAJ_NSTEP = (1, 3), (1, 2), (1, 2)
STENCIL_CASES = [_case(L) for L in STENCIL_L]
MD_CASES = [_case(L, name) for L in MD_L for name in INTEGRATORS[1:]]
TRAJ_CASES = [_case(L, name) for L in sorted(set(ONE_LAUNCH_L + MULTI_LAUNCH_L)) for name in INTEGRATORS]
PB_CASES = [_case(L, name, pb=True, tag='pb') for L in PB_L for name in INTEGRATORS]
CASES = STENCIL_CASES + MD_CASES + TRAJ_CASES + PB_CASES


def case_id(c):
    return f'{c.id}-{c.integrator}'


@functools.lru_cache(maxsize=None)
def inputs(seed, B, L):
    """-> (x, p) [B, 2, L, L] float64, made once and never modified (read-only arrays)"""
    rng = np.random.default_rng(seed)
    x = pin_links(rng.uniform(-PI, PI, (B, 2, L, L)))
    x[B - 1] += BIG * (rng.integers(0, 2, (2, L, L)) * 2 - 1)
    p = 3.0 * rng.normal(size=(B, 2, L, L))
    x.setflags(write=False); p.setflags(write=False)
    return x, p


def ld(a):
    return np.asarray(a, dtype=LD)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def mag(a):
    return np.abs(f64(a))


def nb(a, di, dj):
    """a at site (i + di, j + dj), periodic"""
    return np.roll(a, (-di, -dj), axis=(-2, -1))


def bcol(beta, dtype):
    return np.asarray(beta, dtype=dtype).reshape(-1, 1, 1)


# ---------------------------------------------------------------- the longdouble reference with its bounds: (value, bound) pairs
def exact(a):
    a = ld(a)
    return a, np.zeros(a.shape)


def r_plaq(x, ex):
    a, b = x[:, 0], x[:, 1]
    c, d = nb(a, 0, 1), nb(b, 1, 0)
    e = 3 * U * (mag(a) + mag(b) + mag(c) + mag(d)) + ex[:, 0] + ex[:, 1] + nb(ex[:, 0], 0, 1) + nb(ex[:, 1], 1, 0)
    return (a + d) - (b + c), e


def r_gp(x, ex, beta):
    P, eP = r_plaq(x, ex)
    s = np.sin(P)
    es = eP + 5 * U * mag(s)
    g = bcol(beta, LD) * s
    return g, bcol(beta, np.float64) * es + U * mag(g)


def r_force_of(g, eg):
    f0, f1 = g - nb(g, 0, -1), nb(g, -1, 0) - g
    return np.stack([f0, f1], 1), np.stack([eg + nb(eg, 0, -1) + U * mag(f0), nb(eg, -1, 0) + eg + U * mag(f1)], 1)


def r_force(x, ex, beta):
    return r_force_of(*r_gp(x, ex, beta))


def r_axpy(x, ex, p, ep, a):
    ap = LD(a) * p
    return x + ap, ex + abs(a) * ep + 2 * U * (mag(x) + mag(ap))


def r_kick(p, ep, F, eF, dt):
    t = LD(dt) * F
    q = p - t
    return q, ep + abs(dt) * eF + U * (mag(t) + mag(q))


def r_regularize(x, ex):
    f_ = (x - LD(PI)) / LD(TWO_PI)
    r = LD(TWO_PI) * (f_ - np.floor(f_) - LD(0.5))
    return r, ex + 2 * U * (mag(x) + PI) + 2 * PI * U + U * mag(r)


def r_wrap(x, ex):
    r = np.remainder(x + LD(PI), LD(TWO_PI)) - LD(PI)
    return r, ex + 2 * U * (mag(x) + TWO_PI)


def branch_margin(x):
    """distance of every link to the branch of regularize and of wrap (both at pi mod 2 pi)"""
    f_ = f64((ld(x) - LD(PI)) / LD(TWO_PI))
    return float(np.min(np.abs(f_ - np.round(f_))) * TWO_PI)


def r_md(x, p, beta, name, dt, nstep):
    """-> ((x', e), (p', e)) of the MD `name`, by the schedule of integrator_cases (its own statement of the three integrators).
    The stage's bound is propagated site by site: e(P) takes the e(x) of its own four links, e(f) of a link the e(g) of its two
    plaquettes.  In the maximum norm that is the Lipschitz factor the stencil gives: a link touches two plaquettes, a plaquette
    four links, so |dF| <= c beta max|dx| with c = 2 x 4 = 8 and a stage multiplies a uniform bound by at most
    (1 + 8 beta a (b + ...)); the site-resolved form never exceeds that and keeps a chain of small links apart from the chain of
    large ones."""
    b0, stages = IC.schedule(name, dt, nstep)
    X = r_axpy(*exact(x), *exact(p), b0)
    Pm = exact(p)
    at = X
    for kind, a, b in stages:
        F = r_force(at[0], at[1], beta)
        if kind == 'shift':
            at = r_axpy(*X, *F, -a)
        else:
            Pm = r_kick(*Pm, *F, a)
            X = r_axpy(*X, *Pm, b)
            at = X
    return X, Pm



def r_energy(x, ex, v, ev, beta):
    """-> (H, S, K) [B] longdouble and the bound on H.  S: batch_kernel_cases.action_bounds per chain (the angle in the kernels'
    order, a cosine within 2 ulp, the workgroup sum) + beta u L^2 for ft_sincos's cosine in the one-launch kernels (2.5 ulp = 5 u
    where action_bounds has 4 u) + the roundings of a sum by 1024 threads where action_bounds counts fewer + 2 beta sum e(x): a link
    enters two plaquettes and |d cos| <= |dP|.  K: batch_kernel_cases.kinetic_cap (k_kinetic's count) + (ceil(L^2 / 1024) + 11) u K
    for the one-launch kernels' order (v0^2 + v1^2 per site, the thread's sites, the tree, 16 waves: ceil(L^2 / 1024) + 24 in all
    where the cap has 13) + 2 sum |v| e(v).  H = S + 0.5 K: 0.5 K is exact, the sum rounds once; 2 u |H| is kept."""
    B, _, L, _ = x.shape
    P, _ = r_plaq(x, np.zeros(x.shape))
    cs = np.cos(P)
    bb = bcol(beta, LD).reshape(-1)
    S = -(bb * cs.reshape(B, -1).sum(axis=1))
    K = (v * v).reshape(B, -1).sum(axis=1)
    H = S + LD(0.5) * K
    bv = np.broadcast_to(f64(bb), (B,))
    x64, v64 = f64(x), f64(v)
    bS = np.empty(B)
    for b in range(B):
        s_ref = f64(S[b:b + 1])
        bS[b] = BC.action_bounds(x64[b:b + 1], s_ref, -s_ref / (bv[b] * L * L), float(bv[b]))[0][0]
    more = max(0, BC.sum_roundings(L * L, 1024) - BC.sum_roundings(L * L, BC.nt_action(L)))
    bS = bS + bv * U * (L * L + more * mag(cs).reshape(B, -1).sum(axis=1)) + 2 * bv * ex.reshape(B, -1).sum(axis=1)
    bK = BC.kinetic_cap(v64, f64(K)) + (-(-L * L // 1024) + 11) * U * f64(K) + 2 * (mag(v) * ev).reshape(B, -1).sum(axis=1)
    return (H, S, K), bS + 0.5 * bK + 2 * U * mag(H)


def hold(pair):
    """(value, bound) -> (value, the bound a result is held to)"""
    return pair[0], pair[1] * SLACK


# ---------------------------------------------------------------- what a case's reference holds, computed once and shared
@functools.lru_cache(maxsize=None)
def stencil_reference(c):
    """single operations at the case's inputs -> dict name -> (value, bound):
    plaq, gp, force, step (one fused step: x' = x + a p, p' = p - dt F(x')), kick (v' = v - dt adj(gP), x' = x + a v'), shift
    (x - c adj(gP), c = dt^2 / 24), regularize, wrap"""
    x, p = inputs(c.seed, c.B, c.L)
    X, Pm = exact(x), exact(p)
    out = {'plaq': r_plaq(*X), 'gp': r_gp(*X, c.beta), 'force': r_force(*X, c.beta)}
    y = r_axpy(*X, *Pm, c.a)
    out['step_x'] = y
    out['step_p'] = r_kick(*Pm, *r_force(*y, c.beta), c.dt)
    v1 = r_kick(*Pm, *out['force'], c.dt)
    out['kick_v'], out['kick_x'] = v1, r_axpy(*X, *v1, c.a)
    out['shift'] = r_axpy(*X, *out['force'], -c.dt * c.dt / 24.0)
    out['regularize'], out['wrap'] = r_regularize(*X), r_wrap(*X)
    return {k: hold(v) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def md_reference(c, nstep):
    X, Pm = r_md(*inputs(c.seed, c.B, c.L), c.beta, c.integrator, c.dt, nstep)
    return {'x': hold(X), 'p': hold(Pm)}


Traj = collections.namedtuple('Traj', 'seed x v u H0 H1 dH xr accept rejected redraws margin above_one')


@functools.lru_cache(maxsize=None)
def traj_reference(c, nstep):
    """The case's trajectory with its accept draws fixed on the REFERENCE's numbers: chain b draws u = 0 (accepted whatever the
    round-off: exp(-dH) > 0 for dH < 700) unless it is the chain chosen to be rejected, which draws the largest double below 1 and
    has a reference dH above twice its bound + 4 u (so the device's dH is above 2^-53 and exp(-dH) < 1 - 2^-53 is not above u);
    a chain with dH >= 700 is a rejected one as well.  The first chain that qualifies is the rejected one; if none does, or no
    accepted chain is left, the seed is redrawn by integrator_cases.decided_case's rule (seed + 1000, at most 3 times); what
    happens where that does not help either is said at the end (above_one).
    H0, H1, dH, xr: (value, bound) pairs; xr the regularized end point."""
    kept = None
    for k in range(4):
        seed = c.seed + 1000 * k
        x, v = inputs(seed, c.B, c.L)
        z = np.zeros(x.shape)
        (H0, _, _), bH0 = r_energy(ld(x), z, ld(v), z, c.beta)
        X, Pm = r_md(x, v, c.beta, c.integrator, c.dt, nstep)
        xr = r_regularize(*X)
        (H1, _, _), bH1 = r_energy(xr[0], xr[1], Pm[0], Pm[1], c.beta)
        dH = H1 - H0
        bdH = bH0 + bH1 + U * mag(dH)
        d64 = f64(dH)
        can_reject = d64 > 2 * bdH * SLACK + 4 * U
        forced = d64 >= DH_MAX
        first = int(np.argmax(can_reject)) if can_reject.any() else -1
        rejected = forced.copy()
        if first >= 0:
            rejected[first] = True
        u = np.where(rejected, U_REJECT, U_ACCEPT)
        if kept is None:
            kept = (seed, x, v, H0, bH0, H1, bH1, dH, bdH, xr, X)
        if first >= 0 and not rejected.all():
            return Traj(seed, x, v, u, hold((H0, bH0)), hold((H1, bH1)), hold((dH, bdH)), hold(xr), ~rejected, rejected, k,
                        branch_margin(X[0]), False)
    # every chain of all four draws loses energy by more than its bound (the short Omelyan trajectories from these hot fields at
    # L >= 36 do, systematically): exp(-dH) > 1 whatever the round-off and no uniform below 1 is rejected.  The first draw is kept
    # and its chain of largest dH is rejected by u = 2 exp(-dH): outside a uniform's range, decided by a factor of 2 where the
    # bound on dH moves exp(-dH) by 1e-8 of itself, through the same comparison u < exp(-dH).
    seed, x, v, H0, bH0, H1, bH1, dH, bdH, xr, X = kept
    d64 = f64(dH)
    assert np.all(d64 < -2 * bdH * SLACK) and c.B >= 2, (case_id(c), nstep, d64)
    rejected = np.arange(c.B) == int(np.argmax(d64))
    u = np.where(rejected, 2.0 * np.exp(-d64), U_ACCEPT)
    return Traj(seed, x, v, u, hold((H0, bH0)), hold((H1, bH1)), hold((dH, bdH)), hold(xr), ~rejected, rejected, 0, branch_margin(X[0]), True)


# ---------------------------------------------------------------- the float64 twin, in the kernels' operation order
MUTANTS = ('halo_left_unwrapped', 'kick_neighbours_swapped', 'row_wrap_missing', 'ragged_last_column', 'single_wrap_L4',
           'full_last_drift', 'no_regularize', 'beta0_everywhere', 'shift_kept', 'reject_regularized', 'stride_skipped')


def t_plaq(x):
    a, b = x[:, 0], x[:, 1]
    return ((a - b) - nb(a, 0, 1)) + nb(b, 1, 0)                          # k_plaq, k_force, k_gp_rows, the one-launch kernels


def _beta(beta, mutant):
    return np.asarray(beta, dtype=np.float64).reshape(-1)[:1] if mutant == 'beta0_everywhere' else beta


def t_gp(x, beta, mutant=None):
    return bcol(_beta(beta, mutant), np.float64) * np.sin(t_plaq(x))


def t_adj(g, mutant=None):
    """adj(gP): f0 = gc - g[i][j - 1], f1 = g[i - 1][j] - gc (k_kick_from_gp / k_shift_from_gp / k_force).  Mutants:
      halo_left_unwrapped      g[i][-1] read at flat index i L - 1 of the chain: site (i - 1, L - 1)
      kick_neighbours_swapped  g[i][j + 1] in place of g[i][j - 1]
      row_wrap_missing         g[-1][j] read L doubles before the chain: the last row of the chain before it"""
    B, L = g.shape[0], g.shape[-1]
    gl, gu = nb(g, 0, -1), nb(g, -1, 0)
    if mutant == 'halo_left_unwrapped':
        gl = np.roll(g.reshape(B, -1), 1, axis=1).reshape(g.shape)
    elif mutant == 'kick_neighbours_swapped':
        gl = nb(g, 0, 1)
    elif mutant == 'row_wrap_missing':
        gu = np.roll(g.reshape(-1), L).reshape(g.shape)
    return np.stack([g - gl, gu - g], 1)


def _ragged(out, mutant):
    """ragged_last_column: column L - 1 of a lattice that is no whole number of tiles is never written (the buffers are NaN-filled)"""
    if mutant == 'ragged_last_column' and out.shape[-1] % TS:
        out = out.copy()
        out[..., -1] = np.nan
    return out


def _strided(new, old, mutant):
    """stride_skipped: the first pass only of k_kick_from_gp / k_shift_from_gp (a grid of at most 64 x 256 threads, one site of both
    planes each) -- sites >= 16384 of a chain keep what they held"""
    L = new.shape[-1]
    if mutant != 'stride_skipped' or L * L <= STRIDE_SITES:
        return new
    B = new.shape[0]
    out = new.copy().reshape(B, -1, L * L)
    out[:, :, STRIDE_SITES:] = np.broadcast_to(old, new.shape).reshape(B, -1, L * L)[:, :, STRIDE_SITES:]
    return out.reshape(new.shape)


def t_force(x, beta, mutant=None):
    if mutant == 'single_wrap_L4':
        return t_force_tiles(x, beta, once=True)
    return _ragged(t_adj(t_gp(x, beta, mutant), mutant), mutant)


def t_step(x, p, beta, a, dt, mutant=None):
    """one fused step as k_force<1> / k_leap_rows write it: x' = x + a p; p' = p - dt F(x')"""
    y = x + a * p
    return _ragged(y, mutant), _ragged(p - dt * t_force(y, beta, mutant), mutant)


def t_kick(g, v, x, dt, a, mutant=None):
    """k_kick_from_gp as written: v0 = v - dt f; y0 = x + a v0"""
    f = t_adj(g, mutant)
    v1 = v - dt * f
    return _strided(v1, v, mutant), _strided(x + a * v1, x, mutant)


def t_shift(g, x, c, mutant=None):
    return _strided(x - c * t_adj(g, mutant), np.nan, mutant)


def t_regularize(x):
    f_ = (x - PI) / TWO_PI
    return TWO_PI * (f_ - np.floor(f_) - 0.5)


def t_wrap(x):
    return np.remainder(x + PI, TWO_PI) - PI


def t_leapfrog(x, p, beta, dt, nstep, mutant=None):
    """fthmc_leapfrog: nstep fused steps (a = dt / 2 first, dt after), then the half drift.  full_last_drift: dt there."""
    for k in range(nstep):
        x, p = t_step(x, p, beta, 0.5 * dt if k == 0 else dt, dt, mutant)
    return x + (dt if mutant == 'full_last_drift' else 0.5 * dt) * p, p


def t_md(x, p, beta, name, dt, nstep, mutant=None):
    """ft_md_ws with zero layers / k_hmc_trajectory_sched: x += b0 v, then per stage the seed gP and KICK(a, b) or SHIFT(c).
      full_last_drift   the last stage drifts by the stage before's b (leapfrog: dt for dt / 2)
      shift_kept        the shifted field stays in place of the links behind a SHIFT stage"""
    b0, stages = IC.schedule(name, dt, nstep)
    if mutant == 'full_last_drift':
        full = dt if name == 'leapfrog' else (2.0 * IC.LAMBDA * dt if name == 'omelyan' else 0.5 * dt)
        stages = stages[:-1] + [(stages[-1][0], stages[-1][1], full)]
    x = x + b0 * p
    at = x
    for kind, a, b in stages:
        g = _ragged(t_gp(at, beta, mutant), mutant)
        if kind == 'shift':
            at = t_shift(g, x, a, mutant)
            if mutant == 'shift_kept':
                x = at
        else:
            p, x = t_kick(g, p, x, a, b, mutant)
            at = x
    return x, p


def t_energy(x, v, beta):
    B = x.shape[0]
    bb = np.broadcast_to(np.asarray(beta, dtype=np.float64).reshape(-1), (B,))
    S = np.array([BC.action_twin(x[b:b + 1], float(bb[b]))[0][0] for b in range(B)])
    return S + 0.5 * BC.kinetic_twin(v)


def t_trajectory(x, v, u, beta, name, dt, nstep, mutant=None):
    """-> dict(H0, H1, dH, acc, x_new).  no_regularize: the end point as the MD left it; reject_regularized: a rejected chain
    returned as regularize(x); stride_skipped: k_metropolis's first pass only -- its min(16, ceil(2 L^2 / 2048)) workgroups of 256
    threads write that many links of the chain's flat 2 L^2 and the rest stays NaN"""
    bt = _beta(beta, mutant)
    H0 = t_energy(x, v, bt)
    if name == 'leapfrog':
        x1, v1 = t_leapfrog(x, v, bt, dt, nstep, mutant)
    else:
        x1, v1 = t_md(x, v, bt, name, dt, nstep, mutant)
    xr = x1 if mutant == 'no_regularize' else t_regularize(x1)
    H1 = t_energy(xr, v1, bt)
    dH = H1 - H0
    with np.errstate(over='ignore', invalid='ignore'):
        acc = u < np.exp(-dH)
    old = t_regularize(x) if mutant == 'reject_regularized' else x
    x_new = np.where(acc[:, None, None, None], xr, old)
    if mutant == 'stride_skipped':
        B, n2 = x_new.shape[0], x_new[0].size
        x_new = x_new.copy()
        x_new.reshape(B, n2)[:, min(16, -(-n2 // 2048)) * 256:] = np.nan
    return {'H0': H0, 'H1': H1, 'dH': dH, 'acc': acc, 'x_new': x_new}


def wrap_once(w, L):
    """k_force's fast wrap: min(w, w - L, w + L) taken as unsigned"""
    w = np.asarray(w, dtype=np.int64)
    return np.minimum(np.minimum(w.astype(np.uint32), (w - L).astype(np.uint32)), (w + L).astype(np.uint32)).astype(np.int64)


def window_in_range(L, once=False):
    """every window index k_force forms for lattice L lies inside the lattice (once: with the fast wrap whatever L)"""
    w = np.arange(0, L, TS)[:, None] - 1 + np.arange(TS + 2)[None, :]
    w = wrap_once(w, L) if (once or L >= TS + 2) else (w + L) % L
    return bool(np.all((w >= 0) & (w < L)))


def t_force_tiles(x, beta, once=False):
    """k_force<0> tile by tile: the (TS + 1) x (TS + 2) and (TS + 2) x (TS + 1) link windows gathered at wrapped indices, beta sin P on
    the (TS + 1)^2 window, two differences per site; sites outside the lattice are not written (NaN).  once: the fast wrap for
    every L (mutant single_wrap_L4; an index past the chain reads on into what lies behind it, as the device would).  That mutant
    changes no value: the sites of the lattice use window lines -1 .. L only, which one wrap serves; what wrapping several times
    protects is the range of the READS (an 18-wide window at L = 4 would read up to index 60 of a 16-site plane), so the mutant is
    caught by the exact statement window_in_range, not by a bound."""
    B, _, L, _ = x.shape
    n = L * L
    flat = x.reshape(-1)
    bb = np.broadcast_to(np.asarray(beta, dtype=np.float64).reshape(-1), (B,))
    wr = (lambda w: wrap_once(w, L)) if (once or L >= TS + 2) else (lambda w: (np.asarray(w) + L) % L)
    F = np.full(x.shape, np.nan)
    r17, r18 = np.arange(TS + 1), np.arange(TS + 2)
    for b in range(B):
        for i0 in range(0, L, TS):
            for j0 in range(0, L, TS):
                at0 = wr(i0 - 1 + r17)[:, None] * L + wr(j0 - 1 + r18)[None, :]
                at1 = wr(i0 - 1 + r18)[:, None] * L + wr(j0 - 1 + r17)[None, :]
                sx0 = np.take(flat, b * 2 * n + at0, mode='wrap')
                sx1 = np.take(flat, b * 2 * n + n + at1, mode='wrap')
                sp = bb[b] * np.sin(((sx0[:, :TS + 1] - sx1[:TS + 1, :]) - sx0[:, 1:]) + sx1[1:, :])
                s = sp[1:, 1:]
                ni, nj = min(TS, L - i0), min(TS, L - j0)
                F[b, 0, i0:i0 + ni, j0:j0 + nj] = (s - sp[1:, :-1])[:ni, :nj]
                F[b, 1, i0:i0 + ni, j0:j0 + nj] = (sp[:-1, 1:] - s)[:ni, :nj]
    return F


# ---------------------------------------------------------------- comparing
def frac(got, ref):
    """worst |got - value| / bound of a (value, bound) pair (nan if anything is nan)"""
    val, bound = ref
    return BC.frac(f64(np.abs(ld(got) - val)), bound)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def stencil_twin(c, mutant=None):
    """the twin's answer to every entry of stencil_reference(c)"""
    x, p = inputs(c.seed, c.B, c.L)
    g = _ragged(t_gp(x, c.beta, mutant), mutant)
    out = {'plaq': t_plaq(x), 'gp': g, 'force': t_force(x, c.beta, mutant)}
    out['step_x'], out['step_p'] = t_step(x, p, c.beta, c.a, c.dt, mutant)
    out['kick_v'], out['kick_x'] = t_kick(g, p, x, c.dt, c.a, mutant)
    out['shift'] = t_shift(g, x, c.dt * c.dt / 24.0, mutant)
    out['regularize'], out['wrap'] = t_regularize(x), t_wrap(x)
    return out


def traj_fracs(got, T):
    """-> (dict of worst fractions for H0, H1, dH and the accepted chains' x_new, every exact assertion holds): the accept flags
    are T's, a rejected chain's x_new is x bit for bit"""
    f = {k: frac(got[k], getattr(T, k)) for k in ('H0', 'H1', 'dH')}
    acc = np.asarray(got['acc']) > 0.5
    a, r = np.nonzero(T.accept)[0], np.nonzero(T.rejected)[0]
    f['x_new'] = frac(np.asarray(got['x_new'])[a], (T.xr[0][a], T.xr[1][a]))
    ok = np.array_equal(acc, T.accept) and np.array_equal(bits(np.asarray(got['x_new'])[r]), bits(T.x[r]))
    return f, ok
