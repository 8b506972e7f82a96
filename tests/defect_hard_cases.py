"""The numpy side of the hard-input tests of boundary-condition tempering (tests/test_defect_hard.py, tests/test_z_defect_hard_gpu.py):
the shapes at which the launch geometry of fthmc_amd/csrc/defect.hip and of the sequenced trajectory (defect_trajectory_call,
csrc/api.hip) changes, stencil_cases' hard inputs, a long double reference of every operation that carries its own per-site / per-chain
error bound, a float64 twin in the kernels' operation and summation order (both trajectory paths, the translation) and the named
mutants of the twin.  Built on defect_cases (defect_of, couplings; the definitions and trajectory(), against which the reference here
is cross-checked on the CPU), stencil_cases (inputs, the per-operation bound forms, SLACK, the site-by-site propagation, U_ACCEPT /
U_REJECT), batch_kernel_cases (sum_roundings, action_bounds, kinetic_cap through stencil_cases.r_energy) and meta_hard_cases
(sum_count, the comparison helpers).

Shapes (beta = 2.5, dt = 0.05, nstep 1 and 2, the three integrators rotating; see SHAPES and test_defect_hard.py, which computes what
each reaches from the launchers' arithmetic):
  batch  B 258   L 4    paths 1, 2   chains 256, 257 in k_defect_energy's second workgroup and its b >= B guard
  L36    B 2     L 36   paths 1, 2   512-thread sums: 2 passes + 272 sites; one-launch kernel: 1 pass + 272
  L60    B 2     L 60   paths 1, 2   512 threads: 7 passes + 16; one-launch kernel: 3 passes + 528
  L132   B 2     L 132  path 2       1040 sites in the second pass of k_defect_gp / k_defect_force / k_defect_translate (nstep 1,
                                     leapfrog and force-gradient)
  slice  B 65537 L 4    force, action and translate only: chains 65535, 65536 in the second slice of launch_defect_force / _translate
Defects (defect_of): defect_cases' one, full, wrap and col0; end = (L - 1, L - 1, L): the line starts on the last row, every i but one
takes df_on's a + L branch; at L = 132 straddle = (120, 5, 12), whose plaquettes (124, 5) = site 16373 and (125, 5) = site 16505 lie
either side of the pass edge 16384, and wrapback = (128, 131, 8), which starts in the second pass and wraps into the first.
Couplings: defect_cases.couplings, g_b = (0, beta / 3, beta)[(b + k) % 3]: three different values on chains 255 .. 257; the slice
takes the same below 65535 and (k + 1) % 3, k % 3 on chains 65535, 65536: three different values on 65534 .. 65536, and chains 65535,
65536 differ from chains 0, 1, which a second slice that read g_b from its start would hand them.
Inputs: stencil_cases.inputs (links +-pi, chain 0 with pinned links at +-(pi - 1e-9), the last chain shifted by +-30, momenta x 3); the
uniforms of the accept are drawn from seed + 17.  Every trajectory case holds an accepted and a rejected chain, so that the selection
of (C, Dsum, Q) between the two ends is tested: where the draw accepts none, chain 0 (the first chain with dH < 700) draws U_ACCEPT;
where it rejects none, chain 1 (else the first chain whose dH is above twice its bound + 4 u) draws U_REJECT, and where no chain's dH
is, the chain of largest dH draws 2 exp(-dH) (stencil_cases.traj_reference's rule); `forced` records what was done.

Bounds, u = 2^-53, first order, arrays per site or per chain computed from the inputs' magnitudes, never from a device run; e(.) is
the bound an operand carries.  stencil_cases' forms for plaq, sin (ft_sincos within 2.5 ulp <= 5 u), force, kick, shift, drift,
regularize and the bracket H_p = (-beta) C + K / 2 (stencil_cases.r_energy).  New here:
  w     the weight of a site is a SELECTION (g_b on the defect, beta elsewhere): exact, no bound
  gP    = w sin P: stencil_cases' seed form with w per site     |w| e(sin P) + u |gP|       (w = 0: gP = +-0 exactly, the bound 0)
        k_defect_gp forms it once per site, k_defect_force three times per site (the centre, the left and the upper plaquette, each
        with the weight of ITS site): the same expression of the same links, the same bound; the one-launch kernel decides the
        weight once per owned site
  C     = sum cos P: batch_kernel_cases.action_bounds at beta = 1 (the angle in the kernels' order, a cosine within 2 ulp, R + 4
        roundings of the sum with R = sum_roundings(n, chain_threads(L)), 2 u |C|); + u n for ft_sincos's cosine in the one-launch
        kernel (5 u where action_bounds has 4 u); + (R' - R) u sum |cos P| where meta_hard_cases.sum_count's R' (the one-launch
        kernel's 1024-thread sum) is the larger; + 2 sum e(x): a link enters two plaquettes, |d cos| <= |dP|
  Dsum  the same over the defect's Ld terms only (the other threads add an exact 0.0), the same R:
        u [Ld (9 pi mu + 4) + (R + 4) sum_D |cos P|] + u [Ld + (R' - R) sum_D |cos P|] + 2 u |Dsum| + sum_D e(P), e(P) the sum of
        the e(x) of the plaquette's four links; Ld = 0: Dsum = 0.0 exactly
  S_d   = (-beta) C + (beta - g) Dsum     e((-beta) C) [action_bounds at beta: the product's rounding is in it, + beta times the
        extras of C] + |beta - g| e(Dsum) + 2 u |(beta - g) Dsum| [the difference beta - g and the product] + u |S_d| [the sum]
  H     = ((-beta) C + K / 2) + (beta - g) Dsum     e(H_p) [r_energy] + |beta - g| e(Dsum) + 2 u |(beta - g) Dsum| + u |H|
  Q     the integer charge rint(sum wrap(P) / 2 pi) is compared EXACTLY, where every plaquette's distance to the branch of the wrap
        (pi mod 2 pi) exceeds 8 e(P) (8: the device's P may be e(P) from the reference's, the twin's another; a factor 4 in hand); the
        sum of n wrapped angles is then within n pi (R' + 2) u of a multiple of 2 pi, far from rint's branch
Through an MD the bounds go site by site through the stencil as in stencil_cases.r_md, with w per site in the seed.
An accept is compared where |u - exp(-dH)| > exp(-dH) (2 e(dH) + 4 u) (meta_hard_cases' rule).  Both are conditions on the inputs;
where a draw misses one the seed is redrawn by integrator_cases.decided_case's rule (seed + 1000, at most 3 times), and on the
committed seeds NO chain is left out of either (test_defect_hard.py asserts it with the reference alone).
Every bound is widened by stencil_cases.SLACK = 1 + 2^-8 for the reference's own rounding (2^-11 u per operation)."""
import collections
import functools
import math

import numpy as np

import batch_kernel_cases as BC
import defect_cases as DC
import integrator_cases as IC
import meta_hard_cases as MH
import stencil_cases as SC

U, LD, SLACK = SC.U, SC.LD, SC.SLACK
PI, TWO_PI = SC.PI, SC.TWO_PI
BETA, DT = SC.BETA, SC.DT
NSTEPS = (1, 2)
INTEGRATORS = IC.NAMES
STRIDE_SITES = 64 * 256              # df_stride_grid: at most 64 workgroups of 256 threads, one site each per pass
ENERGY_BLOCK = 256                   # launch_defect_energy: chains per workgroup
SLICE = 65535                        # launch_defect_force / launch_defect_translate: chains per launch (grid y)
ONE_LAUNCH_NT, ONE_LAUNCH_MAXL = 1024, 64          # k_defect_trajectory (TJ_NT, TJ_MAXL)
MARGIN = 8.0
ld, f64, mag, nb = SC.ld, SC.f64, SC.mag, SC.nb
chain_threads = MH.chain_threads
sum_count = MH.sum_count
worst, worst_of, angle_err = MH.worst, MH.worst_of, MH.angle_err

Case = collections.namedtuple('Case', 'shape seed B L kind nstep integrator paths')

# id -> (B, L, defect kinds, paths); the slice has no trajectory
SHAPES = collections.OrderedDict([
    ('batch', (258, 4, ('one', 'full', 'wrap', 'col0', 'end'), (1, 2))),
    ('L36', (2, 36, ('wrap', 'col0', 'end'), (1, 2))),
    ('L60', (2, 60, ('one', 'full', 'end'), (1, 2))),
    ('L132', (2, 132, ('full', 'end', 'straddle', 'wrapback'), (2,))),
    ('slice', (65537, 4, ('wrap', 'end'), ())),
])
KINDS = ('one', 'full', 'wrap', 'col0', 'end', 'straddle', 'wrapback')


def defect_of(kind, L):
    """defect_cases.defect_of's kinds, end (a line of L that starts on the last row) and, at L = 132, straddle and wrapback"""
    if kind == 'end':
        return (L - 1, L - 1, L)
    if kind in ('straddle', 'wrapback'):
        assert L == 132
        return (120, 5, 12) if kind == 'straddle' else (128, 131, 8)
    return DC.defect_of(kind, L)


def couplings(B, k):
    """g_b per chain, mixed out of {0, beta / 3, beta} (see the module docstring for the chains of a second slice)"""
    g = DC.couplings(B, BETA, k)
    vals = (0.0, BETA / 3.0, BETA)
    for r, b in enumerate(range(SLICE, B)):
        g[b] = vals[(k + 1 - r) % 3]
    return g


def _cases():
    out, k = [], 0
    for sid, (B, L, kinds, paths) in SHAPES.items():
        for dk in kinds:
            if not paths:
                runs = [(0, 'none')]
            elif sid == 'L132':                      # nstep 1 only: leapfrog (one stage) and force-gradient (kick, shift, kicks)
                runs = [(1, 'leapfrog'), (1, 'force_gradient')]
            else:
                runs = []
                for n in NSTEPS:
                    runs.append((n, INTEGRATORS[k % 3]))
                    k += 1
            for n, integ in runs:
                out.append(Case(sid, 52000 + 10 * L + B % 1000 + 100 * KINDS.index(dk), B, L, dk, n, integ, paths))
    return tuple(out)


ALL_CASES = _cases()
CASES = tuple(c for c in ALL_CASES if c.paths)                                  # the trajectories
FIELD_CASES = tuple({(c.shape, c.kind): c for c in ALL_CASES}.values())         # force and action see no nstep and no integrator


def case_id(c):
    return f'{c.shape}-{c.kind}-n{c.nstep}-{c.integrator}'


def field_id(c):
    return f'{c.shape}-{c.kind}'


def setup(c):
    """-> (g [B], defect)"""
    return couplings(c.B, KINDS.index(c.kind)), defect_of(c.kind, c.L)


# ---------------------------------------------------------------- the long double reference with its bounds
def r_weights(L, g, df):
    """w[B][L][L] in long double: a selection, exact"""
    return np.where(DC.mask(L, df)[None], ld(g)[:, None, None], LD(BETA))


def r_gp(x, ex, w):
    P, eP = SC.r_plaq(x, ex)
    s = np.sin(P)
    es = eP + 5 * U * mag(s)
    g = w * s
    return g, mag(w) * es + U * mag(g)


def r_force(x, ex, w):
    return SC.r_force_of(*r_gp(x, ex, w))


def _groups(x64):
    """the chains in groups that share action_bounds' mu = max(1, max |x| / pi): the last chain (never regularized) apart"""
    B = x64.shape[0]
    return [slice(0, B)] if B == 1 else [slice(0, B - 1), slice(B - 1, B)]


def r_sums(x, ex, df):
    """-> ((C, e), (Dsum, e), (Q, decided)) per chain"""
    B, L = x.shape[0], x.shape[-1]
    n, Ld = L * L, df[2]
    P, _ = SC.r_plaq(x, np.zeros(x.shape))
    _, eP = SC.r_plaq(x, ex)                                                   # with the 3 u (|a| + ..) of the device's own angle
    ePin = ex[:, 0] + ex[:, 1] + nb(ex[:, 0], 0, 1) + nb(ex[:, 1], 1, 0)
    cs = np.cos(P)
    m = DC.mask(L, df)[None]
    C, Dm = cs.reshape(B, -1).sum(axis=1), (cs * m).reshape(B, -1).sum(axis=1)
    x64 = f64(x)
    R = BC.sum_roundings(n, chain_threads(L))
    more = max(0, sum_count(L) - R)
    sc, scD = mag(cs).reshape(B, -1).sum(axis=1), (mag(cs) * m).reshape(B, -1).sum(axis=1)
    eC, mu = np.empty(B), np.empty(B)
    for sl in _groups(x64):
        c64 = f64(C[sl])
        eC[sl] = BC.action_bounds(x64[sl], -c64, c64 / n, 1.0)[0]
        mu[sl] = max(1.0, float(np.abs(x64[sl]).max()) / math.pi)
    eC = eC + U * (n + more * sc) + 2 * ex.reshape(B, -1).sum(axis=1)
    eD = U * (Ld * (9 * math.pi * mu + 4) + (R + 4) * scD) + U * (Ld + more * scD) + 2 * U * mag(Dm) + (ePin * m).reshape(B, -1).sum(axis=1)
    wr, _ = SC.r_wrap(P, eP)
    qs = wr.reshape(B, -1).sum(axis=1) / LD(TWO_PI)
    Q = np.rint(f64(qs)) + 0.0
    f_ = f64((P - LD(PI)) / LD(TWO_PI))
    dist = np.abs(f_ - np.round(f_)) * TWO_PI
    decided = (dist > MARGIN * eP).reshape(B, -1).all(axis=1) & (np.abs(f64(qs) - Q) < 1e-6)
    return (C, eC), (Dm, eD), (Q, decided)


def r_action(x, ex, g, df):
    """-> dict S, csum, dsum -> (value, bound); Q; decided"""
    B, L = x.shape[0], x.shape[-1]
    n = L * L
    (C, eC), (Dm, eD), (Q, dec) = r_sums(x, ex, df)
    x64 = f64(x)
    Sw = -(LD(BETA) * C)
    eSw = np.empty(B)
    for sl in _groups(x64):
        s64 = f64(Sw[sl])
        eSw[sl] = BC.action_bounds(x64[sl], s64, -s64 / (BETA * n), BETA)[0]
    P, _ = SC.r_plaq(x, np.zeros(x.shape))
    more = max(0, sum_count(L) - BC.sum_roundings(n, chain_threads(L)))
    eSw = eSw + BETA * U * (n + more * mag(np.cos(P)).reshape(B, -1).sum(axis=1)) + 2 * BETA * ex.reshape(B, -1).sum(axis=1)
    dg = LD(BETA) - ld(g)
    S = Sw + dg * Dm
    eS = eSw + mag(dg) * eD + 2 * U * mag(dg * Dm) + U * mag(S)
    return {'S': (S, eS), 'csum': (C, eC), 'dsum': (Dm, eD)}, Q, dec


def r_energy(x, ex, v, ev, g, df):
    """-> ((H, e), (C, e), (Dsum, e), Q, decided)"""
    (Hp, _, _), bH = SC.r_energy(x, ex, v, ev, BETA)
    Cp, Dp, (Q, dec) = r_sums(x, ex, df)
    dg = LD(BETA) - ld(g)
    H = Hp + dg * Dp[0]
    return (H, bH + mag(dg) * Dp[1] + 2 * U * mag(dg * Dp[0]) + U * mag(H)), Cp, Dp, Q, dec


def hold(pair):
    return pair[0], pair[1] * SLACK


@functools.lru_cache(maxsize=None)
def field_reference(c):
    """force and action of the case's start field -> dict(x, g, df, F, S, csum, dsum: held (value, bound) pairs; Q; decided per chain)"""
    x, _ = SC.inputs(c.seed, c.B, c.L)
    g, df = setup(c)
    X = SC.exact(x)
    A, Q, dec = r_action(*X, g, df)
    out = {'x': x, 'g': g, 'df': df, 'F': hold(r_force(*X, r_weights(c.L, g, df))), 'Q': Q, 'decided': dec}
    out.update({k: hold(v) for k, v in A.items()})
    return out


Traj = collections.namedtuple('Traj', 'seed redraws x v u g df H0 H1 dH xr csum dsum Q acc charges_decided accept_decided stages forced xp')


def _traj(c, seed):
    x, v = SC.inputs(seed, c.B, c.L)
    u = np.random.default_rng(seed + 17).uniform(size=c.B)
    g, df = setup(c)
    w = r_weights(c.L, g, df)
    z = np.zeros(x.shape)
    H0, C0, D0, Q0, dec = r_energy(ld(x), z, ld(v), z, g, df)
    b0, stages = IC.schedule(c.integrator, DT, c.nstep)
    X = SC.r_axpy(*SC.exact(x), *SC.exact(v), b0)
    Pm = SC.exact(v)
    at = X
    for kind, a, b in stages:
        F = r_force(at[0], at[1], w)
        if kind == 'shift':
            at = SC.r_axpy(*X, *F, -a)
        else:
            Pm = SC.r_kick(*Pm, *F, a)
            X = SC.r_axpy(*X, *Pm, b)
            at = X
    xr = SC.r_regularize(*X)
    H1, C1, D1, Q1, dec1 = r_energy(xr[0], xr[1], Pm[0], Pm[1], g, df)
    dH = H1[0] - H0[0]
    bdH = H0[1] + H1[1] + U * mag(dH)
    e = np.exp(-dH)
    d64 = f64(dH)
    forced = []
    if not (ld(u) < e).any():                                  # no chain of the draw accepted
        b = int(np.argmax(d64 < SC.DH_MAX))
        u[b] = SC.U_ACCEPT
        forced.append(('accept', b, 'U_ACCEPT'))
    if (ld(u) < e).all():                                      # no chain of the draw rejected
        can = d64 > 2 * bdH * SLACK + 4 * U
        if forced:
            can[forced[0][1]] = False
        if can.any():
            b = 1 if can[1] else int(np.argmax(can))
            u[b] = SC.U_REJECT
            forced.append(('reject', b, 'U_REJECT'))
        else:
            b = 1 + int(np.argmax(d64[1:]))
            u[b] = 2.0 * np.exp(-d64[b])
            forced.append(('reject', b, '2 exp(-dH)'))
    acc = ld(u) < e
    accept_decided = f64(np.abs(ld(u) - e)) > f64(e) * (2 * bdH * SLACK + 4 * U)
    sel = lambda a1, a0: (np.where(acc, a1[0], a0[0]), np.where(acc, a1[1], a0[1]))
    a4 = acc[:, None, None, None]
    xn = (np.where(a4, xr[0], ld(x)), np.where(a4, xr[1], 0.0))
    return Traj(seed, 0, x, v, u, g, df, hold(H0), hold(H1), hold((dH, bdH)), hold(xn), hold(sel(C1, C0)), hold(sel(D1, D0)),
                np.where(acc, Q1, Q0), f64(acc) > 0.5, dec & dec1, accept_decided, len(stages), tuple(forced), hold(xr))


@functools.lru_cache(maxsize=None)
def traj_reference(c):
    """The case's trajectory in long double with its bounds; the seed is redrawn (seed + 1000, at most 3 times) until the charge of
    both ends and the accept of every chain are decided on the reference's numbers.  x_new: the selected field -- the regularized end
    point with its bound where accepted, x with bound 0 where rejected (compared as an angle: a link next to the branch of regularize
    may come back 2 pi away)."""
    for k in range(4):
        T = _traj(c, c.seed + 1000 * k)
        if T.charges_decided.all() and T.accept_decided.all():
            return T._replace(redraws=k)
    raise AssertionError(f'{case_id(c)}: no draw with every charge and accept decided in 3 redraws')


# ---------------------------------------------------------------- the float64 twin, in the kernels' operation and summation order
MUTANTS = ('gp_one_pass', 'force_one_pass', 'translate_one_pass', 'energy_second_block', 'energy_sign', 'line_no_wrap', 'line_along_j',
           'ld_inclusive', 'neighbour_weight', 'selected_is_proposal', 'slice_g_from_zero', 'slice_shift_stride')


def t_on(L, df, mutant=None):
    """df_on of every site [L][L]: a = i - i0; a < 0 ? a + L : a; j == j0 && a < Ld.
      line_no_wrap   without the a + L branch (a negative a passes a < Ld)      line_along_j   the line runs along j from (i0, j0)
      ld_inclusive   a <= Ld"""
    i0, j0, Ld = df
    i, j = np.meshgrid(np.arange(L), np.arange(L), indexing='ij')
    if mutant == 'line_along_j':
        i, j, i0, j0 = j, i, j0, i0
    a = i - i0
    if mutant != 'line_no_wrap':
        a = np.where(a < 0, a + L, a)
    return (j == j0) & ((a <= Ld) if mutant == 'ld_inclusive' else (a < Ld))


def t_weights(L, g, df, mutant=None):
    return np.where(t_on(L, df, mutant)[None], np.asarray(g, dtype=np.float64)[:, None, None], BETA)


def _stale(new, old, mutant, name):
    """the first pass only of a grid-stride kernel: sites >= 64 x 256 of a chain keep what was there (old; NaN where nothing was)"""
    L = new.shape[-1]
    if mutant != name or L * L <= STRIDE_SITES:
        return new
    sh = new.shape
    out = new.reshape(sh[:-2] + (L * L,)).copy()
    out[..., STRIDE_SITES:] = np.nan if old is None else old.reshape(sh[:-2] + (L * L,))[..., STRIDE_SITES:]
    return out.reshape(sh)


def t_gp(x, g, df, mutant=None, before=None):
    """k_defect_gp (and the one-launch kernel's sp = wt sn).  gp_one_pass: sites >= 64 x 256 keep the plane of the stage before"""
    gp = t_weights(x.shape[-1], g, df, mutant) * np.sin(SC.t_plaq(x))
    return _stale(gp, before, mutant, 'gp_one_pass')


def t_force(x, g, df, mutant=None):
    """k_defect_force in launch_defect_force's slices of 65535 chains: three gP per site, each with the weight of its own site.
      neighbour_weight    the left and the upper gP take the centre site's weight
      force_one_pass      sites >= 64 x 256 are never written (NaN)
      slice_g_from_zero   the second slice reads g_b[0 ..]"""
    B, L = x.shape[0], x.shape[-1]
    g = np.array(g, dtype=np.float64)
    if mutant == 'slice_g_from_zero' and B > SLICE:
        g[SLICE:] = g[:B - SLICE]
    w = t_weights(L, g, df, mutant)
    sn = np.sin(SC.t_plaq(x))
    gc = w * sn
    if mutant == 'neighbour_weight':
        gl, gu = w * nb(sn, 0, -1), w * nb(sn, -1, 0)
    else:
        gl, gu = nb(gc, 0, -1), nb(gc, -1, 0)
    return _stale(np.stack([gc - gl, gu - gc], 1), None, mutant, 'force_one_pass')


def block_sums(terms, nt):
    """ft_block_sum of every row of terms [B][n] after the strided loop of nt threads (batch_kernel_cases.strided_partials and
    block_sum, over the chains at once)"""
    B, n = terms.shape
    out = np.empty(B)
    npass = -(-n // nt)
    nt = min(nt, 64 * -(-n // 64))           # the waves behind the last term hold 0.0 and add 0.0: left out, the same bits
    for b0 in range(0, B, 8192):
        t = terms[b0:b0 + 8192]
        a = np.zeros((t.shape[0], npass * nt))
        a[:, :n] = t
        a = a.reshape(-1, npass, nt)
        acc = np.zeros((t.shape[0], nt))
        for r in range(npass):
            acc = acc + a[:, r]
        w = BC.wave_sum(acc.reshape(t.shape[0], -1, 64))
        s = np.zeros(t.shape[0])
        for i in range(w.shape[1]):
            s = s + w[:, i]
        out[b0:b0 + 8192] = s
    return out


def t_sums(x, df, nt, mutant=None):
    """df_chain_sums + ft_block_sum (k_defect_sums, k_defect_action: nt = chain_threads(L); the one-launch kernel: nt = 1024, the
    same two angles per site) -> (C, Dsum, Q)"""
    B, L = x.shape[0], x.shape[-1]
    pc, pq = BC.plaq_angles(x)
    cs = np.cos(pc)
    C = block_sums(cs.reshape(B, -1), nt)
    Dm = block_sums(np.where(t_on(L, df, mutant)[None], cs, 0.0).reshape(B, -1), nt)
    q = block_sums(SC.t_wrap(pq).reshape(B, -1), nt)
    return C, Dm, np.rint(q / TWO_PI) + 0.0


def t_action(x, g, df, mutant=None):
    """k_defect_action -> (S_d, C, Dsum, Q).  energy_sign: (g - beta) Dsum"""
    C, Dm, Q = t_sums(x, df, chain_threads(x.shape[-1]), mutant)
    g = np.asarray(g, dtype=np.float64)
    dg = (g - BETA) if mutant == 'energy_sign' else (BETA - g)
    return (-BETA) * C + dg * Dm, C, Dm, Q


def t_energy(x, v, g, df, path, mutant=None):
    """-> (H, C, Dsum, Q).  path 2: k_defect_sums (S = (-beta) C), k_kinetic, the linear combination S + K / 2, k_defect_energy;
    path 1: the one-launch kernel's 1024-thread sums, K over v0^2 + v1^2 per site, (-beta) C + K / 2 and the defect's term behind it.
      energy_second_block   path 2: chains >= 256 (the second workgroup of k_defect_energy) keep H without the defect's term
      energy_sign           (g - beta) Dsum"""
    B, L = x.shape[0], x.shape[-1]
    g = np.asarray(g, dtype=np.float64)
    dg = (g - BETA) if mutant == 'energy_sign' else (BETA - g)
    if path == 1:
        C, Dm, Q = t_sums(x, df, ONE_LAUNCH_NT, mutant)
        K = block_sums((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]).reshape(B, -1), ONE_LAUNCH_NT)
        hp = (-BETA) * C + 0.5 * K
        return hp + dg * Dm, C, Dm, Q
    C, Dm, Q = t_sums(x, df, chain_threads(L), mutant)
    hp = (-BETA) * C + 0.5 * BC.kinetic_twin(v)
    h = hp + dg * Dm
    if mutant == 'energy_second_block':
        h[ENERGY_BLOCK:] = hp[ENERGY_BLOCK:]
    return h, C, Dm, Q


def t_trajectory(x, v, u, g, df, name, nstep, path, mutant=None):
    """defect_trajectory_call launch by launch (path 2) or k_defect_trajectory (path 1: the same MD arithmetic per site, its own
    sums) -> dict(H0, H1, dH, acc, x_new, csum, dsum, Q; x_prop: the regularized end point of every chain).
      selected_is_proposal   csum, dsum, Q of the proposed end point, whatever the accept"""
    b0, stages = IC.schedule(name, DT, nstep)
    H0, C0, D0, Q0 = t_energy(x, v, g, df, path, mutant)
    y = x + b0 * v
    p, at = v, y
    before = t_gp(x, g, df) if mutant == 'gp_one_pass' else None      # the plane as an evaluation at the start field left it
    for kind, a, b in stages:
        gp = t_gp(at, g, df, mutant, before)
        before = gp
        if kind == 'shift':
            at = SC.t_shift(gp, y, a)
        else:
            p, y = SC.t_kick(gp, p, y, a, b)
            at = y
    xr = SC.t_regularize(y)
    H1, C1, D1, Q1 = t_energy(xr, p, g, df, path, mutant)
    dH = H1 - H0
    with np.errstate(over='ignore', invalid='ignore'):
        acc = u < np.exp(-dH)
    keep = np.ones_like(acc) if mutant == 'selected_is_proposal' else acc
    return {'H0': H0, 'H1': H1, 'dH': dH, 'acc': acc, 'x_new': np.where(acc[:, None, None, None], xr, x), 'csum': np.where(keep, C1, C0),
            'dsum': np.where(keep, D1, D0), 'Q': np.where(keep, Q1, Q0), 'x_prop': xr}


def t_translate(x, rung, top, shift, mutant=None):
    """k_defect_translate in launch_defect_translate's slices of 65535 chains, index by index: a thread walks OUTPUT sites and reads
    the site that lands there; the shifts reduced as C reduces them (%, then + L where negative).
      translate_one_pass   sites >= 64 x 256 are never written (NaN)
      slice_shift_stride   the second slice reads its shifts from shift + b0 where shift + 2 b0 belongs"""
    B, L = x.shape[0], x.shape[-1]
    flat = np.asarray(shift, dtype=np.int64).reshape(-1)
    rung = np.asarray(rung)
    s = np.empty((B, 2), dtype=np.int64)
    for b0 in range(0, B, SLICE):
        nbk = min(SLICE, B - b0)
        base = b0 if (mutant == 'slice_shift_stride' and b0) else 2 * b0
        s[b0:b0 + nbk] = flat[base:base + 2 * nbk].reshape(nbk, 2)
    s = np.fmod(s, L)
    s = np.where(s < 0, s + L, s)
    s = np.where((rung == top)[:, None], s, 0)
    i = np.arange(L)
    fi = i[None, :] - s[:, 0:1]
    fj = i[None, :] - s[:, 1:2]
    fi, fj = np.where(fi < 0, fi + L, fi), np.where(fj < 0, fj + L, fj)
    out = x[np.arange(B)[:, None, None, None], np.arange(2)[None, :, None, None], fi[:, None, :, None], fj[:, None, None, :]]
    return _stale(out, None, mutant, 'translate_one_pass')


TranslateCase = collections.namedtuple('TranslateCase', 'x rung top shift')


@functools.lru_cache(maxsize=None)
def translate_case(sid):
    """L132: chain 0 on the top rung, chain 1 not; slice: every 7th chain on the top rung, and chains 65534 and 65535 (either side of
    the slice edge) with the non-zero shifts (1, 2) and (3, 1), chains 65533 and 65536 beside them on other rungs.  Shifts of the top
    rung's chains are drawn in [-2 L, 3 L): 0, L - 1, negative ones and ones >= L are planted where the draw might miss them."""
    B, L, kinds, paths = SHAPES[sid]
    c = next(k for k in ALL_CASES if k.shape == sid)
    x, _ = SC.inputs(c.seed, B, L)
    rng = np.random.default_rng(c.seed + 29)
    top = 3
    shift = rng.integers(-2 * L, 3 * L, size=(B, 2)).astype(np.int32)
    if sid == 'slice':
        rung = np.where(np.arange(B) % 7 == 0, top, np.arange(B) % 3).astype(np.int32)
        rung[SLICE - 2:SLICE + 2] = (1, top, top, 2)
        shift[SLICE - 1], shift[SLICE] = (1, 2), (3, 1)
        shift[0], shift[7], shift[14], shift[21] = (0, L - 1), (L - 1, 0), (-1, -L - 2), (L, 2 * L + 1)
    else:
        rung = np.array([top, 1], dtype=np.int32)
    rung.setflags(write=False); shift.setflags(write=False)
    return TranslateCase(x, rung, top, shift)


L132_SHIFTS = ((0, 131), (131, 0), (-5, -140), (132, 270), (7, 40))       # 0 and L - 1, negative and < -L, L and >= 2 L, generic


# ---------------------------------------------------------------- comparing
FIELD_OUTPUTS = ('F', 'S', 'csum', 'dsum')
TRAJ_OUTPUTS = ('x_new', 'H0', 'H1', 'dH', 'csum', 'dsum')


def field_fracs(got, ref):
    """got: dict F, S, csum, dsum, Q -> (dict output -> (fraction, where), Q equals the reference's on every chain)"""
    return {k: worst(got[k], ref[k]) for k in FIELD_OUTPUTS}, bool(np.array_equal(np.asarray(got['Q']), ref['Q']))


def traj_fracs(got, T):
    """-> (dict output -> (fraction, where), the accept flags and the charges are the reference's); x_prop (the twin's: the proposed
    end point of every chain, accepted or not, per link) where `got` has it"""
    f = {k: worst(got[k], getattr(T, 'xr' if k == 'x_new' else k), angle=k == 'x_new') for k in TRAJ_OUTPUTS}
    if 'x_prop' in got:
        f['x_prop'] = worst(got['x_prop'], T.xp, angle=True)
    ok = bool(np.array_equal(np.asarray(got['acc']) > 0.5, T.acc)) and bool(np.array_equal(np.asarray(got['Q']), T.Q))
    return f, ok


def field_twin(c, mutant=None):
    ref = field_reference(c)
    S, C, Dm, Q = t_action(ref['x'], ref['g'], ref['df'], mutant)
    return {'F': t_force(ref['x'], ref['g'], ref['df'], mutant), 'S': S, 'csum': C, 'dsum': Dm, 'Q': Q}


def traj_twin(c, path, mutant=None):
    T = traj_reference(c)
    return t_trajectory(T.x, T.v, T.u, T.g, T.df, c.integrator, c.nstep, path, mutant)
