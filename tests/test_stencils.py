"""CPU checks behind tests/test_stencils_gpu.py: the float64 twin of the plain Wilson stencil and trajectory kernels
(tests/stencil_cases.py) stays inside the derived per-site bounds against the longdouble reference on every case -- the proof that
the inputs can meet the bounds without the device --, the reference itself is held to mpmath at 50 digits on the three smallest
lattices, every named mutant of the twin leaves a bound (or breaks an exact assertion) on at least one case, and the integer
arithmetic k_force restates on the host is what it stands for."""
import math

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401

import stencil_cases as C

LD = C.LD


def worst(fs):
    fs = list(fs)
    return math.nan if any(f != f for f in fs) else max(fs)


def test_reference_is_extended_precision():
    """the references need a wider significand than fp64"""
    assert np.finfo(np.longdouble).nmant == 63


# ---------------------------------------------------------------- one evaluation of the twin per (kind, case, nstep)
def run_stencil(c, n, mutant=None):
    ref, tw = C.stencil_reference(c), C.stencil_twin(c, mutant)
    return {k: C.frac(tw[k], ref[k]) for k in ref}, C.window_in_range(c.L, once=mutant == 'single_wrap_L4')


def run_leapfrog(c, n, mutant=None):
    x, p = C.inputs(c.seed, c.B, c.L)
    ref = C.md_reference(c, n)
    xo, po = C.t_leapfrog(x, p, c.beta, c.dt, n, mutant)
    return {'x': C.frac(xo, ref['x']), 'p': C.frac(po, ref['p'])}, True


def run_md(c, n, mutant=None):
    x, p = C.inputs(c.seed, c.B, c.L)
    ref = C.md_reference(c, n)
    xo, po = C.t_md(x, p, c.beta, c.integrator, c.dt, n, mutant)
    return {'x': C.frac(xo, ref['x']), 'p': C.frac(po, ref['p'])}, True


def run_traj(c, n, mutant=None):
    T = C.traj_reference(c, n)
    return C.traj_fracs(C.t_trajectory(T.x, T.v, T.u, c.beta, c.integrator, c.dt, n, mutant), T)


RUNS = ([('stencil', run_stencil, c, 0) for c in C.STENCIL_CASES] +
        [('leapfrog', run_leapfrog, c, n) for c in C.STENCIL_CASES for n in C.LEAP_NSTEP] +
        [('md', run_md, c, n) for c in C.MD_CASES for n in C.MD_NSTEP] +
        [('trajectory', run_traj, c, n) for c in C.TRAJ_CASES + C.PB_CASES for n in C.TRAJ_NSTEP])


def run_id(r):
    return f'{r[0]}-{C.case_id(r[2])}-nstep{r[3]}'


@pytest.mark.parametrize('run', RUNS, ids=run_id)
def test_twin_stays_inside_the_bounds(run):
    kind, fn, c, n = run
    f, ok = fn(c, n)
    w = worst(f.values())
    print(f'TWIN {run_id(run)}: worst error {w:.4f} of the bound  ' + ' '.join(f'{k} {v:.3f}' for k, v in f.items()))
    assert ok and w <= 1.0, f


def test_conditions_on_the_references():
    """what the GPU tests rely on, on the references alone: no link of an input or of an end point nearer than 1e-12 to the branch
    of regularize / wrap (the bounds there are ~1e-14), one accepted and one surely rejected chain per trajectory; the redraws"""
    for c in C.STENCIL_CASES:
        assert C.branch_margin(C.inputs(c.seed, c.B, c.L)[0]) > 1e-12, c.id
    redrawn, above = [], []
    for c in C.TRAJ_CASES + C.PB_CASES:
        for n in C.TRAJ_NSTEP:
            T = C.traj_reference(c, n)
            assert T.margin > 1e-12 and T.accept.any() and T.rejected.any(), (C.case_id(c), n)
            d, b = C.f64(T.dH[0]), T.dH[1]
            assert np.all(d[T.accept] < C.DH_MAX) and np.all(T.u[T.accept] == 0.0)
            if T.above_one:
                assert np.all(d < -2 * b) and np.all(T.u[T.rejected] == 2.0 * np.exp(-d[T.rejected]))
                above.append((C.case_id(c), n))
            else:
                assert np.all(d[T.rejected] > 2 * b[T.rejected]) and np.all(T.u[T.rejected] == C.U_REJECT)
                if T.redraws:
                    redrawn.append((C.case_id(c), n, T.redraws))
    print('REDRAWN trajectory cases (id, nstep, redraws):', redrawn)
    print('REJECTED BY u = 2 exp(-dH) (every chain of four draws loses energy):', above)


@pytest.mark.parametrize('L', C.STENCIL_L)
def test_tile_twin_equals_the_roll_twin(L):
    """k_force restated tile by tile with its window indices = the whole-lattice twin, bit for bit (every site written once)"""
    c = C.STENCIL_CASES[C.STENCIL_L.index(L)]
    x, _ = C.inputs(c.seed, c.B, c.L)
    assert np.array_equal(C.bits(C.t_force_tiles(x, c.beta)), C.bits(C.t_force(x, c.beta)))


@pytest.mark.parametrize('lo,hi', [(0.0, 0.05), (0.0, 0.5), (-0.5, 0.0), (-3.1, 3.1), (C.PI - 1e-6, C.PI + 1e-6), (27.0, 33.0), (-33.0, -27.0)])
def test_regularize_and_wrap_twins_on_dense_samples(lo, hi):
    """the float64 twins of ft_regularize / ft_wrap inside their bounds on 400000 links of every interval where a rounding of the
    two changes its size: just above 0 (f_ in (-1/2, 0): f_ + 1 rounds), around the branch, the never-regularized range"""
    x = np.random.default_rng(int(1000 * (hi + 40))).uniform(lo, hi, 400000)
    x = x[np.abs(np.abs(x) - C.PI) > 1e-12]                          # the branch itself: see branch_margin
    fr = C.frac(C.t_regularize(x), C.hold(C.r_regularize(*C.exact(x))))
    fw = C.frac(C.t_wrap(x), C.hold(C.r_wrap(*C.exact(x))))
    print(f'DENSE ({lo}, {hi}): regularize {fr:.4f} wrap {fw:.4f} of the bound')
    assert fr <= 1.0 and fw <= 1.0


# ---------------------------------------------------------------- the reference against mpmath
@pytest.mark.parametrize('L', (4, 12, 16))
def test_reference_against_mpmath(L):
    """the longdouble reference against the same operations at 50 digits: inside the 2^-8 of the bound that SLACK sets aside"""
    import mpmath
    mp = mpmath.mp.clone()
    mp.dps = 50
    c = C.STENCIL_CASES[C.STENCIL_L.index(L)]
    x64, p64 = C.inputs(c.seed, c.B, c.L)
    ref = C.stencil_reference(c)

    def arr(a):
        return np.array([mp.mpf(float(v)) for v in np.ravel(a)], dtype=object).reshape(np.shape(a))
    msin, mcos, mfloor = (np.frompyfunc(f, 1, 1) for f in (mp.sin, mp.cos, mp.floor))
    x, p = arr(x64), arr(p64)
    beta, dt, a, pi = mp.mpf(c.beta), mp.mpf(c.dt), mp.mpf(c.a), mp.mpf(C.PI)

    def plaq(y):
        return y[:, 0] - y[:, 1] - C.nb(y[:, 0], 0, 1) + C.nb(y[:, 1], 1, 0)

    def force(y):
        g = beta * msin(plaq(y))
        return g, np.stack([g - C.nb(g, 0, -1), C.nb(g, -1, 0) - g], 1)
    g, F = force(x)
    y = x + a * p
    v1 = p - dt * F
    f_ = (x - pi) / (2 * pi)
    r = x + pi
    out = {'plaq': plaq(x), 'gp': g, 'force': F, 'step_x': y, 'step_p': p - dt * force(y)[1], 'kick_v': v1, 'kick_x': x + a * v1,
           'shift': x - mp.mpf(c.dt * c.dt / 24.0) * F, 'regularize': 2 * pi * (f_ - mfloor(f_) - mp.mpf(0.5)),
           'wrap': r - 2 * pi * mfloor(r / (2 * pi)) - pi}
    assert sorted(out) == sorted(ref)
    share = (C.SLACK - 1.0) / C.SLACK
    for k, (val, bound) in ref.items():
        m = np.array([LD(mp.nstr(v, 40)) for v in out[k].ravel()], dtype=LD).reshape(val.shape)
        f = C.BC.frac(C.f64(np.abs(val - m)), bound * share)
        print(f'MPMATH L={L} {k}: the reference is {f:.4f} of its share of the bound from mpmath')
        assert f <= 1.0, k
    # the energies
    (H, S, K), bH = C.r_energy(C.ld(x64), np.zeros(x64.shape), C.ld(p64), np.zeros(x64.shape), c.beta)
    for b in range(c.B):
        Hm = -beta * sum(mcos(plaq(x)[b]).ravel()) + sum((p[b] * p[b]).ravel()) / 2
        assert abs(float(H[b] - LD(mp.nstr(Hm, 40)))) <= bH[b] * (C.SLACK - 1.0), b


# ---------------------------------------------------------------- the mutants
def test_every_mutant_leaves_a_bound():
    caught = {}
    for m in C.MUTANTS:
        for run in RUNS:
            kind, fn, c, n = run
            f, ok = fn(c, n, m)
            w = worst(f.values())
            if not ok or not w <= 1.0:
                caught[m] = run_id(run)
                print(f'MUTANT {m}: caught first by {run_id(run)} ({w:.3g} of the bound, exact assertions {"hold" if ok else "fail"})')
                break
    assert sorted(caught) == sorted(C.MUTANTS), sorted(set(C.MUTANTS) - set(caught))


# ---------------------------------------------------------------- host arithmetic the kernels restate
def test_reciprocal_multiply_divisions_of_k_force():
    """(u * ((1 << 20) + W - 1) / W) >> 20 = u / W for the window widths 18, 17 below the window sizes 306, 306 and 289; the operands
    of the 24-bit multiply fit 24 bits and the product 32"""
    for W, n in ((18, 17 * 18), (17, 18 * 17), (17, 17 * 17)):
        m = ((1 << 20) + W - 1) // W
        assert m < 1 << 24 and n < 1 << 24 and (n - 1) * m < 1 << 32
        for u in range(n):
            assert (u * m) >> 20 == u // W, (W, u)


def test_once_wrapped_window_index_is_the_remainder():
    """min(w, w - L, w + L) as unsigned = w mod L for every tile origin and window offset of every L % 4 == 0, 18 <= L <= 256"""
    off = np.arange(C.TS + 2)
    for L in range(20, 257, 4):
        for o in range(0, L, C.TS):
            w = o - 1 + off
            assert np.array_equal(C.wrap_once(w, L), w % L), (L, o)
    assert C.TS + 2 == 18 and not np.array_equal(C.wrap_once(np.arange(-1, 17), 4), np.arange(-1, 17) % 4)
