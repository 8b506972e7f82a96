"""GPU tests of the plain Wilson stencil and trajectory kernels (fthmc_amd/csrc/wilson.hip: k_force<0|1|2> and their per-chain-beta
instances, k_leap_rows, k_gp_rows, k_kick_rows, k_shift_rows, k_kick_from_gp, k_shift_from_gp, k_hmc_trajectory,
k_hmc_trajectory_sched, k_metropolis, k_plaq, k_wrap, k_axpy, k_axpy_copy), each held PER SITE on every lattice class the code treats
differently: slow-wrap tiles (L = 4, 12, 16), ragged fast-wrap tiles (20, 36), exact tiles (48), just past a row-strip size (68), past
one pass of the grid-stride kernels (132), row strips of one and two segments (64, 128), the one-launch trajectories with partly
filled site slots (4, 8, 36, 60, 64).

References, bounds and inputs: tests/stencil_cases.py (numpy longdouble at the fp64 inputs; every bound a per-site array derived from
the inputs' magnitudes; links pinned at +-pi, one chain of links ~ 30, momenta x 3, per-chain beta distinct per chain);
tests/test_stencils.py holds the float64 twin to the same bounds on the CPU and shows that each named mutant leaves them.  The C ABI
is called directly: every output lands in a slice of a NaN-filled buffer whose guard words must keep their bits, every call runs
twice and gives the same bits, every test leaves FTHMC_LEAP_ROWS, the variant and the small-path switch as it found them.  Each test
prints its worst error as a fraction of the bound under the kernel family it belongs to (WORST <family> <value>)."""
import os

import numpy as np
import pytest
import torch

import stencil_cases as C
from gpu_support import D, Poisoned, lib, module_defaults, ops, switches

pytestmark = pytest.mark.gpu
_defaults = module_defaults()

CODES = C.IC.CODES


@pytest.fixture(autouse=True)
def _switches_left_as_found():
    before = (os.environ.get('FTHMC_LEAP_ROWS'), ops.get_variant(), ops.get_small_path())
    yield
    assert (os.environ.get('FTHMC_LEAP_ROWS'), ops.get_variant(), ops.get_small_path()) == before


def note(family, value):
    print(f'WORST {family} {value:.4f}')
    assert value <= 1.0, (family, value)


def twice(call, sizes):
    """call(*outputs) with fresh NaN-filled outputs of `sizes` doubles, twice: the same bits, the guards intact -> numpy arrays"""
    runs = []
    for _ in range(2):
        outs = [Poisoned(n) for n in sizes]
        assert call(*[o.t for o in outs]) == 0
        torch.cuda.synchronize()
        assert all(o.intact() for o in outs)
        runs.append([o.t.cpu().numpy() for o in outs])
    for a, b in zip(*runs):
        assert np.array_equal(C.bits(a), C.bits(b))
    return runs[0]


def ws_of(x, c):
    return ops._ws(x, c.B, c.L, 0)


# ---------------------------------------------------------------- the device's answers
def dev_force(c, x):
    return twice(lambda F: lib.fthmc_wilson_force(ops._p(x), c.B, c.L, c.beta, ops._p(F), ops._stream(x)), [x.numel()])[0].reshape(x.shape)


def dev_plaq(c, x):
    return twice(lambda P: lib.fthmc_plaquettes(ops._p(x), ops._p(P), c.B, c.L, ops._stream(x)), [x.numel() // 2])[0].reshape(c.B, c.L, c.L)


def dev_ft_force0(c, x):
    ws, nb = ws_of(x, c)
    return twice(lambda F: lib.fthmc_ft_force_v(ops._p(x), None, None, 0, c.B, c.L, 0, c.beta, ops._p(F), ws, nb, ops._stream(x), 0),
                 [x.numel()])[0].reshape(x.shape)


def dev_md(c, x, p, name, nstep):
    """fthmc_leapfrog for the leapfrog, fthmc_md for the schedules -> (x', p')"""
    ws, nb = ws_of(x, c)
    if name == 'leapfrog':
        call = lambda xo, po: lib.fthmc_leapfrog(ops._p(x), ops._p(p), c.B, c.L, c.beta, c.dt, nstep, ops._p(xo), ops._p(po), ws, nb, ops._stream(x))
    else:
        call = lambda xo, po: lib.fthmc_md(ops._p(x), ops._p(p), c.B, c.L, c.beta, c.dt, nstep, CODES[name], ops._p(xo), ops._p(po), ws, nb,
                                           ops._stream(x))
    xo, po = twice(call, [x.numel()] * 2)
    return xo.reshape(x.shape), po.reshape(x.shape)


def dev_traj(c, T, nstep):
    """fthmc_hmc_trajectory (leapfrog), fthmc_hmc_trajectory_int (schedules) or, for a per-chain beta, fthmc_hmc_trajectory_pb"""
    x, v, u = D(T.x), D(T.v), D(T.u)
    ws, nb = ws_of(x, c)
    p, s = ops._p, ops._stream(x)
    if isinstance(c.beta, tuple):
        bb = D(c.beta)
        call = lambda xn, dH, acc, H0, H1: lib.fthmc_hmc_trajectory_pb(p(x), p(v), p(u), c.B, c.L, p(bb), c.dt, nstep, CODES[c.integrator], p(xn),
                                                                      p(dH), p(acc), p(H0), p(H1), ws, nb, s)
    elif c.integrator == 'leapfrog':
        call = lambda xn, dH, acc, H0, H1: lib.fthmc_hmc_trajectory(p(x), p(v), p(u), c.B, c.L, c.beta, c.dt, nstep, p(xn), p(dH), p(acc), p(H0),
                                                                   p(H1), ws, nb, s)
    else:
        call = lambda xn, dH, acc, H0, H1: lib.fthmc_hmc_trajectory_int(p(x), p(v), p(u), c.B, c.L, c.beta, c.dt, nstep, CODES[c.integrator], p(xn),
                                                                       p(dH), p(acc), p(H0), p(H1), ws, nb, s)
    xn, dH, acc, H0, H1 = twice(call, [x.numel()] + [c.B] * 4)
    assert np.array_equal(C.bits(x.cpu().numpy()), C.bits(T.x))                      # the inputs are only read
    return {'x_new': xn.reshape(T.x.shape), 'dH': dH, 'acc': acc, 'H0': H0, 'H1': H1}


def both_settings(L, run):
    """run() with the row strips on (as the library starts) and, at L % 64 == 0, with FTHMC_LEAP_ROWS = 0 as well
    -> [(setting, result), ...]"""
    out = [(1, run())]
    if L % 64 == 0:
        with switches(leap_rows=False):
            out.append((0, run()))
    return out


def same_bits(a, b):
    return all(np.array_equal(C.bits(s), C.bits(t)) for s, t in zip(a, b))


def case_of(cases, L, name='leapfrog'):
    return next(c for c in cases if c.L == L and c.integrator == name)


# ---------------------------------------------------------------- force and plaquettes
@pytest.mark.parametrize('L', C.STENCIL_L)
def test_force_and_plaquettes_per_site(L):
    c = case_of(C.STENCIL_CASES, L)
    ref = C.stencil_reference(c)
    x = D(C.inputs(c.seed, c.B, c.L)[0])
    # k_force<0> and k_plaq serve every L whatever FTHMC_LEAP_ROWS says: at L = 64, 128 the second setting runs the same two
    # kernels again and must give the same bits
    res = both_settings(L, lambda: (dev_force(c, x), dev_plaq(c, x)))
    for setting, (F, P) in res:
        note('tile', C.frac(F, ref['force']))
        note('grid-stride', C.frac(P, ref['plaq']))
    assert len(res) == 1 or same_bits(res[0][1], res[1][1])


@pytest.mark.parametrize('L', (20, 64))
def test_ft_force_with_zero_layers_is_the_wilson_force(L):
    """the Fout branch of k_kick_from_gp / k_kick_rows behind the seed kernels"""
    c = case_of(C.STENCIL_CASES, L)
    ref = C.stencil_reference(c)
    x = D(C.inputs(c.seed, c.B, c.L)[0])
    res = both_settings(L, lambda: dev_ft_force0(c, x))
    for setting, F in res:
        note('row strip' if setting and L % 64 == 0 else 'grid-stride', C.frac(F, ref['force']))
    assert len(res) == 1 or same_bits([res[0][1]], [res[1][1]])


# ---------------------------------------------------------------- MD
@pytest.mark.parametrize('L', C.STENCIL_L)
def test_leapfrog_per_site(L):
    c = case_of(C.STENCIL_CASES, L)
    x, p = (D(t) for t in C.inputs(c.seed, c.B, c.L))
    for n in C.LEAP_NSTEP:
        ref = C.md_reference(c, n)
        res = both_settings(L, lambda: dev_md(c, x, p, 'leapfrog', n))
        for setting, (xo, po) in res:
            fam = 'row strip' if setting and L % 64 == 0 else 'tile'
            print(f'L={L} nstep {n} rows {setting}: x {C.frac(xo, ref["x"]):.3f} p {C.frac(po, ref["p"]):.3f} of the bound')
            note(fam, max(C.frac(xo, ref['x']), C.frac(po, ref['p'])))
        assert len(res) == 1 or same_bits(res[0][1], res[1][1]), n                # k_leap_rows = k_force<1>, bit for bit


@pytest.mark.parametrize('name', C.INTEGRATORS[1:])
@pytest.mark.parametrize('L', C.MD_L)
def test_schedule_md_per_site(L, name):
    """fthmc_md: k_force<2> / k_gp_rows, k_kick_from_gp / k_kick_rows, k_shift_from_gp / k_shift_rows, k_axpy_copy"""
    c = case_of(C.MD_CASES, L, name)
    x, p = (D(t) for t in C.inputs(c.seed, c.B, c.L))
    for n in C.MD_NSTEP:
        ref = C.md_reference(c, n)
        res = both_settings(L, lambda: dev_md(c, x, p, name, n))
        for setting, (xo, po) in res:
            fam = 'row strip' if setting and L % 64 == 0 else 'grid-stride'
            print(f'L={L} {name} nstep {n} rows {setting}: x {C.frac(xo, ref["x"]):.3f} p {C.frac(po, ref["p"]):.3f} of the bound')
            note(fam, max(C.frac(xo, ref['x']), C.frac(po, ref['p'])))
        assert len(res) == 1 or same_bits(res[0][1], res[1][1]), n                # the row-strip kernels = the grid-stride ones


# ---------------------------------------------------------------- trajectories
def check_traj(c, n, family):
    T = C.traj_reference(c, n)
    got = dev_traj(c, T, n)
    f, ok = C.traj_fracs(got, T)
    print(f'{C.case_id(c)} nstep {n} (draw {T.redraws}{", u above one" if T.above_one else ""}): H0 {got["H0"].tolist()} H1 {got["H1"].tolist()} '
          f'dH {got["dH"].tolist()} acc {got["acc"].tolist()}; of the bounds: ' + ' '.join(f'{k} {v:.3f}' for k, v in f.items()))
    assert ok, (got['acc'], T.accept)
    note(family, max(f['H0'], f['H1'], f['dH']))
    note(family if family == 'one-launch' else 'metropolis', f['x_new'])


@pytest.mark.parametrize('name', C.INTEGRATORS)
@pytest.mark.parametrize('L', C.ONE_LAUNCH_L)
def test_one_launch_trajectory(L, name):
    """k_hmc_trajectory / k_hmc_trajectory_sched<false>"""
    for n in C.TRAJ_NSTEP:
        check_traj(case_of(C.TRAJ_CASES, L, name), n, 'one-launch')


@pytest.mark.parametrize('name', C.INTEGRATORS)
@pytest.mark.parametrize('L', C.MULTI_LAUNCH_L)
def test_multi_launch_trajectory(L, name):
    """the step kernels, k_wrap and k_metropolis; L = 8, 36 with the VALU variant, which has no one-launch kernel"""
    fam = 'tile' if name == 'leapfrog' else 'grid-stride'
    with switches(variant=0 if L <= 64 else 1):
        for n in C.TRAJ_NSTEP:
            check_traj(case_of(C.TRAJ_CASES, L, name), n, fam)


@pytest.mark.parametrize('name', C.INTEGRATORS)
@pytest.mark.parametrize('L', C.PB_L)
def test_per_chain_beta_trajectory(L, name):
    """fthmc_hmc_trajectory_pb with a beta distinct per chain: the one-launch kernel (20), the tile and grid-stride kernels (68), the
    row strips (128)"""
    fam = 'one-launch' if L <= 64 else ('row strip' if L % 64 == 0 else ('tile' if name == 'leapfrog' else 'grid-stride'))
    for n in C.TRAJ_NSTEP:
        check_traj(case_of(C.PB_CASES, L, name), n, fam)


# ---------------------------------------------------------------- k_wrap
@pytest.mark.parametrize('L', (4, 132))
def test_wrap_and_regularize_per_link(L):
    """one workgroup (L = 4) and, with the L = 132 field eight times over, past the 2048 x 256 threads of the grid (557568 links)"""
    c = case_of(C.STENCIL_CASES, L)
    ref = C.stencil_reference(c)
    reps = 8 if L == 132 else 1
    x64 = np.tile(C.inputs(c.seed, c.B, c.L)[0].reshape(-1), reps)
    assert reps == 1 or x64.size > 2048 * 256
    x = D(x64)
    for key, fn in (('wrap', lib.fthmc_wrap), ('regularize', lib.fthmc_regularize)):
        out = twice(lambda o: fn(ops._p(x), ops._p(o), x.numel(), ops._stream(x)), [x.numel()])[0]
        val, bound = ref[key]
        note('grid-stride', C.frac(out, (np.tile(val.reshape(-1), reps), np.tile(bound.reshape(-1), reps))))
