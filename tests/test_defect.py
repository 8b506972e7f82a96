"""CPU-only tests of boundary-condition tempering (csrc/defect.hip): the C ABI declares and exports the five entry points
and the wrappers, the driver and the `fthmc` aliases exist, the refusals refuse and the workspace rule holds; the numpy twin of
tests/defect_cases.py has a force that is the gradient of its own action, agrees with itself between float64 and long double (the
rounding figures the GPU tests' 8x rule rests on) and leaves no chain out on the committed inputs; exact_defect_plaquette against its
limits, a brute-force sum and a sampled run's values; the twin as a sampler against the exact <Q^2>; the entry points' host side as a
stand-alone program under AddressSanitizer + UBSan."""
import inspect
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

import defect_cases as DC

LD = np.longdouble
ENTRY_POINTS = ('fthmc_defect_ws_bytes', 'fthmc_defect_trajectory', 'fthmc_defect_force', 'fthmc_defect_action', 'fthmc_defect_translate')


def test_header_library_wrappers_driver_and_alias_carry_the_new_entry_points():
    import ctypes
    from fthmc_amd import _lib, ops
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'fthmc_hip.h')).read()
    declared = set(re.findall(r'\b(fthmc_[a-z0-9_]+)\s*\(', header))
    for name in ENTRY_POINTS:
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    section = header[header.index('---- Boundary-condition tempering'):header.index('---- training')]
    assert section.count('No reference counterpart.') == 4               # one per declaration (force and action share theirs)
    sig = _lib.SIGNATURES['fthmc_defect_trajectory']
    assert len(sig) == 25 and sig[5] is ctypes.c_double and sig[6] is ctypes.c_void_p and sig[7:10] == [ctypes.c_int] * 3
    assert sig[10] is ctypes.c_double and sig[11:14] == [ctypes.c_int] * 3 and sig[23] is ctypes.c_size_t
    assert len(_lib.SIGNATURES['fthmc_defect_force']) == 10 and len(_lib.SIGNATURES['fthmc_defect_action']) == 13
    assert len(_lib.SIGNATURES['fthmc_defect_translate']) == 8 and lib.fthmc_defect_ws_bytes.restype is ctypes.c_size_t
    p = inspect.signature(ops.defect_trajectory).parameters
    assert list(p) == ['x', 'v', 'u', 'beta', 'g_b', 'defect', 'dt', 'nstep', 'integrator', 'path', 'out']
    assert (p['integrator'].default, p['path'].default, p['out'].default) == ('leapfrog', 0, None)
    assert list(inspect.signature(ops.defect_force).parameters) == ['x', 'beta', 'g_b', 'defect']
    assert list(inspect.signature(ops.defect_action).parameters) == ['x', 'beta', 'g_b', 'defect', 'out']
    assert list(inspect.signature(ops.defect_translate).parameters) == ['x', 'rung', 'top', 'shift', 'out']
    import fthmc
    import fthmc_amd
    import fthmc.defect as d1
    import fthmc_amd.defect as d2
    import fthmc.utils.observables as o1
    assert d1 is d2 and fthmc.run_ptbc is d2.run_ptbc is fthmc_amd.run_ptbc
    p = inspect.signature(d2.run_ptbc).parameters
    assert list(p) == ['param', 'cs', 'n_ladders', 'ntraj', 'defect', 'swap_every', 'translate', 'integrator', 'seed', 'x', 'captured', 'shard']
    assert (p['defect'].default, p['swap_every'].default, p['translate'].default, p['integrator'].default, p['seed'].default,
            p['x'].default, p['captured'].default, p['shard'].default) == (None, 1, True, 'leapfrog', None, None, True, None)
    assert d2.default_defect(16) == (0, 0, 4) and d2.default_defect(4) == (0, 0, 1)
    from fthmc_amd import tempering
    seeds = {d2.shift_seed(7), tempering.swap_seed(7), tempering.init_seed(7), 7}
    assert len(seeds) == 4                                                # a key domain of its own
    p = inspect.signature(o1.exact_defect_plaquette).parameters
    assert list(p) == ['beta', 'L', 'c', 'Ld', 'on_defect', 'nmax'] and (p['on_defect'].default, p['nmax'].default) == (True, 40)
    # no torch operator for this feature: the operator table stays what tests/test_torch_boundary.py pins
    import fthmc_amd.torch_ops as TO
    assert not [n for n in TO.__all__ if 'defect' in n]


def test_refusals_refuse_and_the_workspace_rule():
    """the argument checks of the C entry points come before anything touches the device: stand-in addresses are never read"""
    from fthmc_amd import _lib, ops
    from fthmc_amd._lib import FthmcError
    lib = _lib.load()
    X, V, U, G, O, W, F, R, S = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000, 0x70000000, 0x80000000, 0x90000000
    ARG, UNS, WS = -1, -2, -4
    inf, nan = float('inf'), float('nan')

    def traj(x=X, v=V, u=U, B=4, L=8, beta=2.0, g=G, i0=1, j0=2, Ld=3, nstep=2, integ=0, path=1, out=O, ws=None, nbytes=0):
        return lib.fthmc_defect_trajectory(x, v, u, B, L, beta, g, i0, j0, Ld, 0.1, nstep, integ, path, out, None, None, None, None,
                                           None, None, None, ws, nbytes, None)

    def frc(x=X, B=4, L=8, beta=2.0, g=G, i0=1, j0=2, Ld=3, out=F):
        return lib.fthmc_defect_force(x, B, L, beta, g, i0, j0, Ld, out, None)

    def act(x=X, B=4, L=8, beta=2.0, g=G, i0=1, j0=2, Ld=3):
        return lib.fthmc_defect_action(x, B, L, beta, g, i0, j0, Ld, O, None, None, None, None)

    def trn(x=X, B=4, L=8, rung=R, top=3, shift=S, out=O):
        return lib.fthmc_defect_translate(x, B, L, rung, top, shift, out, None)
    for f in (traj, frc, act, trn):
        assert f(x=None) == ARG
        for B in (0, -1, 4194304):
            assert f(B=B) == ARG
        for L in (0, 2, 6, 10, -8, 32768):
            assert f(L=L) == ARG
    for f in (traj, frc, act):
        assert f(g=None) == ARG
        for Ld in (-1, 9, 2 ** 31 - 1):
            assert f(Ld=Ld) == ARG
        for i in (-1, 8, 2 ** 31 - 1):
            assert f(i0=i) == ARG and f(j0=i) == ARG
        for beta in (inf, -inf, nan):
            assert f(beta=beta) == ARG
    assert traj(v=None) == ARG and traj(u=None) == ARG and traj(out=None) == ARG and frc(out=None) == ARG
    assert trn(out=None) == ARG and trn(out=X) == ARG and trn(rung=None) == ARG and trn(shift=None) == ARG
    for n in (0, -1):
        assert traj(nstep=n) == ARG
    for p in (-1, 3, 255):
        assert traj(path=p) == ARG
    assert traj(L=68, path=1) == ARG and traj(out=X, path=1) == ARG       # what the one-launch path does not serve
    assert traj(integ=3) == UNS and traj(integ=-1) == UNS and traj(integ=3, nstep=0) == ARG and traj(integ=3, Ld=9) == ARG   # the arguments come first
    # (every call here is refused before a launch: the legal edges -- Ld = 0 and L, B = 1 and 65535, every path -- are walked by
    # tests/hip/defect_walk.cpp against the build that launches nothing)
    # the workspace: none for the one-launch path; the sequenced path's otherwise (path 0 may take it)
    wsb = lib.fthmc_defect_ws_bytes
    assert wsb(4, 8, 1) == 0 and wsb(4, 128, 1) == 0
    assert wsb(4, 8, 0) == wsb(4, 8, 2) > lib.fthmc_ws_bytes(None, 4, 8, 0) and wsb(4, 8, 2) % 256 == 0
    assert wsb(0, 8, 2) == 0 and wsb(2, 6, 2) == 0 and wsb(2, 8, 3) == 0 and wsb(2, 8, -1) == 0
    need = wsb(4, 8, 2)
    assert traj(path=2) == WS and traj(path=2, ws=W, nbytes=need - 1) == WS and traj(path=2, ws=None, nbytes=need) == WS
    assert traj(path=0, out=X) == WS and traj(path=0, L=68) == WS         # path 0 where the one-launch kernel does not serve
    assert traj(path=2, x=None) == ARG and traj(path=2, integ=7) == UNS   # ARG, then UNSUPPORTED, then the workspace
    # the sequenced path serves B <= 65535 (its kernels put the chain on grid y): unsupported beyond, and no workspace size
    assert traj(B=65536, path=2) == UNS and traj(B=65536, path=0, out=X) == UNS and traj(B=65536, path=2, nstep=0) == ARG
    assert wsb(65535, 8, 2) > 0 and wsb(65536, 8, 2) == 0 and wsb(65536, 8, 0) == 0
    x = torch.zeros(2, 2, 8, 8, dtype=torch.float64)
    with pytest.raises(FthmcError):
        ops.defect_force(x, 2.0, torch.zeros(2, dtype=torch.float64), (0, 0, 2))     # CPU tensors: there is no CPU fallback
    with pytest.raises(FthmcError):
        ops.defect_translate(x, torch.zeros(2, dtype=torch.int32), 1, torch.zeros(2, 2, dtype=torch.int32))


# ---------------------------------------------------------------- the twin
@pytest.mark.parametrize('L,amp,beta,dk', [(4, math.pi, 2.0, 'wrap'), (8, 0.3, 6.0, 'col0'), (12, math.pi, 6.0, 'full'), (8, math.pi, 2.0, 'one')])
def test_twin_force_is_the_gradient_of_its_action(L, amp, beta, dk):
    """central differences of S_d in long double, on and next to the defect; 1e-6 relative to the largest force"""
    B = 3
    df, g = DC.defect_of(dk, L), DC.couplings(B, beta, 0)
    x = DC.links(B, L, 300 + L, amp)
    F = DC.force(x, beta, g, df, LD)
    h = LD(1e-5)
    rng = np.random.default_rng(L)
    on = np.argwhere(DC.mask(L, df))
    sites = [(rng.integers(B), rng.integers(2), rng.integers(L), rng.integers(L)) for _ in range(16)]
    sites += [(b, mu, (i + di) % L, (j + dj) % L) for b in range(B) for mu in range(2) for i, j in on[:2] for di, dj in ((0, 0), (1, 0), (0, 1))]
    worst = 0.0
    for b, mu, i, j in sites:
        xp, xm = x.astype(LD), x.astype(LD)
        xp[b, mu, i, j] += h; xm[b, mu, i, j] -= h
        d = (DC.action(xp, beta, g, df, LD)[0][b] - DC.action(xm, beta, g, df, LD)[0][b]) / (2 * h)
        worst = max(worst, float(abs(d - F[b, mu, i, j])))
    scale = float(np.abs(F).max())
    print(f'L {L} {dk}: |central difference - force| max {worst:.2e}, force scale {scale:.2e}')
    assert worst <= 1e-6 * scale


def test_float64_twin_against_the_long_double_twin_and_no_chain_is_left_out():
    """the rounding figures of the float64 arithmetic on the committed cases (the GPU tests' bounds are the project's figures for the
    plain kernels, or 8x these where a case needs more), and the cap: no chain of any case is left out"""
    worst = {'force': 0.0, 'S': 0.0, 'H0': 0.0, 'x_new': 0.0, 'dH': 0.0, 'H1': 0.0, 'csum': 0.0, 'dsum': 0.0}
    for c in DC.CASES:
        B, L, amp, beta, nstep, integ, dk = c
        x, v, u, g, df, ref = DC.case(c)
        assert not ref['left_out'].any(), (DC.case_id(c), ref['u_margin'])
        r64 = DC.trajectory(x, v, u, beta, g, df, DC.DT, nstep, integ, dt=np.float64)
        assert np.array_equal(r64['acc'], ref['acc']) and not r64['left_out'].any(), DC.case_id(c)
        assert np.array_equal(r64['Q'], ref['Q']), DC.case_id(c)
        F64, FLD = DC.force(x, beta, g, df, np.float64), DC.force(x, beta, g, df, LD)
        S64, SLD = DC.action(x, beta, g, df, np.float64)[0], DC.action(x, beta, g, df, LD)[0]
        fig = {'force': DC.rel_err(F64, FLD), 'S': float(np.abs((S64.astype(LD) - SLD) / SLD).max()),
               'H0': float(np.abs((r64['H0'].astype(LD) - ref['H0']) / ref['H0']).max()),
               'x_new': float(np.abs(r64['x_new'].astype(LD) - ref['x_new']).max()),
               'dH': float(np.abs(r64['dH'].astype(LD) - ref['dH']).max()),
               'H1': float(np.abs((r64['H1'].astype(LD) - ref['H1']) / ref['H1']).max()),
               'csum': DC.rel_err(r64['csum'], ref['csum']), 'dsum': float(np.abs(r64['dsum'].astype(LD) - ref['dsum']).max())}
        for k, val in fig.items():
            worst[k] = max(worst[k], val)
    print('float64 twin vs long double twin, worst over the cases:', {k: f'{val:.2e}' for k, val in worst.items()})
    # far inside the project's figures for the plain kernels: the 8x rule never widens a bound on these cases
    assert 8 * worst['force'] <= 1e-11 and 8 * worst['S'] <= 1e-10 and 8 * worst['H0'] <= 1e-10 and 8 * worst['x_new'] <= 1e-9
    assert 8 * worst['H1'] <= 1e-8 and 8 * worst['dH'] <= 1e-9 and 8 * worst['csum'] <= 1e-11


def test_cases_cover_what_they_claim():
    seen = {k: set() for k in ('shape', 'amp', 'beta', 'nstep', 'integ', 'defect')}
    for B, L, amp, beta, nstep, integ, dk in DC.CASES:
        for k, val in zip(seen, ((B, L), amp, beta, nstep, integ, dk)):
            seen[k].add(val)
        seen.setdefault(('defect', dk), set()).update({('amp', amp), ('beta', beta), ('nstep', nstep), ('integ', integ)})
    assert seen['shape'] == set(DC.SHAPES) and seen['amp'] == set(DC.AMPS) and seen['beta'] == set(DC.BETAS)
    assert seen['nstep'] == set(DC.NSTEPS) and seen['integ'] == set(DC.INTEGRATORS) and seen['defect'] == set(DC.DEFECTS)
    for dk in DC.DEFECTS:
        assert len(seen[('defect', dk)]) == 2 + 2 + 2 + 3, dk                # every defect meets every value of every axis
        assert {(B, L) for B, L, a, b, n, i, d in DC.CASES if d == dk} == set(DC.SHAPES), dk
    assert len(DC.CASES) == len(set(DC.CASES)) == len(DC.DEFECTS) * len(DC.SHAPES)
    assert (3, 32) in DC.SHAPES_ONE_LAUNCH and (2, 36) in DC.SHAPES_ONE_LAUNCH and (2, 64) in DC.SHAPES_ONE_LAUNCH
    for L in (4, 8, 36, 128):
        m = {dk: DC.mask(L, DC.defect_of(dk, L)) for dk in DC.DEFECTS}
        assert m['none'].sum() == 0 and m['one'].sum() == 1 and m['full'].sum() == L and m['full'][:, 1].all()
        assert m['wrap'].sum() == min(4, L) and m['wrap'][L - 2, L - 1] and m['wrap'][0, L - 1] and m['col0'][3:6, 0].sum() == min(3, L - 3)
    for B, beta in ((3, 2.0), (5, 6.0)):
        assert set(DC.couplings(B, beta, 0)) == {0.0, beta / 3.0, beta}
    # the twin's translation and swap against their statements
    x = DC.links(3, 8, 1, 1.0)
    t = DC.translate(x, [0, 2, 2], 2, [[1, 2], [3, 7], [0, 0]])
    assert np.array_equal(t[0], x[0]) and np.array_equal(t[2], x[2]) and t[1, 1, (2 + 3) % 8, (5 + 7) % 8] == x[1, 1, 2, 5]
    gs = np.array([0.0, 1.0, 2.0])
    g_b, rung, chain_of = gs.copy(), np.arange(3), np.arange(3)
    a = DC.swap(gs, np.array([1.0, 0.0, 5.0]), np.array([[0.5, 0.5]]), g_b, rung, chain_of, 0)     # d = (0 - 1)(0 - 1) = 1: accepted
    assert list(a[0]) == [1.0, -1.0] and list(rung) == [1, 0, 2] and list(chain_of) == [1, 0, 2] and list(g_b) == [1.0, 0.0, 2.0]
    a = DC.swap(gs, np.array([1.0, 0.0, -5.0]), np.array([[0.5, 0.5]]), g_b, rung, chain_of, 1)    # pair (1, 2): chains 0 and 2, d = (1 - 2)(-5 - 1) = 6
    assert a[0][0] == -1.0 and a[0][1] == (1.0 if 0.5 < math.exp((1.0 - 2.0) * (-5.0 - 1.0)) else 0.0)


# ---------------------------------------------------------------- the exact defect plaquette
def test_exact_defect_plaquette_against_its_limits_a_brute_force_sum_and_a_sampled_run():
    from fthmc_amd.utils.observables import exact_defect_plaquette, exact_wilson_loop
    for beta, L in ((6.0, 16), (2.0, 8), (0.7, 4)):
        w = exact_wilson_loop(beta, L, 1, 1)
        for Ld in (1, 4, L):
            assert abs(exact_defect_plaquette(beta, L, 1.0, Ld) - w) <= 1e-13 and abs(exact_defect_plaquette(beta, L, 1.0, Ld, False) - w) <= 1e-13
        assert abs(exact_defect_plaquette(beta, L, 0.3, 0, False) - w) <= 1e-13
        assert exact_defect_plaquette(beta, L, 0.0, 3) == 0.0
        assert abs(exact_defect_plaquette(beta, L, 1e-9, 3) - 0.5e-9 * beta) <= 1e-15          # I_1(y) / I_0(y) -> y / 2
        assert abs(exact_defect_plaquette(beta, L, 0.0, 3, False) - exact_defect_plaquette(beta, L, 1e-12, 3, False)) <= 1e-12
    with pytest.raises(ValueError):
        exact_defect_plaquette(6.0, 16, 0.5, 0)
    with pytest.raises(ValueError):
        exact_defect_plaquette(6.0, 16, 1.5, 4)

    def bessel(n, y, terms=400):                                          # I_n(y) by its power series, long double
        y, s, t = LD(y), LD(0), None
        for k in range(terms):
            t = (y / 2) ** n / LD(math.factorial(n)) if k == 0 else t * (y / 2) ** 2 / (LD(k) * LD(k + n))
            s += t
        return s

    def brute(beta, V, c, Ld, on, nmax=30):
        num = den = LD(0)
        y = c * beta if on else beta
        for n in range(-nmax, nmax + 1):
            a = abs(n)
            w = bessel(a, beta) ** (V - Ld) * bessel(a, c * beta) ** Ld
            dI = (bessel(abs(a - 1), y) + bessel(a + 1, y)) / 2
            num += w * dI / bessel(a, y); den += w
        return float(num / den)
    for beta, L, c, Ld in ((6.0, 4, 1 / 7, 2), (2.0, 4, 0.5, 4), (3.0, 6, 0.9, 1)):
        for on in (True, False):
            e, b = exact_defect_plaquette(beta, L, c, Ld, on), brute(beta, L * L, c, Ld, on)
            print(f'beta {beta} L {L} c {c:.3f} Ld {Ld} on {on}: {e:.15f} brute {b:.15f}')
            assert abs(e - b) <= 1e-12
    # a sampled run (L = 16, beta = 6, Ld = 4, K = 8 rungs linear in c): 0.3935 on the defect at c = 1 / 7 and 0.9124 off it, to its 3e-3
    assert abs(exact_defect_plaquette(6.0, 16, 1 / 7, 4) - 0.3935) <= 3e-3
    assert abs(exact_defect_plaquette(6.0, 16, 1 / 7, 4, False) - 0.9124) <= 3e-3


# ---------------------------------------------------------------- the twin as a sampler
def test_twin_sampler_reproduces_the_exact_charge_moment_on_the_periodic_rung():
    """L = 16, beta = 6 (plain HMC is frozen there), 32 ladders of K = 8 rungs linear in c, a defect of 4 plaquettes, 600 leapfrog
    trajectories (tau = 1, 10 steps) from a cold start, a swap round and a translation of the top rung after every trajectory: <Q^2> of
    rung K - 1 within |z| <= 4 of the exact value (jackknife over the ladders), every swap pair accepted at >= 0.2.  The averages leave
    out the first 100 trajectories, as the GPU test does (tests/test_z_defect_gpu.py): a cold start has Q = 0 and cos P = 1 everywhere, a
    bias of the mean the error bar knows nothing of; the figure over all 600 is printed beside it"""
    from fthmc_amd.utils.observables import exact_charge_moment, exact_defect_plaquette
    M, K = 32, 8
    cs = np.linspace(0.0, 1.0, K)
    r = DC.sampler(16, 6.0, cs, M, 600, (0, 0, 4))
    exact = exact_charge_moment(6.0, 16)
    therm = 100
    print(f'all 600 trajectories: <Q^2> {float((r["Q"] ** 2).mean()):.4f}')
    q2 = (r['Q'][therm:] ** 2).mean(axis=0)                               # per ladder
    jk = (q2.sum() - q2) / (M - 1)
    mean, err = q2.mean(), math.sqrt((M - 1) * np.mean((jk - jk.mean()) ** 2))
    z = (mean - exact) / err
    dp = r['dplaq'][therm:].mean(axis=(0, 2))
    print(f'<Q^2> {mean:.4f} +- {err:.4f}, exact {exact:.4f}, z {z:+.2f}; acceptance {r["acc"]:.3f}, mean |dQ| {r["dq"]:.4f}, swaps '
          f'{np.round(r["swap_acc"], 3)}; defect <cos P> {np.round(dp, 4)} exact '
          f'{np.round([exact_defect_plaquette(6.0, 16, c, 4) for c in cs], 4)}')
    assert abs(exact - 1.1947014482) < 1e-6
    assert abs(z) <= 4.0
    assert (r['swap_acc'] >= 0.2).all()
    assert r['dq'] > 0.1 and r['acc'] > 0.5


# ---------------------------------------------------------------- the entry points under the sanitizers
def test_defect_entry_points_walk_clean_under_asan_and_ubsan(tmp_path):
    """tests/hip/defect_walk.cpp: a stand-alone program against the host-side sanitizer build of the library (launches are no-ops
    there), built with -fsanitize=address,undefined by the recipe next to `make san`'s: the five entry points through their refusals,
    the workspace rule, legal calls on every path up to the largest shapes.  Its own process, nothing preloaded."""
    csrc = os.path.join(ROOT, 'fthmc_amd', 'csrc')
    exe = str(tmp_path / 'defect_walk')
    r = subprocess.run(['make', '-C', csrc, '-f', 'san.mk', 'san_defect', 'SANEXE=' + exe], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and os.path.exists(exe), r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ)
    env.update(ASAN_OPTIONS='detect_leaks=1:abort_on_error=1:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert 'ERROR: AddressSanitizer' not in r.stderr and 'runtime error:' not in r.stderr, r.stderr[-6000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out['calls'] > 300 and out['refusals'] >= 80
