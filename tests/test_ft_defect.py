"""CPU-only tests of boundary-condition tempering through the flow (ftHMC with a defect on the physical field): the C ABI
declares and exports the four entry points and the wrappers, the driver and the `fthmc` aliases exist; the refusals refuse, in the
header's order; the workspace rule; the torch float64 twin of tests/ft_defect_cases.py has a force that is the gradient of its own
action, is oracle.ref_cpu.ft_hmc with g = beta, is tests/defect_cases.trajectory without layers and leaves no chain out on the
committed seeds; the flow commutes with the translations by multiples of 4 and with no others; the entry points' host side as a
stand-alone program under AddressSanitizer + UBSan."""
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

import defect_cases as DC
import ft_defect_cases as FD
import meta_cases as MC

ENTRY_POINTS = ('fthmc_ft_defect_ws_bytes', 'fthmc_ft_defect_trajectory_v', 'fthmc_ft_defect_force_v', 'fthmc_ft_defect_action_v')


def test_header_library_wrappers_driver_and_alias_carry_the_new_entry_points():
    import ctypes
    from fthmc_amd import _lib, ops
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'fthmc_hip.h')).read()
    declared = re.findall(r'\b(fthmc_[a-z0-9_]+)\s*\(', header)
    for name in ENTRY_POINTS:
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    # the section stands behind the last declaration the header had, and every declaration of it says what the reference has
    assert declared.index('fthmc_ft_defect_ws_bytes') > declared.index('fthmc_profile_stages')
    section = header[header.index('---- Flowed boundary-condition tempering'):]
    assert section.count('No reference counterpart.') == 3 and 'The reference has no counterpart' in section   # force and action share theirs
    sig = _lib.SIGNATURES['fthmc_ft_defect_trajectory_v']
    assert len(sig) == 31 and sig[9] is ctypes.c_double and sig[10] is ctypes.c_void_p and sig[11:14] == [ctypes.c_int] * 3
    assert sig[14] is ctypes.c_double and sig[15:17] == [ctypes.c_int] * 2 and sig[28] is ctypes.c_size_t and sig[30] is ctypes.c_uint64
    assert len(_lib.SIGNATURES['fthmc_ft_defect_force_v']) == 17 and len(_lib.SIGNATURES['fthmc_ft_defect_action_v']) == 21
    assert lib.fthmc_ft_defect_ws_bytes.restype is ctypes.c_size_t
    p = inspect.signature(ops.ft_defect_trajectory).parameters
    assert list(p) == ['x', 'v', 'u', 'w', 'n_layers', 'beta', 'g_b', 'defect', 'dt', 'nstep', 'act', 'integrator', 'out', 'state_in', 'groups',
                       'arch', 'wkey', 'side_streams']
    assert [p[k].default for k in list(p)[10:]] == ['silu', 'leapfrog', None, None, 1, None, None, None]
    p = inspect.signature(ops.ft_defect_force).parameters
    assert list(p) == ['x', 'w', 'n_layers', 'beta', 'g_b', 'defect', 'act', 'arch', 'wkey']
    assert list(inspect.signature(ops.ft_defect_action).parameters) == list(p)
    assert list(inspect.signature(ops.ft_defect_ws_bytes).parameters) == ['B', 'L', 'n_layers', 'arch']
    import fthmc
    import fthmc_amd
    import fthmc.defect as d1
    import fthmc_amd.defect as d2
    assert d1 is d2 and fthmc.run_ft_ptbc is d2.run_ft_ptbc is fthmc_amd.run_ft_ptbc and fthmc.run_ptbc is d2.run_ptbc
    p = inspect.signature(d2.run_ft_ptbc).parameters
    assert list(p) == ['param', 'flow', 'cs', 'n_ladders', 'ntraj', 'defect', 'swap_every', 'translate', 'integrator', 'seed', 'x', 'captured',
                       'shard', 'act']
    assert [p[k].default for k in list(p)[5:]] == [None, 1, True, 'leapfrog', None, None, True, None, 'silu']
    # run_ptbc itself keeps its arguments (tests/test_defect.py pins the list)
    assert 'flow' not in inspect.signature(d2.run_ptbc).parameters
    with pytest.raises(ValueError):
        d2.run_ft_ptbc(None, None, [0.0, 1.0], 1, 1)
    # no torch operator for this feature: the operator table stays what tests/test_torch_boundary.py pins
    import fthmc_amd.torch_ops as TO
    assert not [n for n in TO.__all__ if 'defect' in n]


def test_refusals_their_order_and_the_workspace_rule():
    """the argument checks of the C entry points come before anything touches the device: stand-in addresses are never read"""
    from fthmc_amd import _lib
    lib = _lib.load()
    X, V, U, G, O, W, F, WT = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000, 0x70000000, 0x80000000
    ARG, UNS, WS = -1, -2, -4
    inf, nan = float('inf'), float('nan')

    def traj(x=X, v=V, u=U, w=WT, arch=None, nl=2, B=4, L=8, act=0, beta=2.0, g=G, i0=6, j0=7, Ld=4, nstep=2, integ=0, out=O, ws=None, nbytes=0):
        return lib.fthmc_ft_defect_trajectory_v(x, v, u, w, arch, nl, B, L, act, beta, g, i0, j0, Ld, 0.1, nstep, integ, out, None, None, None,
                                                None, None, None, None, None, None, ws, nbytes, None, 0)

    def frc(x=X, w=WT, arch=None, nl=2, B=4, L=8, act=0, beta=2.0, g=G, i0=6, j0=7, Ld=4, out=F, ws=None, nbytes=0):
        return lib.fthmc_ft_defect_force_v(x, w, arch, nl, B, L, act, beta, g, i0, j0, Ld, out, ws, nbytes, None, 0)

    def act_(x=X, w=WT, arch=None, nl=2, B=4, L=8, act=0, beta=2.0, g=G, i0=6, j0=7, Ld=4, ws=None, nbytes=0):
        return lib.fthmc_ft_defect_action_v(x, w, arch, nl, B, L, act, beta, g, i0, j0, Ld, O, None, None, None, None, ws, nbytes, None, 0)
    for f in (traj, frc, act_):
        assert f(x=None) == ARG and f(g=None) == ARG and f(w=None) == ARG and f(nl=-1) == ARG
        for B in (0, -1, 4194304):
            assert f(B=B) == ARG
        for L in (0, 2, 6, 10, -8, 32768):
            assert f(L=L, i0=0, j0=0, Ld=0) == ARG
        for Ld in (-1, 9, 2 ** 31 - 1):
            assert f(Ld=Ld) == ARG
        for s in (-1, 8, 2 ** 31 - 1):
            assert f(i0=s) == ARG and f(j0=s) == ARG
        for beta in (inf, -inf, nan):
            assert f(beta=beta) == ARG
        assert f(Ld=0, ws=None) == WS and f(Ld=8) == WS                   # the edges of the defect are legal: the next refusal answers
        # FTHMC_ERR_UNSUPPORTED behind every FTHMC_ERR_ARG and before the workspace (none is given here)
        assert f(act=3) == UNS and f(act=-1) == UNS and f(act=3, Ld=9) == ARG
        assert f(B=65536, L=20) == UNS and f(B=65536, L=20, beta=nan) == ARG
        # then the workspace
        need = lib.fthmc_ft_defect_ws_bytes(None, 4, 8, 2)
        assert f() == WS and f(ws=W, nbytes=need - 1) == WS and f(ws=None, nbytes=need) == WS
    assert traj(v=None) == ARG and traj(u=None) == ARG and traj(out=None) == ARG and frc(out=None) == ARG
    for n in (0, -1):
        assert traj(nstep=n) == ARG
    assert traj(integ=3) == UNS and traj(integ=-1) == UNS and traj(integ=3, nstep=0) == ARG and traj(integ=3, beta=nan) == ARG
    # the force and action entry points always run the sequenced kernels (B <= 65535); the trajectory only where it is sequenced
    lib.fthmc_set_small_path(1)
    assert frc(B=65536) == UNS and act_(B=65536) == UNS and traj(B=65536) == WS
    lib.fthmc_set_small_path(0)
    try:
        assert traj(B=65536) == UNS
    finally:
        lib.fthmc_set_small_path(1)
    # the workspace rule: fthmc_ws_bytes and the three rows of chain sums (C, Dsum, Q), rounded like every region
    wsb = lib.fthmc_ft_defect_ws_bytes
    for B, L, nl in ((4, 8, 2), (3, 20, 2), (1, 4, 0), (130, 16, 4), (65535, 4, 0)):
        base = lib.fthmc_ws_bytes(None, B, L, nl)
        assert base > 0 and wsb(None, B, L, nl) == base + (3 * B * 8 + 255) // 256 * 256 and wsb(None, B, L, nl) % 256 == 0
    assert wsb(None, 0, 8, 2) == 0 and wsb(None, 4, 0, 2) == 0 and wsb(None, 4, 8, -1) == 0
    from fthmc_amd import ops
    arch = ((4, 6, 5), 5, 3)
    assert ops.ft_defect_ws_bytes(4, 8, 2, arch) == ops.ws_bytes(4, 8, 2, arch) + 256


# ---------------------------------------------------------------- the twin
@pytest.mark.parametrize('dk,amp', [('wrap', 0.3), ('full', 3.1), ('one', 3.1), ('col0', 1.0)])
def test_twin_force_is_the_gradient_of_its_own_action(dk, amp):
    """central differences of the twin's S, on the defect's links and elsewhere: 1e-6 relative (tests/test_ft_meta.py's bound)"""
    B, L, nl, beta = 3, 8, 2, 2.0
    df, g = DC.defect_of(dk, L), torch.from_numpy(DC.couplings(B, beta, 0))
    flow = FD.flow_of('one', nl, 1.0)
    x = torch.from_numpy(MC.links(B, L, 321, amp))
    F = FD.force(x, flow, beta, g, df)
    h, rng, worst = 1e-5, np.random.default_rng(8), 0.0
    sites = [(0, df[0], df[1]), (1, df[0], df[1])] + [tuple(int(rng.integers(0, n)) for n in (2, L, L)) for _ in range(10)]
    for mu, i, j in sites:
        xp, xm = x.clone(), x.clone()
        xp[:, mu, i, j] += h
        xm[:, mu, i, j] -= h
        with torch.no_grad():
            fd = (FD.action(xp, flow, beta, g, df)[0] - FD.action(xm, flow, beta, g, df)[0]) / (2 * h)
        worst = max(worst, float((fd - F[:, mu, i, j]).abs().max()))
    assert worst <= 1e-6 * max(1.0, float(F.abs().max())), worst


@pytest.mark.parametrize('nstep', [1, 3])
def test_twin_with_g_equal_to_beta_is_the_reference_trajectory(nstep):
    """leapfrog with g = beta on every chain (any defect) = oracle.ref_cpu.ft_hmc(mode='md'), to rounding"""
    B, L, nl, beta = 3, 8, 2, 3.0
    flow = FD.flow_of('one', nl, 1.0)
    x = torch.from_numpy(MC.links(B, L, 55, 1.0))
    v, u = MC.draws(B, L, 56)
    v = torch.from_numpy(v)
    dH, _, acc, newx, h0, h1 = FD.R.ft_hmc(x, v, torch.from_numpy(u), flow, beta, 0.1, nstep)
    for dk in ('none', 'wrap', 'full'):
        r = FD.trajectory(x, v, u, flow, beta, np.full(B, beta), DC.defect_of(dk, L), 0.1, nstep, 'leapfrog')
        assert np.array_equal(r['acc'], acc.numpy())
        np.testing.assert_allclose(r['H0'], h0.numpy(), rtol=1e-14)
        np.testing.assert_allclose(r['H1'], h1.numpy(), rtol=1e-12)
        np.testing.assert_allclose(r['dH'], dH.numpy(), rtol=1e-9, atol=1e-11)
        np.testing.assert_allclose(r['x_new'], newx.numpy(), rtol=0, atol=1e-12)


@pytest.mark.parametrize('integ,dk', [('leapfrog', 'wrap'), ('omelyan', 'full'), ('force_gradient', 'col0')])
def test_twin_without_layers_is_the_plain_twin_in_float64(integ, dk):
    """no layers: tests/defect_cases.trajectory evaluated in float64, to rounding"""
    B, L, beta, nstep = 3, 8, 2.0, 2
    x = MC.links(B, L, 61, 1.0)
    v, u = MC.draws(B, L, 62)
    g, df = DC.couplings(B, beta, 1), DC.defect_of(dk, L)
    r = FD.trajectory(torch.from_numpy(x), torch.from_numpy(v), u, [], beta, g, df, 0.1, nstep, integ)
    p = DC.trajectory(x, v, u, beta, g, df, 0.1, nstep, integ, dt=np.float64)
    assert np.array_equal(r['acc'], p['acc']) and np.array_equal(np.rint(r['Q']), p['Q'])
    np.testing.assert_allclose(r['H0'], p['H0'], rtol=1e-13)
    np.testing.assert_allclose(r['H1'], p['H1'], rtol=1e-12)
    np.testing.assert_allclose(r['dsum'], p['dsum'], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(r['plaq'], p['csum'] / (L * L), rtol=1e-12)
    np.testing.assert_allclose(r['x_new'], p['x_new'], rtol=0, atol=1e-12)


def test_no_chain_is_left_out_on_the_committed_seeds():
    left, umin = 0, np.inf
    for c in FD.CASES:
        r = FD.case(c)[6]
        left += int(r['left_out'].sum())
        with np.errstate(divide='ignore', over='ignore', invalid='ignore'):
            umin = min(umin, float(np.nanmin(r['u_margin'] / np.exp(-r['dH']))))
    print(f'{len(FD.CASES)} cases, {left} chains left out; smallest accept margin {umin:.3e} exp(-dH)')
    assert left == 0 and umin >= FD.U_MARGIN
    # the cases are the issue's table: every path's shapes, every defect, every integrator, both steepnesses, mixed couplings
    assert {c[0] for c in FD.CASES} == {'one', 'off', 'tiled', 'valu', 'gen', 'nolayers'}
    assert {(c[1], c[2], c[3]) for c in FD.CASES if c[0] == 'one'} == {(3, 8, 2), (2, 12, 3), (4, 16, 4)}
    assert {(c[1], c[2], c[3]) for c in FD.CASES if c[0] == 'tiled'} == {(2, 20, 2), (2, 32, 2), (2, 64, 2)}
    assert {c[7] for c in FD.CASES} == set(MC.INTEGRATORS) and {c[9] for c in FD.CASES} == {1.0, 3.0}
    assert all({c[8] for c in FD.CASES if c[:4] == s} == set(DC.DEFECTS) for s in {c[:4] for c in FD.CASES})
    assert all(len(set(FD.inputs(c)[3])) > 1 for c in FD.CASES)


@pytest.mark.parametrize('L,nl', [(8, 8), (12, 3), (16, 5)])
def test_the_flow_commutes_with_translations_by_multiples_of_four_only(L, nl):
    """the stripe masks have period 4 across the stripes: F(roll x) = roll F(x) and the same log det J for shifts that are multiples of 4
    in both directions (1e-12), and for no shift of 1 (above 1e-3)"""
    flow = FD.R.default_flow(nl, torch.Generator().manual_seed(3))
    x = torch.from_numpy(MC.links(2, L, 70 + L, 1.0))
    with torch.no_grad():
        y, ld = FD.R.flow_forward(x, flow)
        for sh in ((4, 0), (0, 4), (4, 8), (L - 4, 4)):
            ys, lds = FD.R.flow_forward(torch.roll(x, sh, (2, 3)), flow)
            assert float((ys - torch.roll(y, sh, (2, 3))).abs().max()) <= 1e-12 and float((lds - ld).abs().max()) <= 1e-12, sh
        for sh in ((1, 0), (0, 1), (1, 1)):
            ys, lds = FD.R.flow_forward(torch.roll(x, sh, (2, 3)), flow)
            assert float((ys - torch.roll(y, sh, (2, 3))).abs().max()) > 1e-3, sh


# ---------------------------------------------------------------- the entry points under the sanitizers
def test_ft_defect_entry_points_walk_clean_under_asan_and_ubsan(tmp_path):
    """tests/hip/ft_defect_walk.cpp: a stand-alone program against the host-side sanitizer build of the library (launches are no-ops
    there), built with -fsanitize=address,undefined by the generic recipe next to `make san`'s: the four entry points through their
    refusals and precedence, the workspace rule, legal calls on every branch up to the largest shapes.  Its own process, nothing
    preloaded."""
    csrc = os.path.join(ROOT, 'fthmc_amd', 'csrc')
    exe = str(tmp_path / 'ft_defect_walk')
    r = subprocess.run(['make', '-C', csrc, '-f', 'san.mk', 'san_ft_defect', 'SANEXE=' + exe], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and os.path.exists(exe), r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ)
    env.update(ASAN_OPTIONS='detect_leaks=1:abort_on_error=1:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert 'ERROR: AddressSanitizer' not in r.stderr and 'runtime error:' not in r.stderr, r.stderr[-6000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out['calls'] > 3000 and out['refusals'] >= 300
