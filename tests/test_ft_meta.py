"""CPU-only tests of metadynamics ftHMC (the bias in the charge through the flow): the C ABI declares and exports the
four entry points and the wrappers, the driver and the `fthmc` aliases exist; the refusals refuse, in the header's order; the
workspace rule; the row rule of the chain groups; the torch float64 twin of tests/ft_meta_cases.py has a force that is the gradient
of its own S_b (inside the table and on the wall), is oracle.ref_cpu.ft_hmc under a zero table and leaves no chain out on the
committed seeds; the entry points' host side as a stand-alone program under AddressSanitizer + UBSan."""
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

import ft_meta_cases as FC
import meta_cases as MC

ENTRY_POINTS = ('fthmc_ft_meta_ws_bytes', 'fthmc_ft_meta_trajectory_v', 'fthmc_ft_meta_force_v', 'fthmc_ft_meta_action_v')


def test_header_library_wrappers_driver_and_alias_carry_the_new_entry_points():
    import ctypes
    from fthmc_amd import _lib, ops
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'fthmc_hip.h')).read()
    declared = set(re.findall(r'\b(fthmc_[a-z0-9_]+)\s*\(', header))
    for name in ENTRY_POINTS:
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    section = header[header.index('Metadynamics ftHMC'):header.index('/* ---- training')]
    assert section.count('No reference counterpart.') >= 3 and 'The reference has no counterpart' in section
    sig = _lib.SIGNATURES['fthmc_ft_meta_trajectory_v']
    assert len(sig) == 33 and sig[9] is ctypes.c_double and sig[12] is ctypes.c_int and sig[13] is _lib.SIGNATURES['fthmc_meta_force'][4]
    assert sig[16] is ctypes.c_double and sig[17] is ctypes.c_double and sig[30] is ctypes.c_size_t and sig[32] is ctypes.c_uint64
    assert len(_lib.SIGNATURES['fthmc_ft_meta_force_v']) == 18 and len(_lib.SIGNATURES['fthmc_ft_meta_action_v']) == 21
    assert lib.fthmc_ft_meta_ws_bytes.restype is ctypes.c_size_t
    p = inspect.signature(ops.ft_meta_trajectory).parameters
    assert list(p) == ['x', 'v', 'u', 'w', 'n_layers', 'beta', 'dt', 'nstep', 'table', 'qmax', 'wall', 'act', 'integrator', 'out', 'state_in',
                       'groups', 'arch', 'wkey', 'side_streams']
    assert [p[k].default for k in list(p)[10:]] == [0.0, 'silu', 'leapfrog', None, None, 1, None, None, None]
    p = inspect.signature(ops.ft_meta_force).parameters
    assert list(p) == ['x', 'w', 'n_layers', 'beta', 'table', 'qmax', 'wall', 'act', 'arch', 'wkey'] and p['wall'].default == 0.0
    assert list(inspect.signature(ops.ft_meta_action).parameters) == list(p)
    assert list(inspect.signature(ops.ft_meta_ws_bytes).parameters) == ['B', 'L', 'n_layers', 'arch']
    import fthmc
    import fthmc_amd
    import fthmc.meta as m1
    import fthmc_amd.meta as m2
    assert m1 is m2 and fthmc.run_ft_meta is m2.run_ft_meta is fthmc_amd.run_ft_meta and fthmc.run_meta is m2.run_meta
    p = inspect.signature(m2.run_ft_meta).parameters
    assert list(p) == ['param', 'flow', 'x', 'potential', 'n_build', 'w', 'integrator', 'use_graph', 'act']
    assert [p[k].default for k in list(p)[2:]] == [None, None, 0, 0.0, 'leapfrog', None, 'silu']
    # run_meta itself keeps its arguments: no flow is its only form (tests/test_meta.py pins the list)
    assert 'flow' not in inspect.signature(m2.run_meta).parameters
    with pytest.raises(ValueError):
        m2.run_ft_meta(None, None)
    # no torch operator for this feature: the operator table stays what tests/test_torch_boundary.py pins
    import fthmc_amd.torch_ops as TO
    assert not [n for n in TO.__all__ if 'meta' in n]


def test_refusals_their_order_and_the_workspace_rule():
    """the argument checks of the C entry points come before anything touches the device: stand-in addresses are never read"""
    from fthmc_amd import _lib
    lib = _lib.load()
    X, V, U, T, O, W, F, WT = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000, 0x70000000, 0x80000000
    ARG, UNS, WS = -1, -2, -4
    inf, nan = float('inf'), float('nan')

    def traj(x=X, v=V, u=U, w=WT, arch=None, nl=2, B=4, L=8, act=0, nstep=2, integ=0, tab=T, G=2, nb=11, qmax=2.0, wall=1.0, out=O, ws=None,
             nbytes=0):
        return lib.fthmc_ft_meta_trajectory_v(x, v, u, w, arch, nl, B, L, act, 2.0, 0.1, nstep, integ, tab, G, nb, qmax, wall, out, None, None,
                                              None, None, None, None, None, None, None, None, ws, nbytes, None, 0)

    def frc(x=X, w=WT, arch=None, nl=2, B=4, L=8, act=0, tab=T, G=2, nb=11, qmax=2.0, wall=1.0, out=F, ws=None, nbytes=0):
        return lib.fthmc_ft_meta_force_v(x, w, arch, nl, B, L, act, 2.0, tab, G, nb, qmax, wall, out, ws, nbytes, None, 0)

    def act_(x=X, w=WT, arch=None, nl=2, B=4, L=8, act=0, tab=T, G=2, nb=11, qmax=2.0, wall=1.0, ws=None, nbytes=0):
        return lib.fthmc_ft_meta_action_v(x, w, arch, nl, B, L, act, 2.0, tab, G, nb, qmax, wall, O, None, None, None, ws, nbytes, None, 0)
    for f in (traj, frc, act_):
        assert f(x=None) == ARG and f(tab=None) == ARG and f(w=None) == ARG and f(nl=-1) == ARG
        for B in (0, -1, 4194304):
            assert f(B=B, G=1) == ARG
        for L in (0, 2, 6, 10, -8, 32768):
            assert f(L=L) == ARG
        for G in (0, -1, 3, 8):
            assert f(G=G) == ARG
        for nb in (1, 0, -5, 65537):
            assert f(nb=nb) == ARG
        for qmax in (0.0, -1.0, inf, -inf, nan):
            assert f(qmax=qmax) == ARG
        for wall in (-1.0, -1e-300, inf, nan):
            assert f(wall=wall) == ARG
        # FTHMC_ERR_UNSUPPORTED behind every FTHMC_ERR_ARG and before the workspace (none is given here)
        assert f(act=3) == UNS and f(act=-1) == UNS and f(act=3, nb=1) == ARG
        assert f(B=65536, G=1, L=20) == UNS and f(B=65536, G=1, L=20, wall=-1.0) == ARG
        # then the workspace
        need = lib.fthmc_ft_meta_ws_bytes(None, 4, 8, 2)
        assert f() == WS and f(ws=W, nbytes=need - 1) == WS and f(ws=None, nbytes=need) == WS
    assert traj(v=None) == ARG and traj(u=None) == ARG and traj(out=None) == ARG and frc(out=None) == ARG
    for n in (0, -1):
        assert traj(nstep=n) == ARG
    assert traj(integ=3) == UNS and traj(integ=-1) == UNS and traj(integ=3, nstep=0) == ARG and traj(integ=3, wall=nan) == ARG
    # the force and action entry points always run the sequenced kernels (B <= 65535); the trajectory only where it is sequenced
    lib.fthmc_set_small_path(1)
    assert frc(B=65536, G=1) == UNS and act_(B=65536, G=1) == UNS and traj(B=65536, G=1) == WS
    lib.fthmc_set_small_path(0)
    try:
        assert traj(B=65536, G=1) == UNS
    finally:
        lib.fthmc_set_small_path(1)
    # the workspace rule: fthmc_ws_bytes and the two rows of chain sums, rounded like every region
    wsb = lib.fthmc_ft_meta_ws_bytes
    for B, L, nl in ((4, 8, 2), (3, 20, 2), (1, 4, 0), (130, 16, 4), (65535, 4, 0)):
        base = lib.fthmc_ws_bytes(None, B, L, nl)
        assert base > 0 and wsb(None, B, L, nl) == base + (2 * B * 8 + 255) // 256 * 256 and wsb(None, B, L, nl) % 256 == 0
    assert wsb(None, 0, 8, 2) == 0 and wsb(None, 4, 0, 2) == 0 and wsb(None, 4, 8, -1) == 0
    from fthmc_amd import ops
    arch = ((4, 6, 5), 5, 3)
    assert ops.ft_meta_ws_bytes(4, 8, 2, arch) == ops.ws_bytes(4, 8, 2, arch) + 256


def test_the_row_rule_of_the_chain_groups():
    """with one row every group reads the whole table; otherwise a group must be whole rows and is handed its own"""
    from fthmc_amd import ops
    one, rows4 = torch.zeros(1, 11, dtype=torch.float64), torch.zeros(4, 11, dtype=torch.float64)
    assert ops._meta_group_rows(one, 8, ops._group_edges(2, 8)) == [None, None]
    assert ops._meta_group_rows(torch.zeros(11, dtype=torch.float64), 8, ops._group_edges(3, 8)) == [None, None, None]
    assert ops._meta_group_rows(rows4, 8, ops._group_edges(2, 8)) == [(0, 2), (2, 4)]
    assert ops._meta_group_rows(rows4, 8, ops._group_edges([2, 6], 8)) == [(0, 1), (1, 4)]
    assert ops._meta_group_rows(rows4, 8, ops._group_edges(4, 8)) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert ops._meta_group_rows(torch.zeros(8, 11, dtype=torch.float64), 8, ops._group_edges([3, 5], 8)) == [(0, 3), (3, 8)]
    for groups in (3, 8, [1, 7], [3, 5]):                                # an edge inside a row of two chains
        with pytest.raises(ValueError):
            ops._meta_group_rows(rows4, 8, ops._group_edges(groups, 8))
    with pytest.raises(ValueError):
        ops._meta_group_rows(torch.zeros(3, 11, dtype=torch.float64), 8, ops._group_edges(1, 8))


# ---------------------------------------------------------------- the twin
@pytest.mark.parametrize('tk,amp', [('quad', 0.3), ('quad', 3.1), ('wall', 3.1)])
def test_twin_force_is_the_gradient_of_its_own_action(tk, amp):
    """central differences of the twin's S_b on a smooth table, inside the table and on the wall: 1e-6 relative (tests/test_meta.py's bound)"""
    B, L, nl, beta = 3, 8, 2, 2.0
    tab = MC.table('quad', 1) if tk == 'quad' else MC.Table(np.zeros((1, 11)), 0.05, 10.0)      # |Q_m| > 0.05: every chain on the wall
    flow = FC.flow_of('one', nl, 1.0)
    x = torch.from_numpy(MC.links(B, L, 321, amp))
    F, margin = FC.force(x, flow, beta, tab)
    with torch.no_grad():
        qm = FC.charge_m(FC.R.flow_forward(x, flow)[0]).numpy()
    assert margin.min() > 1e-4
    assert np.all(np.abs(qm) > tab.qmax) if tk == 'wall' else np.all(np.abs(qm) < tab.qmax)
    h, rng, worst = 1e-5, np.random.default_rng(8), 0.0
    for _ in range(12):
        mu, i, j = (int(rng.integers(0, n)) for n in (2, L, L))
        xp, xm = x.clone(), x.clone()
        xp[:, mu, i, j] += h
        xm[:, mu, i, j] -= h
        with torch.no_grad():
            fd = (FC.biased_action(xp, flow, beta, tab)[0] - FC.biased_action(xm, flow, beta, tab)[0]) / (2 * h)
        worst = max(worst, float((fd - F[:, mu, i, j]).abs().max()))
    assert worst <= 1e-6 * max(1.0, float(F.abs().max())), worst


@pytest.mark.parametrize('integ_nstep', [1, 3])
def test_twin_with_a_zero_table_is_the_reference_trajectory(integ_nstep):
    """leapfrog under a zero table without a wall = oracle.ref_cpu.ft_hmc(mode='md'), to rounding"""
    B, L, nl, beta = 3, 8, 2, 3.0
    flow = FC.flow_of('one', nl, 1.0)
    x = torch.from_numpy(MC.links(B, L, 55, 1.0))
    v, u = MC.draws(B, L, 56)
    v = torch.from_numpy(v)
    r = FC.trajectory(x, v, u, flow, beta, 0.1, integ_nstep, 'leapfrog', MC.table('zero', 1))
    dH, _, acc, newx, h0, h1 = FC.R.ft_hmc(x, v, torch.from_numpy(u), flow, beta, 0.1, integ_nstep)
    assert np.array_equal(r['acc'], acc.numpy()) and not r['vbias'].any()
    np.testing.assert_allclose(r['H0'], h0.numpy(), rtol=1e-14)
    np.testing.assert_allclose(r['H1'], h1.numpy(), rtol=1e-12)
    np.testing.assert_allclose(r['dH'], dH.numpy(), rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(r['x_new'], newx.numpy(), rtol=0, atol=1e-12)


def test_no_chain_is_left_out_on_the_committed_seeds():
    left, tmin, umin = 0, np.inf, np.inf
    for c in FC.CASES:
        r = FC.case(c)[5]
        left += int(r['left_out'].sum())
        tmin = min(tmin, float(r['t_margin'].min()))
        with np.errstate(divide='ignore', over='ignore', invalid='ignore'):
            umin = min(umin, float(np.nanmin(r['u_margin'] / np.exp(-r['dH']))))
    print(f'{len(FC.CASES)} cases, {left} chains left out; smallest lookup margin {tmin:.3e}, smallest accept margin {umin:.3e} exp(-dH)')
    assert left == 0 and tmin >= FC.T_MARGIN and umin >= FC.U_MARGIN
    # the cases are the issue's table: every path, every table kind, both row layouts, both steepnesses, every integrator
    assert {c[0] for c in FC.CASES} == {'one', 'off', 'tiled', 'valu', 'gen', 'nolayers'}
    assert {(c[1], c[2], c[3]) for c in FC.CASES if c[0] == 'one'} == {(3, 8, 2), (2, 12, 3), (4, 16, 4)}
    assert {c[7] for c in FC.CASES} == set(MC.INTEGRATORS) and {c[10] for c in FC.CASES} == {1.0, 3.0}
    assert all({c[9] for c in FC.CASES if (c[0], c[1]) == (p, B)} == {1, B} for p, B in {(c[0], c[1]) for c in FC.CASES})


# ---------------------------------------------------------------- the entry points under the sanitizers
def test_ft_meta_entry_points_walk_clean_under_asan_and_ubsan(tmp_path):
    """tests/hip/ft_meta_walk.cpp: a stand-alone program against the host-side sanitizer build of the library (launches are no-ops
    there), built with -fsanitize=address,undefined by the recipe next to `make san`'s: the four entry points through their refusals
    and precedence, the workspace rule, legal calls on every branch up to the largest shapes.  Its own process, nothing preloaded."""
    csrc = os.path.join(ROOT, 'fthmc_amd', 'csrc')
    exe = str(tmp_path / 'ft_meta_walk')
    r = subprocess.run(['make', '-C', csrc, '-f', 'san.mk', 'san_ft_meta', 'SANFTMETA=' + exe], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and os.path.exists(exe), r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ)
    env.update(ASAN_OPTIONS='detect_leaks=1:abort_on_error=1:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert 'ERROR: AddressSanitizer' not in r.stderr and 'runtime error:' not in r.stderr, r.stderr[-6000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out['calls'] > 3000 and out['refusals'] >= 300
