"""CPU-only tests of metadynamics HMC (csrc/meta.hip): the C ABI declares and exports the five entry points and the
wrappers, the driver and the `fthmc` aliases exist, the refusals refuse; the numpy twin of tests/meta_cases.py has a force that is
the gradient of its own biased action, agrees with itself between float64 and long double (the rounding figures the GPU tests' 8x
rule rests on) and leaves no chain out on the committed inputs; the deposit's two-node split, range and chain order;
MetaPotential against the definitions; reweighted_mean on a constructed example; the twin as a sampler against the exact
<Q^2>; the entry points' host side as a stand-alone program under AddressSanitizer + UBSan."""
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

import meta_cases as MC

LD = np.longdouble
Q2_EXACT_L8_B4 = 0.4820159295
ENTRY_POINTS = ('fthmc_meta_ws_bytes', 'fthmc_meta_trajectory', 'fthmc_meta_deposit', 'fthmc_meta_force', 'fthmc_meta_action')


def test_header_library_wrappers_driver_and_alias_carry_the_new_entry_points():
    import ctypes
    from fthmc_amd import _lib, ops
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'fthmc_hip.h')).read()
    declared = set(re.findall(r'\b(fthmc_[a-z0-9_]+)\s*\(', header))
    for name in ENTRY_POINTS:
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert header.count('No reference counterpart.') >= 4                # one per declaration (force and action share theirs)
    sig = _lib.SIGNATURES['fthmc_meta_trajectory']
    assert len(sig) == 25 and sig[5] is ctypes.c_double and sig[8] is ctypes.c_int and sig[12] is ctypes.c_double and sig[23] is ctypes.c_size_t
    assert len(_lib.SIGNATURES['fthmc_meta_deposit']) == 8 and len(_lib.SIGNATURES['fthmc_meta_force']) == 11
    assert len(_lib.SIGNATURES['fthmc_meta_action']) == 13 and lib.fthmc_meta_ws_bytes.restype is ctypes.c_size_t
    p = inspect.signature(ops.meta_trajectory).parameters
    assert list(p) == ['x', 'v', 'u', 'beta', 'dt', 'nstep', 'table', 'qmax', 'wall', 'integrator', 'path', 'out']
    assert (p['wall'].default, p['integrator'].default, p['path'].default, p['out'].default) == (0.0, 'leapfrog', 0, None)
    assert list(inspect.signature(ops.meta_deposit).parameters) == ['qm', 'table', 'qmax', 'w']
    assert list(inspect.signature(ops.meta_force).parameters) == ['x', 'beta', 'table', 'qmax', 'wall']
    assert list(inspect.signature(ops.meta_action).parameters) == ['x', 'beta', 'table', 'qmax', 'wall', 'out']
    import fthmc
    import fthmc_amd
    import fthmc.meta as m1
    import fthmc_amd.meta as m2
    import fthmc.utils.observables as o1
    assert m1 is m2 and fthmc.run_meta is m2.run_meta is fthmc_amd.run_meta and fthmc.MetaPotential is m2.MetaPotential is fthmc_amd.MetaPotential
    p = inspect.signature(m2.run_meta).parameters
    assert list(p) == ['param', 'x', 'potential', 'n_build', 'w', 'integrator', 'use_graph']
    assert (p['x'].default, p['potential'].default, p['n_build'].default, p['w'].default, p['integrator'].default, p['use_graph'].default) == \
        (None, None, 0, 0.0, 'leapfrog', None)
    p = inspect.signature(m2.MetaPotential.__init__).parameters
    assert list(p) == ['self', 'nb', 'qmax', 'wall', 'groups'] and p['groups'].default == 1
    p = inspect.signature(o1.reweighted_mean).parameters
    assert list(p) == ['values', 'vbias', 'n_block'] and p['n_block'].default == o1.N_BLOCK
    # no torch operator for this feature: the operator table stays what tests/test_torch_boundary.py pins
    import fthmc_amd.torch_ops as TO
    assert not [n for n in TO.__all__ if 'meta' in n]


def test_refusals_refuse_and_the_workspace_rule():
    """the argument checks of the C entry points come before anything touches the device: stand-in addresses are never read"""
    from fthmc_amd import _lib, ops
    from fthmc_amd._lib import FthmcError
    lib = _lib.load()
    X, V, U, T, O, W, F = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000, 0x70000000
    ARG, UNS, WS = -1, -2, -4
    inf, nan = float('inf'), float('nan')

    def traj(x=X, v=V, u=U, B=4, L=8, nstep=2, integ=0, tab=T, G=2, nb=11, qmax=2.0, wall=1.0, path=1, out=O, ws=None, nbytes=0):
        return lib.fthmc_meta_trajectory(x, v, u, B, L, 2.0, 0.1, nstep, integ, tab, G, nb, qmax, wall, path, out, None, None, None, None,
                                         None, None, ws, nbytes, None)

    def dep(qm=X, B=4, G=2, nb=11, qmax=2.0, w=0.1, tab=T):
        return lib.fthmc_meta_deposit(qm, B, G, nb, qmax, w, tab, None)

    def frc(x=X, B=4, L=8, tab=T, G=2, nb=11, qmax=2.0, wall=1.0, out=F):
        return lib.fthmc_meta_force(x, B, L, 2.0, tab, G, nb, qmax, wall, out, None)

    def act(x=X, B=4, L=8, tab=T, G=2, nb=11, qmax=2.0, wall=1.0):
        return lib.fthmc_meta_action(x, B, L, 2.0, tab, G, nb, qmax, wall, O, None, None, None)
    for f in (traj, frc, act):
        assert f(x=None) == ARG and f(tab=None) == ARG
        for B in (0, -1, 4194304):
            assert f(B=B) == ARG
        for L in (0, 2, 6, 10, -8, 32768):
            assert f(L=L) == ARG
        for wall in (-1.0, -1e-300, inf, nan):
            assert f(wall=wall) == ARG
    assert traj(v=None) == ARG and traj(u=None) == ARG and traj(out=None) == ARG and frc(out=None) == ARG
    assert dep(qm=None) == ARG and dep(tab=None) == ARG and dep(B=0) == ARG and dep(B=4194304) == ARG
    for w in (-1.0, inf, nan):
        assert dep(w=w) == ARG
    for f in (traj, dep, frc, act):
        for G in (0, -1, 3, 8):                                           # B % G
            assert f(G=G) == ARG
        for nb in (1, 0, -5, 65537):
            assert f(nb=nb) == ARG
        for qmax in (0.0, -1.0, inf, -inf, nan):
            assert f(qmax=qmax) == ARG
    for n in (0, -1):
        assert traj(nstep=n) == ARG
    for p in (-1, 3, 255):
        assert traj(path=p) == ARG
    assert traj(L=68, path=1) == ARG and traj(out=X, path=1) == ARG       # what the one-launch path does not serve
    assert traj(integ=3) == UNS and traj(integ=-1) == UNS and traj(integ=3, nstep=0) == ARG     # the arguments come first
    # (every call here is refused before a launch: the legal edges -- nb = 2 and 65536, G = 1 and B, wall = 0, w = 0 -- are walked by
    # tests/hip/meta_walk.cpp against the build that launches nothing)
    # the workspace: none for the one-launch path; the sequenced path's otherwise (path 0 may take it)
    wsb = lib.fthmc_meta_ws_bytes
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
        ops.meta_force(x, 2.0, torch.zeros(1, 5, dtype=torch.float64), 2.0)          # CPU tensors: there is no CPU fallback
    with pytest.raises(FthmcError):
        ops.meta_deposit(torch.zeros(2, dtype=torch.float64), torch.zeros(1, 5, dtype=torch.float64), 2.0, 0.1)


# ---------------------------------------------------------------- the twin
@pytest.mark.parametrize('L,amp,beta', [(4, math.pi, 2.0), (8, 0.3, 6.0), (12, math.pi, 6.0)])
def test_twin_force_is_the_gradient_of_its_biased_action(L, amp, beta):
    """central differences of S_b in long double on a smooth table (V = a q^2 sampled finely: the interpolant's slope is continuous to
    O(delta)), inside and on the wall; 1e-6 relative to the largest force"""
    B = 2
    a = 0.7
    nb, qmax = 4001, 3.0
    q = -qmax + np.arange(nb) * (2 * qmax / (nb - 1))
    tab = MC.Table(a * q * q, qmax, 2 * a)                               # the wall continues the parabola's curvature
    x = MC.links(B, L, 300 + L, amp)
    F, margin = MC.force(x, beta, tab, LD)
    assert margin.min() > 1e-4                                           # no lookup next to a node: the differences stay on one segment
    h = LD(1e-5)
    rng = np.random.default_rng(L)
    worst = 0.0
    for _ in range(24):
        b, mu, i, j = rng.integers(B), rng.integers(2), rng.integers(L), rng.integers(L)
        xp, xm = x.astype(LD), x.astype(LD)
        xp[b, mu, i, j] += h; xm[b, mu, i, j] -= h
        d = (MC.biased_action(xp, beta, tab, LD)[0][b] - MC.biased_action(xm, beta, tab, LD)[0][b]) / (2 * h)
        worst = max(worst, float(abs(d - F[b, mu, i, j])))
    scale = float(np.abs(F).max())
    print(f'L {L}: |central difference - force| max {worst:.2e}, force scale {scale:.2e}')
    assert worst <= 1e-6 * scale


def test_float64_twin_against_the_long_double_twin_and_no_chain_is_left_out():
    """the rounding figures of the float64 arithmetic on the committed cases (the GPU tests' bounds are the project's figures for the
    plain kernels, or 8x these where a table needs more), and the cap: no chain of any case is left out"""
    worst = {'force': 0.0, 'S': 0.0, 'x_new': 0.0, 'dH': 0.0, 'H1': 0.0}
    by_table = {}
    for c in MC.CASES:
        B, L, amp, beta, nstep, integ, tk, G = c
        x, v, u, tab, ref = MC.case(c)
        assert not ref['left_out'].any(), (MC.case_id(c), ref['t_margin'], ref['u_margin'])
        r64 = MC.trajectory(x, v, u, beta, MC.DT, nstep, integ, tab, dt=np.float64)
        assert np.array_equal(r64['acc'], ref['acc']) and not r64['left_out'].any(), MC.case_id(c)
        F64, FLD = MC.force(x, beta, tab, np.float64)[0], MC.force(x, beta, tab, LD)[0]
        S64, SLD = MC.biased_action(x, beta, tab, np.float64)[0], MC.biased_action(x, beta, tab, LD)[0]
        fig = {'force': MC.rel_err(F64, FLD), 'S': float(np.abs((S64.astype(LD) - SLD) / SLD).max()),
               'x_new': float(np.abs(r64['x_new'].astype(LD) - ref['x_new']).max()),
               'dH': float(np.abs(r64['dH'].astype(LD) - ref['dH']).max()),
               'H1': float(np.abs((r64['H1'].astype(LD) - ref['H1']) / ref['H1']).max())}
        for k, val in fig.items():
            worst[k] = max(worst[k], val)
            row = by_table.setdefault(tk, dict.fromkeys(fig, 0.0))
            row[k] = max(row[k], val)
    print('float64 twin vs long double twin, worst over the cases:', {k: f'{val:.2e}' for k, val in worst.items()})
    for tk, fig in by_table.items():
        print(f'  {tk}:', {k: f'{val:.2e}' for k, val in fig.items()})
    # far inside the project's figures for the plain kernels: the 8x rule never widens a bound on these cases
    assert 8 * worst['force'] <= 1e-11 and 8 * worst['S'] <= 1e-10 and 8 * worst['x_new'] <= 1e-9 and 8 * worst['H1'] <= 1e-8
    assert 8 * worst['dH'] <= 1.0


def test_cases_cover_what_they_claim():
    seen = {k: set() for k in ('shape', 'amp', 'beta', 'nstep', 'integ', 'table', 'G1')}
    for B, L, amp, beta, nstep, integ, tk, G in MC.CASES:
        for k, val in zip(seen, ((B, L), amp, beta, nstep, integ, tk, G == 1)):
            seen[k].add(val)
        seen.setdefault(('table', tk), set()).update({('amp', amp), ('beta', beta), ('nstep', nstep), ('integ', integ)})
    assert seen['shape'] == set(MC.SHAPES) and seen['amp'] == set(MC.AMPS) and seen['beta'] == set(MC.BETAS)
    assert seen['nstep'] == set(MC.NSTEPS) and seen['integ'] == set(MC.INTEGRATORS) and seen['table'] == set(MC.TABLES) and seen['G1'] == {True, False}
    for tk in MC.TABLES:
        assert len(seen[('table', tk)]) == 2 + 2 + 2 + 3, tk                # every table meets every value of every axis
        # ... and every shape, with one shared row and with one row per chain
        assert {(B, L, G) for B, L, a, b, n, i, t, G in MC.CASES if t == tk} == {(B, L, G) for B, L in MC.SHAPES for G in (1, B)}, tk
    assert len(MC.CASES) == len(set(MC.CASES)) == 3 * (2 * len(MC.SHAPES) - 1)
    # the rough table puts chains on the wall and inside
    out = ins = 0
    for c in MC.CASES:
        if c[6] == 'rough':
            x, v, u, tab, ref = MC.case(c)
            q = MC.f64(MC.charge_m(x, LD))
            out += int((np.abs(q) > tab.qmax).sum()); ins += int((np.abs(q) < tab.qmax).sum())
    assert out >= 4 and ins >= 4, (out, ins)


# ---------------------------------------------------------------- deposit
def test_deposit_two_node_split_range_and_chain_order():
    tab = MC.Table(np.zeros((2, 11)), 2.0, 0.0)                          # delta = 0.4
    w = 0.25
    tab.deposit(np.array([0.1, 5.0, -2.0, 1.9]), w)                      # row 0: chains 0, 1; row 1: chains 2, 3
    f = (0.1 + 2.0) / 0.4 - 5
    assert np.flatnonzero(tab.V[0]).tolist() == [5, 6] and abs(tab.V[0, 5] - w * (1 - f)) < 1e-15 and abs(tab.V[0, 6] - w * f) < 1e-15
    assert abs(tab.V[0].sum() - w) < 1e-15                               # q = 5 is outside: nothing
    assert tab.V[1, 0] == w and abs(tab.V[1, 9] + tab.V[1, 10] - w) < 1e-15 and tab.V[1, 1:9].sum() == 0      # q = -qmax: all on node 0
    t2 = MC.Table(np.zeros((1, 11)), 2.0, 0.0).deposit(np.array([2.0, -2.0000001, np.nan, 2.5]), w)
    assert not t2.V.any()                                                # q = +qmax, beyond either end, NaN: outside
    # chain order: three hills on node 0 (q = -qmax: f = 0 exactly), one of 1 and two of half an ulp of 1 -- 1 first swallows both, 1 last
    # sees their sum
    h = 2.0 ** -53
    a, b = MC.Table(np.zeros((1, 11)), 2.0, 0.0), MC.Table(np.zeros((1, 11)), 2.0, 0.0)
    for wk in (1.0, h, h):
        a.deposit(np.array([-2.0]), wk)
    for wk in (h, h, 1.0):
        b.deposit(np.array([-2.0]), wk)
    assert a.V[0, 0] == 1.0 and b.V[0, 0] == 1.0 + 2.0 ** -52
    # one call with several walkers equals the walkers one call each, in order
    q = np.random.default_rng(3).uniform(-2.2, 2.2, 257)
    one = MC.Table(np.zeros((1, 81)), 2.0, 0.0).deposit(q, 0.01)
    each = MC.Table(np.zeros((1, 81)), 2.0, 0.0)
    for qq in q:
        each.deposit(np.array([qq]), 0.01)
    assert np.array_equal(one.V, each.V) and abs(one.V.sum() - 0.01 * (np.abs(q) < 2.0).sum()) < 1e-12


def test_meta_potential_value_and_slope_follow_the_definitions():
    from fthmc_amd.meta import MetaPotential
    pot = MetaPotential(11, 2.0, 3.0, groups=2)
    V = np.random.default_rng(8).normal(size=(2, 11))
    pot.load_state_dict({'nb': 11, 'qmax': 2.0, 'wall': 3.0, 'groups': 2, 'table': V})
    assert abs(pot.delta - 0.4) < 1e-16 and np.allclose(pot.nodes, np.linspace(-2, 2, 11), atol=1e-15)
    for g in (0, 1):
        assert np.allclose(pot.value(pot.nodes[:-1], g), V[g, :-1], atol=1e-14)          # the nodes themselves (the last one: below)
        q = np.array([-1.9, -0.3, 0.0, 0.77, 1.999])
        i = np.floor((q + 2.0) / 0.4).astype(int); f = (q + 2.0) / 0.4 - i
        assert np.allclose(pot.value(q, g), V[g, i] + f * (V[g, i + 1] - V[g, i]), atol=1e-14)
        assert np.allclose(pot.slope(q, g), (V[g, i + 1] - V[g, i]) / 0.4, atol=1e-13)
        # the wall, and q = +-qmax: -qmax is node 0 of the table, +qmax lands outside with d = 0
        assert pot.value(2.0, g) == V[g, -1] and pot.slope(2.0, g) == 0.0
        assert pot.value(-2.0, g) == V[g, 0] and abs(pot.slope(-2.0, g) - (V[g, 1] - V[g, 0]) / 0.4) < 1e-13
        assert abs(pot.value(2.5, g) - (V[g, -1] + 0.5 * 3.0 * 0.25)) < 1e-14 and abs(pot.slope(2.5, g) - 1.5) < 1e-14
        assert abs(pot.value(-3.0, g) - (V[g, 0] + 0.5 * 3.0 * 1.0)) < 1e-14 and abs(pot.slope(-3.0, g) + 3.0) < 1e-14
        # the twin's lookup is the same statement
        qq = np.random.default_rng(9).uniform(-3, 3, 64)
        tv, ts, _ = MC.Table(V[g], 2.0, 3.0).lookup(qq, np.float64)
        assert np.array_equal(tv, pot.value(qq, g)) and np.array_equal(ts, pot.slope(qq, g))
    sd = pot.state_dict()
    assert set(sd) == {'nb', 'qmax', 'wall', 'groups', 'table'} and np.array_equal(sd['table'], V)
    other = MetaPotential(11, 1.0, 0.0, groups=2).load_state_dict(sd)
    assert other.qmax == 2.0 and other.wall == 3.0 and np.array_equal(other.numpy(), V)
    with pytest.raises(ValueError):
        MetaPotential(12, 2.0, 3.0).load_state_dict(sd)
    for bad in ((1, 2.0, 0.0), (5, 0.0, 0.0), (5, float('nan'), 0.0), (5, 1.0, -1.0), (65537, 1.0, 0.0)):
        with pytest.raises(ValueError):
            MetaPotential(*bad)


def test_reweighted_mean_on_a_constructed_example():
    from fthmc_amd.utils.observables import reweighted_mean
    o = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]])
    vb = np.array([[0.0, math.log(2.0)], [math.log(3.0), 0.0], [0.0, 0.0]])
    wgt = np.array([[1, 2], [3, 1], [1, 1]], dtype=float)
    mean, err = reweighted_mean(o, vb, n_block=2)
    assert abs(mean - (wgt * o).sum() / wgt.sum()) < 1e-14
    jk = np.array([(wgt[:, 1] * o[:, 1]).sum() / wgt[:, 1].sum(), (wgt[:, 0] * o[:, 0]).sum() / wgt[:, 0].sum()])   # delete chain 0, chain 1
    assert abs(err - math.sqrt(1 * np.mean((jk - jk.mean()) ** 2))) < 1e-14
    # the common maximum is taken out before exponentiating: a shift of the potential changes nothing and nothing overflows
    m2, e2 = reweighted_mean(o, vb + 5000.0, n_block=2)
    assert abs(m2 - mean) < 1e-12 and abs(e2 - err) < 1e-12
    # no bias: the plain mean and the standard error of independent samples
    s = np.random.default_rng(4).normal(size=400)
    m, e = reweighted_mean(s, np.zeros(400), n_block=400)
    assert abs(m - s.mean()) < 1e-14 and abs(e - s.std(ddof=1) / 20.0) < 1e-12
    assert math.isnan(reweighted_mean(s[:1], np.zeros(1))[1])
    with pytest.raises(ValueError):
        reweighted_mean(o, vb[:2])


# ---------------------------------------------------------------- the twin as a sampler
def test_twin_sampler_reproduces_the_exact_charge_moment_by_reweighting():
    """L = 8, beta = 4, 128 chains cold, one shared table (nb = 61, qmax = 3, wall = 50), w = 0.002, 200 build + 400 static leapfrog
    trajectories (tau = 1, 10 steps): the reweighted <Q^2> under the frozen table within |z| <= 4 of the exact 0.4820159295"""
    from fthmc_amd.utils.observables import reweighted_mean
    tab = MC.Table(np.zeros((1, 61)), 3.0, 50.0)
    r = MC.sampler(8, 4.0, 128, tab, 200, 400, 0.002)
    q2, err = reweighted_mean(r['Q'] ** 2, r['vbias'], n_block=128)
    z = (q2 - Q2_EXACT_L8_B4) / err
    print(f'<Q^2> {q2:.4f} +- {err:.4f}, exact {Q2_EXACT_L8_B4:.4f}, z {z:+.2f}; acceptance {r["acc"]:.3f}, mean |dQ| {r["dq"]:.4f}, '
          f'table range {tab.V.max() - tab.V.min():.3f}')
    assert abs(z) <= 4.0
    assert tab.V.max() > 0.5 and r['acc'] > 0.5


# ---------------------------------------------------------------- the entry points under the sanitizers
def test_meta_entry_points_walk_clean_under_asan_and_ubsan(tmp_path):
    """tests/hip/meta_walk.cpp: a stand-alone program against the host-side sanitizer build of the library (launches are no-ops
    there), built with -fsanitize=address,undefined by the recipe next to `make san`'s: the five entry points through their refusals,
    the workspace rule, legal calls on both paths up to the largest shapes.  Its own process, nothing preloaded."""
    csrc = os.path.join(ROOT, 'fthmc_amd', 'csrc')
    exe = str(tmp_path / 'meta_walk')
    r = subprocess.run(['make', '-C', csrc, '-f', 'san.mk', 'san_meta', 'SANMETA=' + exe], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and os.path.exists(exe), r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ)
    env.update(ASAN_OPTIONS='detect_leaks=1:abort_on_error=1:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert 'ERROR: AddressSanitizer' not in r.stderr and 'runtime error:' not in r.stderr, r.stderr[-6000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out['calls'] > 300 and out['refusals'] >= 80
