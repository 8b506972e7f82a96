"""CPU-only tests of the local-update sampler (heatbath / overrelaxation): the C ABI declares and exports the entry point and the
wrappers, the operator schema and the `fthmc` alias exist, the refusals refuse; the numpy twin of tests/local_update_cases.py keeps
the action under overrelaxation, draws von Mises numbers, samples 2D U(1) to the exact finite-volume loops, and stays inside its own
derived bound when run in float64; the entry point's host side as a stand-alone program under AddressSanitizer + UBSan."""
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

import local_update_cases as LC
import wilson_loop_cases as WC


def test_header_library_wrappers_schema_and_alias_carry_the_new_entry_point():
    import ctypes
    from fthmc_amd import _lib, ops
    import fthmc_amd.torch_ops as TO
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'fthmc_hip.h')).read()
    declared = set(re.findall(r'\b(fthmc_[a-z0-9_]+)\s*\(', header))
    assert 'fthmc_local_update' in declared and hasattr(lib, 'fthmc_local_update') and 'fthmc_local_update' in _lib.SIGNATURES
    sig = _lib.SIGNATURES['fthmc_local_update']
    assert len(sig) == 13 and sig[3] is ctypes.c_double and sig[9] is ctypes.c_int64
    assert list(inspect.signature(ops.local_update).parameters) == ['x', 'beta', 'seeds', 'n_hb', 'n_or', 'nsweep', 'sweep0', 'classes', 'out']
    p = inspect.signature(ops.local_update).parameters
    assert (p['n_hb'].default, p['n_or'].default, p['nsweep'].default, p['sweep0'].default, p['classes'].default) == (1, 0, 1, 0, 0xF)
    schema = str(torch.ops.fthmc_hip.local_update.default._schema)
    assert schema.startswith('fthmc_hip::local_update(Tensor x, float beta, Tensor? beta_b, Tensor? seeds') and schema.endswith('-> Tensor'), schema
    assert 'local_update' in TO.__all__
    y = torch.ops.fthmc_hip.local_update(torch.empty(3, 2, 8, 8, dtype=torch.float64, device='meta'), 2.0, None, None, 0, 1)
    assert tuple(y.shape) == (3, 2, 8, 8)
    import fthmc.local as l1
    import fthmc_amd.local as l2
    import fthmc.utils.qed_helpers as q1
    assert l1 is l2 and callable(l1.run_local) and callable(q1.heatbath) and callable(q1.overrelax)
    p = inspect.signature(l1.run_local).parameters
    assert list(p)[:6] == ['param', 'x', 'n_overrelax', 'sweeps_per_traj', 'loops', 'loops_every']
    assert (p['x'].default, p['n_overrelax'].default, p['sweeps_per_traj'].default, p['loops'].default, p['loops_every'].default) == (None, 0, 1, None, 1)
    from fthmc.hmc import run_hmc
    assert inspect.signature(run_hmc).parameters['overrelax'].default == 0
    assert inspect.signature(q1.overrelax).parameters['n'].default == 1 and inspect.signature(q1.heatbath).parameters['seeds'].default is None


def test_refusals_refuse():
    """the argument checks of the C entry point come before anything touches the device: stand-in addresses are never read"""
    from fthmc_amd import _lib, ops
    from fthmc_amd._lib import FthmcError
    lib = _lib.load()
    X, S, O = 0x10000000, 0x20000000, 0x30000000

    def call(x=X, B=2, L=8, beta=2.0, bb=None, seeds=S, n_hb=1, n_or=1, nsweep=1, sweep0=0, classes=15, out=O):
        return lib.fthmc_local_update(x, B, L, beta, bb, seeds, n_hb, n_or, nsweep, sweep0, classes, out, None)
    ARG = -1
    assert call(x=None) == ARG and call(out=None) == ARG and call(seeds=None) == ARG
    for B in (0, -1, 4194304):
        assert call(B=B) == ARG
    for L in (0, 2, 6, 10, -8, 32768):
        assert call(L=L) == ARG
    assert call(n_hb=-1) == ARG and call(n_or=-1) == ARG and call(nsweep=-1) == ARG and call(sweep0=-1) == ARG
    for c in (0, 16, -1, 255):
        assert call(classes=c) == ARG
    # the heatbath-sweep index is one 32-bit counter word: sweep0 + nsweep n_hb <= 2^32
    assert call(sweep0=2 ** 32, n_hb=1, nsweep=1) == ARG and call(sweep0=2 ** 32 - 1, n_hb=1, nsweep=2) == ARG
    assert call(sweep0=0, n_hb=65536, nsweep=65537) == ARG and call(sweep0=2 ** 40) == ARG
    assert call(sweep0=5, n_hb=2 ** 31 - 1, nsweep=2 ** 31 - 1) == ARG
    x = torch.zeros(2, 2, 8, 8, dtype=torch.float64)
    with pytest.raises(FthmcError):
        ops.local_update(x, 2.0, None, n_hb=0, n_or=1)                   # a CPU tensor: there is no CPU fallback
    import fthmc_amd.torch_ops  # noqa: F401
    with pytest.raises(NotImplementedError):
        torch.ops.fthmc_hip.local_update(x, 2.0, None, None, 0, 1)


# ---------------------------------------------------------------- the twin: overrelaxation
@pytest.mark.parametrize('L,amp', [(4, math.pi), (8, math.pi), (12, 50.0)])
def test_twin_overrelaxation_conserves_the_action_and_is_an_involution(L, amp):
    x = LC.uniform_links(3, L, 40 + L, amp)
    s0 = LC.action_sum(x)
    for mu, p in LC.CLASSES:
        r = LC.class_update(x, mu, p, 'or', 2.0)
        y = r['x']
        # the class's links move by their bound each; a link sits in two plaquettes, |d cos| <= |d angle|
        tol = 2.0 * r['bound'].sum(axis=1)
        assert np.all(np.abs((LC.action_sum(y) - s0).astype(np.float64)) <= tol), (mu, p)
        assert np.all(r['margin'] == np.inf) and np.all(r['attempts'] == 0)
        y64 = y.astype(np.float64)
        r2 = LC.class_update(y64, mu, p, 'or', 2.0)
        back = LC.circ_dist(r2['new'], LC.regularize(x[:, mu, r['ii'], r['jj']].astype(LC.LD)))
        assert np.all(back <= r['bound'] + r2['bound'] + 2.0 ** -52 * math.pi), (mu, p, float(back.max()))
        other = np.ones((2, L, L), dtype=bool); other[mu, r['ii'], r['jj']] = False
        assert np.array_equal(y64[:, other], x[:, other])


# ---------------------------------------------------------------- the twin: the von Mises draw
@pytest.mark.parametrize('kappa', [0.0, 1e-8, 1e-3, 0.5, 2.0, 12.0])
def test_twin_heatbath_draws_von_mises_numbers(kappa):
    B, n = 64, 2048
    d = LC.vonmises_draw(np.full((B, n), kappa), np.zeros((B, n)), LC.chain_seeds(B, 17), np.arange(n), 1, 7)
    th = d['theta'].astype(np.float64)
    assert np.all(d['accepted']) and np.all(np.isfinite(th)) and np.all(np.abs(th) <= math.pi)
    assert 1 <= int(d['attempts'].min()) and int(d['attempts'].max()) <= LC.MAX_ATTEMPTS
    c = np.cos(th)
    se = c.std(ddof=1) / math.sqrt(c.size)
    z = (c.mean() - LC.bessel_ratio(kappa)) / se
    print(f'kappa {kappa}: <cos> {c.mean():.6f} exact {LC.bessel_ratio(kappa):.6f} z {z:+.2f}, attempts mean {d["attempts"].mean():.3f} max {d["attempts"].max()}')
    assert abs(z) <= 4.5
    assert abs(np.sin(th).mean()) <= 4.5 * np.sin(th).std(ddof=1) / math.sqrt(c.size)          # both signs of the angle


def test_twin_heatbath_is_finite_on_the_cancelling_staple_pair_and_at_large_kappa():
    L = 8
    x = np.zeros((1, 2, L, L))
    x[0, 1, 3, 0::2] = math.pi                     # x0[2][j]: (a, b) = (pi, 0) for even j, (0, pi) for odd j: cos((a + b) / 2) = 6e-17
    seeds = LC.chain_seeds(1, 3)
    for mu, p in LC.CLASSES:
        for kind in ('hb', 'or'):
            r = LC.class_update(x, mu, p, kind, 2.0, seeds, 0)
            new = r['new'].astype(np.float64)
            assert np.all(np.isfinite(new)) and np.all(new >= -math.pi) and np.all(new < math.pi)
    r = LC.class_update(x, 0, 0, 'hb', 2.0, seeds, 0)
    assert r['kappa'].min() < 1e-15 and r['ambiguous'].any()
    d = LC.vonmises_draw(np.full((2, 512), 1e9), np.zeros((2, 512)), LC.chain_seeds(2, 4), np.arange(512), 0, 0, dt=np.float64)
    assert np.all(np.isfinite(d['theta'][d['accepted']])) and int(d['attempts'].max()) <= LC.MAX_ATTEMPTS


# ---------------------------------------------------------------- the twin inside its own bound
@pytest.mark.parametrize('B,L,amp', LC.CASES, ids=lambda v: str(int(v)))
def test_float64_twin_stays_inside_the_derived_bound_and_no_chain_is_left_out(B, L, amp):
    """the bound is derived for fp64 arithmetic: the same formulas in float64 numpy must land inside it; and on the fields and seeds
    the device tests use (LC.case), no accept decision comes closer than MARGIN_MIN and no link is ambiguous: nothing is left out"""
    for kind in ('or', 'hb'):
        x, seeds, twin = LC.case(B, L, kind, amp)
        for k, (mu, p) in enumerate(LC.CLASSES):
            a = twin[k]
            b = LC.class_update(x, mu, p, kind, LC.BETA, seeds, LC.SWEEP, dt=np.float64)
            assert np.array_equal(a['attempts'], b['attempts']) and int(a['attempts'].max()) <= LC.MAX_ATTEMPTS
            assert float(a['margin'].min()) >= LC.MARGIN_MIN and not a['ambiguous'].any()
            ratio = LC.circ_dist(a['new'], b['new']) / a['bound']
            assert float(ratio.max()) <= 1.0, (kind, mu, p, float(ratio.max()))
            assert float(np.median(a['bound'])) < 1e-12                 # a bound that still sees an index error


# ---------------------------------------------------------------- the twin as a sampler
@pytest.mark.parametrize('n_or', [0, 2])
def test_twin_sampler_reproduces_the_exact_small_loops(n_or):
    from fthmc_amd.utils import observables as O
    B, L, beta, ntherm, nmeas = 96, 8, 2.0, 40, 160
    x = LC.uniform_links(B, L, 77)
    seeds = LC.chain_seeds(B, 78 + n_or)
    acc = np.zeros((B, 4, 4))
    for k in range(ntherm + nmeas):
        x = LC.sweep(x, beta, seeds, k, n_or=n_or)
        if k >= ntherm:
            acc += WC.loops_ref(x, 4, 4).astype(np.float64)
    chain = acc / nmeas
    mean, se = chain.mean(axis=0), chain.std(axis=0, ddof=1) / math.sqrt(B)
    for R in range(1, 5):
        for T in range(1, 5):
            if R * T <= 4:
                z = (mean[R - 1, T - 1] - O.exact_wilson_loop(beta, L, R, T)) / se[R - 1, T - 1]
                print(f'n_or {n_or} W({R},{T}) {mean[R - 1, T - 1]:.5f} exact {O.exact_wilson_loop(beta, L, R, T):.5f} z {z:+.2f}')
                assert abs(z) <= 4.5, (R, T, z)


# ---------------------------------------------------------------- the entry point under the sanitizers
def test_local_update_entry_point_walks_clean_under_asan_and_ubsan(tmp_path):
    """tests/hip/local_walk.cpp: a stand-alone program against the host-side sanitizer build of the library (launches are no-ops
    there), built with -fsanitize=address,undefined by the recipe next to `make san`'s: every refusal, the counter arithmetic at its
    edges, and legal calls on both paths up to the largest shapes (the host code's geometry and loops; the order of the launches is
    the device tests' to see).  Its own process, nothing preloaded."""
    csrc = os.path.join(ROOT, 'fthmc_amd', 'csrc')
    exe = str(tmp_path / 'local_walk')
    r = subprocess.run(['make', '-C', csrc, '-f', 'san.mk', 'san_local', 'SANLOCAL=' + exe], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and os.path.exists(exe), r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ)
    env.update(ASAN_OPTIONS='detect_leaks=1:abort_on_error=1:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert 'ERROR: AddressSanitizer' not in r.stderr and 'runtime error:' not in r.stderr, r.stderr[-6000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out['calls'] > 400 and out['refusals'] >= 90
