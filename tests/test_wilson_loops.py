"""CPU-only tests of the Wilson-loop observable: the C ABI declares and exports the entry points and the wrappers, the operator
schema and the `fthmc` alias exist; the numpy oracle of tests/wilson_loop_cases.py against an independent path walk and against
what it must give; the float64 twin of the device algorithm inside the derived error bound; the exact finite-volume formula of
fthmc_amd/utils/observables.py against mpmath; the entry points as a stand-alone program under AddressSanitizer + UBSan."""
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

import tempering_cases as TC
import wilson_loop_cases as WC
from oracle import ref_cpu as R

NEW = ('fthmc_wilson_loops_ws_bytes', 'fthmc_wilson_loops')


def test_header_library_wrappers_schema_and_alias_carry_the_new_entry_points():
    import ctypes
    import inspect
    from fthmc_amd import _lib, ops
    import fthmc_amd.torch_ops as TO
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'fthmc_hip.h')).read()
    declared = set(re.findall(r'\b(fthmc_[a-z0-9_]+)\s*\(', header))
    for name in NEW:
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES['fthmc_wilson_loops_ws_bytes'] == [ctypes.c_int] * 4
    assert lib.fthmc_wilson_loops_ws_bytes.restype is ctypes.c_size_t
    assert len(_lib.SIGNATURES['fthmc_wilson_loops']) == 10
    assert int(lib.fthmc_wilson_loops_ws_bytes(2, 8, 8, 8)) > 0 and int(lib.fthmc_wilson_loops_ws_bytes(2, 8, 9, 8)) == 0
    assert callable(ops.wilson_loops) and list(inspect.signature(ops.wilson_loops).parameters) == ['x', 'Rmax', 'Tmax', 'out', 'mean_out']
    schema = str(torch.ops.fthmc_hip.wilson_loops.default._schema)
    assert 'Tensor x, int Rmax, int Tmax' in schema and schema.endswith('-> Tensor'), schema
    assert 'wilson_loops' in TO.__all__
    y = torch.ops.fthmc_hip.wilson_loops(torch.empty(3, 2, 8, 8, dtype=torch.float64, device='meta'), 5, 7)   # the fake-shape function
    assert tuple(y.shape) == (3, 5, 7)
    import fthmc.utils.qed_helpers as q1
    import fthmc_amd.utils.qed_helpers as q2
    import fthmc.utils.observables as o1
    import fthmc_amd.utils.observables as o2
    assert q1 is q2 and callable(q1.wilson_loops) and callable(q1.polyakov_correlator)
    assert o1 is o2 and all(callable(getattr(o1, n)) for n in ('exact_wilson_loop', 'string_tension_exact', 'creutz_ratios', 'loop_table'))
    from fthmc.ft_hmc import FieldTransformation
    from fthmc.hmc import run_hmc
    for fn in (FieldTransformation.run, run_hmc):
        p = inspect.signature(fn).parameters
        assert p['loops'].default is None and p['loops_every'].default == 1


def test_operator_and_wrapper_refuse_cpu_tensors_and_bad_tables():
    from fthmc_amd import ops
    from fthmc_amd._lib import FthmcError
    import fthmc_amd.torch_ops  # noqa: F401
    x = torch.zeros(2, 2, 8, 8, dtype=torch.float64)
    with pytest.raises(NotImplementedError):
        torch.ops.fthmc_hip.wilson_loops(x, 2, 2)
    with pytest.raises(FthmcError):
        ops.wilson_loops(x, 2)
    from fthmc_amd.ft_hmc import FieldTransformation
    for bad in ((0, 2), (2, 9), (9, 1)):
        with pytest.raises(ValueError):
            FieldTransformation._loops_arg(bad, 8)
    assert FieldTransformation._loops_arg(None, 8) is None and FieldTransformation._loops_arg(3, 8) == (3, 3)


# ---------------------------------------------------------------- the oracle
@pytest.mark.parametrize('L', [4, 5, 8])
def test_oracle_against_a_link_by_link_path_walk(L):
    x = WC.uniform_links(1, L, 100 + L)
    a, b = WC.loops_ref(x, L, L), WC.loops_walk(x, L, L)
    assert float(np.abs(a - b).max()) < 1e-17 * 2 * L * 8          # longdouble: 4 L additions of angles <= pi, 2^-64 each


def test_oracle_plaquette_gauge_invariance_unit_and_known_answer():
    rng = np.random.default_rng(11)
    for L in (4, 8, 12):
        x = WC.uniform_links(3, L, L)
        W = WC.loops_ref(x, L, L)
        P = R.plaq(torch.from_numpy(x)).numpy()                    # the oracle's plaquettes
        assert float(np.abs(W[:, 0, 0] - np.cos(P).reshape(3, -1).mean(axis=1)).max()) < 1e-15
        alpha = rng.uniform(-50, 50, (3, L, L))
        Wg = WC.loops_ref(WC.gauge_transform(x, alpha), L, L)
        assert float(np.abs(Wg - W).max()) < 1e-13                 # the transformed links are rounded to doubles of size ~100
        assert np.all(WC.loops_ref(np.zeros((2, 2, L, L)), L, L) == 1)
        assert float(np.abs(W[:, L - 1, L - 1] - 1).max()) < 1e-15     # W(L, L) = 1: every link appears twice with opposite signs
        assert float(np.abs(W[:, :, L - 1] - WC.polyakov_correlator_ref(x, L)).max()) < 1e-15
    for L in (8, 12):
        for k in (1, 3):
            W = WC.loops_ref(WC.known_answer_field(L, k), L, L)[0]
            assert float(np.abs(W - WC.known_answer(L, k, L, L)).max()) < 1e-14 * k * L


@pytest.mark.parametrize('shape', WC.SHAPES, ids=lambda s: 'B%d-L%d-R%d-T%d' % s)
def test_float64_twin_of_the_device_algorithm_stays_inside_the_derived_bound(shape):
    B, L, Rmax, Tmax = shape
    B = min(B, 3)
    x = WC.uniform_links(B, L, 7 * L + Rmax)
    tol = WC.tolerance(L, Rmax, Tmax, WC.mu_of(x))
    err = np.abs(WC.loops_twin64(x, Rmax, Tmax) - WC.loops_ref(x, Rmax, Tmax)).astype(np.float64)
    print('twin |err| / tol max', float((err.max(axis=0) / tol).max()))
    assert np.all(err <= tol[None]), float((err.max(axis=0) / tol).max())


def test_float64_twin_on_the_hard_fields():
    """a gauge transformation of amplitude 50 (links of magnitude ~100: the bound at the transformed field's max|x|), the
    known-answer field, and the worst case for the prefix sums: every link near +pi"""
    rng = np.random.default_rng(5)
    for L in (8, 12, 64):
        Rm, Tm = min(L, 9), min(L, 9)
        x = WC.gauge_transform(WC.uniform_links(2, L, L + 1), rng.uniform(-50, 50, (2, L, L)))
        for f in (x, WC.known_answer_field(L, 3), np.full((1, 2, L, L), 3.14159)):
            tol = WC.tolerance(L, Rm, Tm, WC.mu_of(f))
            err = np.abs(WC.loops_twin64(f, Rm, Tm) - WC.loops_ref(f, Rm, Tm)).astype(np.float64)
            assert np.all(err <= tol[None]), (L, float((err.max(axis=0) / tol).max()))
    assert np.all(WC.loops_twin64(np.zeros((2, 2, 8, 8)), 8, 8) == 1.0)


def test_derived_bound_lies_below_the_ceiling_on_every_gpu_shape():
    for B, L, Rmax, Tmax in WC.SHAPES + ((1, 1028, 2, 3),):
        for mu in (1.0, 6.0, 33.0):
            WC.tolerance(L, Rmax, Tmax, mu)                        # asserts it
    assert WC.issue_bound(64, 1, 1, 1.0) < 2.9e-12 and WC.derived_bound(64, 64, 64, 1.0) < 4.5e-13


# ---------------------------------------------------------------- the exact formula
def _mp_exact(beta, V, A):
    import mpmath as mp
    mp.mp.dps = 30
    b = mp.mpf(beta)
    I = {n: mp.besseli(n, b) for n in range(-61, 62)}
    return mp.fsum(I[n] ** (V - A) * I[n + 1] ** A for n in range(-60, 61)) / mp.fsum(I[n] ** V for n in range(-60, 61))


@pytest.mark.parametrize('beta,L', [(2.0, 8), (4.0, 16), (6.0, 64)])
def test_exact_formula_against_mpmath(beta, L):
    from fthmc_amd.utils import observables as O
    V = L * L
    for Rr, T in ((1, 1), (1, 2), (2, 3), (1, L), (L // 2, L // 2), (L // 2, L), (L - 1, L), (L, L - 1)):     # A = V / 2 among them
        want = _mp_exact(beta, V, Rr * T)
        got = O.exact_wilson_loop(beta, L, Rr, T)
        assert abs(got - float(want)) <= 1e-10 * float(want), (Rr, T, got, float(want))
    # areas that are no R x T product on this lattice (A = V - 1 among them): the same formula as a function of the area
    for A in (V - 1, V - 2, V // 2 + 1, 7, 0):
        want = _mp_exact(beta, V, A)
        got = O.exact_loop_of_area(beta, V, A)
        assert abs(got - float(want)) <= 1e-10 * float(want), (A, got, float(want))


def test_exact_formula_plaquette_symmetry_unit_and_creutz_ratios():
    from fthmc_amd.utils import observables as O
    for beta, L in ((0.5, 4), (2.0, 8), (3.5, 12), (6.0, 16)):
        assert abs(O.exact_wilson_loop(beta, L, 1, 1) - TC.exact_plaquette(beta, L * L)) < 1e-13
        assert abs(O.exact_wilson_loop(beta, L, L, L) - 1.0) < 1e-14
        for Rr, T, R2, T2 in ((1, L, L - 1, L), (2, L // 2, L, L - 1), (L // 2, L, L // 2, L)):      # areas A and V - A
            assert Rr * T + R2 * T2 == L * L
            a, b = O.exact_wilson_loop(beta, L, Rr, T), O.exact_wilson_loop(beta, L, R2, T2)
            assert abs(a - b) <= 1e-12 * a, (beta, L, Rr, T)
        with pytest.raises(ValueError):
            O.exact_wilson_loop(beta, L, L + 1, 1)
    import mpmath as mp
    for beta in (0.7, 2.0, 6.0):
        sigma = O.string_tension_exact(beta)
        assert abs(sigma + float(mp.log(mp.besseli(1, beta) / mp.besseli(0, beta)))) < 1e-14
        Rg, Tg = np.arange(1, 7)[:, None], np.arange(1, 6)[None, :]
        chi = O.creutz_ratios(np.exp(-sigma * Rg * Tg))          # the exact infinite-volume table: an area law
        assert chi.shape == (5, 4) and float(np.abs(chi - sigma).max()) < 1e-12


def test_loop_table_is_the_blocked_mean():
    from fthmc_amd.utils import observables as O
    rng = np.random.default_rng(2)
    s = rng.normal(0.5, 0.1, (64, 3, 4))
    mean, err = O.loop_table(s, n_block=16)
    bm = s.reshape(16, 4, 3, 4).mean(axis=1)
    assert np.allclose(mean, bm.mean(axis=0), rtol=0, atol=1e-15) and np.allclose(err, bm.std(axis=0) / np.sqrt(15), rtol=1e-12)
    m2, e2 = O.loop_table([torch.from_numpy(t) for t in s], n_block=16)
    assert np.array_equal(m2, mean) and np.array_equal(e2, err)
    m3, _ = O.loop_table(np.stack([s, s], axis=1), n_block=16)   # [n, chains, R, T]: chains averaged
    assert np.allclose(m3, mean, rtol=0, atol=1e-15)


# ---------------------------------------------------------------- the entry points under the sanitizers
def test_loop_entry_points_walk_clean_under_asan_and_ubsan(tmp_path):
    """tests/hip/loops_walk.cpp: a stand-alone program against the host-side sanitizer build of the library (launches are no-ops
    there), built with -fsanitize=address,undefined by the recipe next to `make san`'s: every refusal, the smallest refused shapes,
    legal sizes up to B = 2^20 and L = FTHMC_MAX_L, workspace sizes monotone.  Its own process, nothing preloaded."""
    csrc = os.path.join(ROOT, 'fthmc_amd', 'csrc')
    exe = str(tmp_path / 'loops_walk')
    r = subprocess.run(['make', '-C', csrc, '-f', 'san.mk', 'san_loops', 'SANLOOPS=' + exe], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and os.path.exists(exe), r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ)
    env.update(ASAN_OPTIONS='detect_leaks=1:abort_on_error=1:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert 'ERROR: AddressSanitizer' not in r.stderr and 'runtime error:' not in r.stderr, r.stderr[-6000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out['calls'] > 900 and out['refusals'] > 500
