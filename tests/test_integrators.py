"""CPU-only tests of the MD integrators (leapfrog, Omelyan 2MN, 4th-order force-gradient): the C ABI declares and exports the new
entry points, the schedule the library states (csrc/integrator.h through fthmc_integrator_schedule) against the one written out in
tests/integrator_cases.py, the Python keywords, the reference integrators themselves (order, reversibility, leapfrog bit for bit)
and the schedule header as a stand-alone program under AddressSanitizer + UBSan."""
import ctypes
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

import integrator_cases as IC
from oracle import ref_cpu as R

NEW = ('fthmc_integrator_forces', 'fthmc_integrator_schedule', 'fthmc_md', 'fthmc_hmc_trajectory_int', 'fthmc_ft_md_v',
       'fthmc_ft_trajectory_int_v')


def test_header_library_and_signatures_carry_the_integrator_entry_points():
    from fthmc_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'fthmc_hip.h')).read()
    declared = set(re.findall(r'\b(fthmc_[a-z0-9_]+)\s*\(', header))
    for name in NEW:
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    for macro, val in (('FTHMC_INT_LEAPFROG', 0), ('FTHMC_INT_OMELYAN', 1), ('FTHMC_INT_FORCE_GRADIENT', 2)):
        assert re.search(r'#define\s+%s\s+%d\b' % (macro, val), header), macro
    assert _lib.INTEGRATORS == IC.CODES
    S = _lib.SIGNATURES
    # the twins take their originals' arguments plus the integrator (the flowed ones: before the weight version, which stays last)
    assert len(S['fthmc_md']) == len(S['fthmc_leapfrog']) + 1 and len(S['fthmc_hmc_trajectory_int']) == len(S['fthmc_hmc_trajectory']) + 1
    assert S['fthmc_ft_md_v'] == S['fthmc_ft_leapfrog_v'][:-1] + [ctypes.c_int, ctypes.c_uint64]
    assert S['fthmc_ft_trajectory_int_v'] == S['fthmc_ft_trajectory_v'][:-1] + [ctypes.c_int, ctypes.c_uint64]


@pytest.mark.parametrize('nstep', [1, 2, 7])
def test_force_counts(nstep):
    from fthmc_amd import _lib, ops
    lib = _lib.load()
    for name, code in IC.CODES.items():
        assert lib.fthmc_integrator_forces(code, nstep) == IC.forces(name, nstep) == ops.integrator_forces(name, nstep)
        assert len(IC.schedule(name, 0.1, nstep)[1]) == IC.forces(name, nstep)


def test_force_count_refusals():
    from fthmc_amd import _lib, ops
    lib = _lib.load()
    for code in (-1, 3, 99):
        assert lib.fthmc_integrator_forces(code, 4) < 0
    for code in (0, 1, 2):
        assert lib.fthmc_integrator_forces(code, 0) < 0 and lib.fthmc_integrator_forces(code, -3) < 0
    with pytest.raises(ValueError):
        ops.integrator_forces('verlet', 4)
    with pytest.raises(ValueError):
        ops.integrator_forces('omelyan', 0)


def _c_schedule(code, dt, nstep, cap):
    from fthmc_amd import _lib
    lib = _lib.load()
    b0 = ctypes.c_double(-7.0)
    n = max(cap, 1)
    kind, a, b = (ctypes.c_int * n)(*([-7] * n)), (ctypes.c_double * n)(*([-7.0] * n)), (ctypes.c_double * n)(*([-7.0] * n))
    rc = lib.fthmc_integrator_schedule(code, dt, nstep, ctypes.byref(b0), kind, a, b, cap)
    return rc, b0.value, list(kind), list(a), list(b)


def _ulps(x, y):
    return abs(x - y) / np.spacing(max(abs(x), abs(y))) if x != y else 0.0


@pytest.mark.parametrize('name', IC.NAMES)
@pytest.mark.parametrize('dt,nstep', [(0.125, 1), (0.1, 2), (1.0 / 7.0, 7), (0.5 / 3.0, 3)])
def test_library_schedule_is_the_written_out_schedule(name, dt, nstep):
    from fthmc_amd import _lib, ops
    b0, stages = IC.schedule(name, dt, nstep)
    n = len(stages)
    rc, cb0, kind, a, b = _c_schedule(IC.CODES[name], dt, nstep, n)
    assert rc == n
    assert _ulps(cb0, b0) <= 1
    for i, (k, sa, sb) in enumerate(stages):
        assert kind[i] == (_lib.STAGE_SHIFT if k == 'shift' else _lib.STAGE_KICK), (i, kind[i], k)        # kinds exact
        assert _ulps(a[i], sa) <= 1 and _ulps(b[i], sb) <= 1, (i, a[i], sa, b[i], sb)
    tau = dt * nstep
    kicks = math.fsum(a[i] for i in range(n) if kind[i] == _lib.STAGE_KICK)
    drifts = math.fsum([cb0] + [b[i] for i in range(n) if kind[i] == _lib.STAGE_KICK])
    assert abs(kicks - tau) <= 4 * np.spacing(tau) and abs(drifts - tau) <= 4 * np.spacing(tau), (kicks - tau, drifts - tau)
    assert all(b[i] == 0.0 for i in range(n) if kind[i] == _lib.STAGE_SHIFT)
    # a cap one short is refused and nothing is written
    rc, cb0, kind, a, b = _c_schedule(IC.CODES[name], dt, nstep, n - 1)
    assert rc < 0 and cb0 == -7.0 and all(k == -7 for k in kind) and all(v == -7.0 for v in a + b)
    # the Python view of the same list
    pb0, pst = ops.integrator_schedule(name, dt, nstep)
    assert _ulps(pb0, b0) <= 1 and [s[0] for s in pst] == [s[0] for s in stages]


def test_python_keywords_default_to_leapfrog():
    from fthmc_amd import hmc, ops
    from fthmc_amd.ft_hmc import FieldTransformation
    from fthmc_amd.utils import qed_helpers as qed
    fns = [ops.leapfrog, ops.hmc_trajectory, ops.ft_leapfrog, ops.ft_trajectory, FieldTransformation.__init__,
           qed.leapfrog, qed.hmc, qed.ft_leapfrog, qed.ft_hmc, qed.ft_run, hmc.run_hmc]
    for fn in fns:
        p = inspect.signature(fn).parameters
        assert 'integrator' in p and p['integrator'].default == 'leapfrog', fn
    assert callable(ops.integrator_forces) and callable(ops.integrator_schedule)
    with pytest.raises(ValueError):
        ops.integrator_code('verlet')


def test_config_classes_carry_no_integrator_field():
    from fthmc_amd.config import Param, TrainConfig, lfConfig
    for cls in (Param, TrainConfig, lfConfig):
        assert 'integrator' not in inspect.signature(cls.__init__).parameters, cls


# ---------------------------------------------------------------- the reference integrators are what they claim
@pytest.fixture(scope='module')
def case():
    g = torch.Generator().manual_seed(0)
    flow = R.default_flow(4, g)
    x = (torch.rand(4, 2, 8, 8, generator=g) * 2 - 1) * 3
    v = torch.randn(4, 2, 8, 8, generator=g)
    x, v = x.double(), v.double()
    flow = [tuple(t.double() for t in w) for w in flow]
    return flow, x, v, 2.0, 1.0


def _max_dh(case, name, nstep):
    flow, x, v, beta, tau = case
    with torch.no_grad():
        h0 = R.ft_action(x, flow, beta) + 0.5 * (v * v).flatten(1).sum(1)
    x_, v_ = IC.ft_md(x, v, flow, beta, name, tau / nstep, nstep)
    with torch.no_grad():
        h1 = R.ft_action(x_, flow, beta) + 0.5 * (v_ * v_).flatten(1).sum(1)
    return float((h1 - h0).abs().max())


@pytest.mark.parametrize('name,order', [('leapfrog', 1.8), ('omelyan', 1.8), ('force_gradient', 3.5)])
def test_observed_order(case, name, order):
    """log2(max|dH|(nstep 8) / max|dH|(nstep 16)) at tau = 1: 2 for the second-order schemes, 4 for the force-gradient one"""
    d8, d16 = _max_dh(case, name, 8), _max_dh(case, name, 16)
    print(f'{name}: max|dH| {d8:.4g} (nstep 8) {d16:.4g} (nstep 16), order {math.log2(d8 / d16):.3f}')
    assert math.log2(d8 / d16) >= order, (d8, d16)


@pytest.mark.parametrize('name', IC.NAMES)
def test_reversible(case, name):
    flow, x, v, beta, tau = case
    x1, v1 = IC.ft_md(x, v, flow, beta, name, tau / 8, 8)
    x2, v2 = IC.ft_md(x1, -v1, flow, beta, name, tau / 8, 8)
    assert float((x2 - x).abs().max()) < 1e-10 and float((v2 + v).abs().max()) < 1e-10


def test_leapfrog_schedule_is_the_reference_leapfrog_bit_for_bit(case):
    flow, x, v, beta, tau = case
    for nstep in (1, 3):
        a = IC.ft_md(x, v, flow, beta, 'leapfrog', tau / 5, nstep)
        b = R.leapfrog(x, v, lambda y: R.ft_force(y, flow, beta), tau / 5, nstep)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        a = IC.plain_md(x, v, beta, 'leapfrog', tau / 5, nstep)
        b = R.leapfrog(x, v, lambda y: R.wilson_force(y, beta), tau / 5, nstep)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---------------------------------------------------------------- the schedule header under the sanitizers
def test_schedule_header_walks_clean_under_asan_and_ubsan(tmp_path):
    """csrc/integrator.h in a stand-alone program (tests/hip/integrator_walk.cpp) built with -fsanitize=address,undefined by the
    recipe next to `make san`'s: all three integrators, nstep 1 .. 64, every short cap.  Its own process, nothing preloaded."""
    csrc = os.path.join(ROOT, 'fthmc_amd', 'csrc')
    exe = str(tmp_path / 'integrator_walk')
    r = subprocess.run(['make', '-C', csrc, '-f', 'san.mk', 'san_integrator', 'SANWALK=' + exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and os.path.exists(exe), r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ)
    env.update(ASAN_OPTIONS='detect_leaks=1:abort_on_error=1:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert 'ERROR: AddressSanitizer' not in r.stderr and 'runtime error:' not in r.stderr, r.stderr[-6000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out['calls'] > 10000 and out['refusals'] > 10000
