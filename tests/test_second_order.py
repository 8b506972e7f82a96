"""CPU-only tests of the second-order path (the VJPs of S_eff and of the force): the C ABI declares and exports it, the ctypes
signatures, the workspace sizes, the compiled operators, the host side under the sanitizers, and the fixture."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

NEW = ('fthmc_ft_action_vjp', 'fthmc_ft_force_vjp', 'fthmc_vjp_ws_bytes')


def test_header_library_and_signatures_carry_the_second_order_entry_points():
    from fthmc_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'fthmc_hip.h')).read()
    declared = set(re.findall(r'\b(fthmc_[a-z0-9_]+)\s*\(', header))
    for name in NEW:
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES['fthmc_ft_action_vjp']) == 15 and len(_lib.SIGNATURES['fthmc_ft_force_vjp']) == 14
    assert _lib.SIGNATURES['fthmc_vjp_ws_bytes'] == _lib.SIGNATURES['fthmc_ws_bytes']


def test_vjp_workspace_sizes():
    from fthmc_amd import _lib, ops
    lib = _lib.load()
    head = int(lib.fthmc_ws_head_bytes())
    for a in (None, ((4, 6), 5, 3), ((16,), 3, 1), ((8, 8), 3, 2, True), ((), 1, 1)):
        ap = ops._arch(a)
        prev = 0
        for B, L, nl in ((1, 8, 0), (1, 8, 1), (2, 8, 1), (2, 12, 1), (2, 12, 2), (8, 64, 2), (8, 64, 8), (32, 256, 16)):
            n = int(lib.fthmc_vjp_ws_bytes(ap, B, L, nl))
            assert n > head and n >= prev, (a, B, L, nl, n, prev)
            prev = n
        assert ops.vjp_ws_bytes(4, 16, 3, a) == lib.fthmc_vjp_ws_bytes(ap, 4, 16, 3)
    for B, L, nl in ((0, 8, 2), (2, 6, 2), (2, 0, 2), (2, 8, -1), (4194304, 8, 1), (2, 32768, 1), (4194303, 32764, 64)):
        assert lib.fthmc_vjp_ws_bytes(None, B, L, nl) == 0, (B, L, nl)
    assert lib.fthmc_vjp_ws_bytes(ops._arch(((8, 8), 17, 2)), 2, 8, 2) == 0       # even / too large a kernel
    assert lib.fthmc_vjp_ws_bytes(ops._arch(((4,), 15, 2)), 2, 4, 2) == 0        # circular pad wider than the lattice
    assert lib.fthmc_vjp_ws_bytes(ops._arch(((4,), 15, 2)), 2, 4, 0) > 0         # ... no net without layers


def test_compiled_operators_define_the_vjps_and_refuse_cpu_tensors():
    so = os.path.join(ROOT, 'fthmc_amd', 'libfthmc_torch.so')
    if not os.path.exists(so):
        pytest.skip('libfthmc_torch.so not built (make -C fthmc_amd/csrc)')
    import fthmc_amd.torch_ops as T
    assert T.BACKEND == 'compiled'
    for name in ('ft_action_vjp', 'ft_force_vjp'):
        assert name in T.__all__
        sch = str(getattr(torch.ops.fthmc_hip, name).default._schema)
        assert sch.startswith('fthmc_hip::' + name + '(')
        assert 'int n_mix=2' in sch and 'int[]? hidden=None' in sch and 'int kernel_size=3' in sch, sch
    assert 'Tensor? glogdet=None' in str(torch.ops.fthmc_hip.ft_action_vjp.default._schema)
    x = torch.zeros(1, 2, 8, 8, dtype=torch.float64)
    w = torch.zeros(955, dtype=torch.float64)
    with pytest.raises(NotImplementedError):
        torch.ops.fthmc_hip.ft_force_vjp(x, w, 1, 1.0, 0, x)
    with pytest.raises(NotImplementedError):
        torch.ops.fthmc_hip.ft_action_vjp(x, w, 1, 1.0, 0, torch.ones(1, dtype=torch.float64))


def test_fake_functions_give_the_vjp_shapes():
    import fthmc_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        x = torch.empty(3, 2, 8, 8, dtype=torch.float64, device='cuda')
        w = torch.empty(2 * 955, dtype=torch.float64, device='cuda')
        gx, gw = torch.ops.fthmc_hip.ft_force_vjp(x, w, 2, 1.0, 0, x)
        assert gx.shape == x.shape and gw.shape == w.shape
        gx, gw = torch.ops.fthmc_hip.ft_action_vjp(x, w, 2, 1.0, 0, x.new_empty(3))
        assert gx.shape == x.shape and gw.shape == w.shape


def test_public_entry_points_have_no_cpu_fallback():
    from fthmc_amd import ops
    from fthmc_amd._lib import FthmcError
    x = torch.zeros(1, 2, 8, 8, dtype=torch.float64)
    with pytest.raises(FthmcError):
        ops.ft_force_vjp(x, None, 0, 1.0, x)
    with pytest.raises(FthmcError):
        ops.ft_action_vjp(x, None, 0, 1.0, torch.ones(1, dtype=torch.float64))


def test_second_order_fixture_is_small_and_complete():
    path = os.path.join(ROOT, 'tests', 'golden', 'second_order_L8.npz')
    assert os.path.getsize(path) < 100 * 1024
    g = np.load(path)
    nl = int(g['n_layers'])
    assert g['x'].shape == g['g'].shape == g['Hg'].shape == g['F'].shape == (2, 2, 8, 8) and nl == 2 and str(g['act']) == 'silu'
    for li in range(nl):
        for pi in range(6):
            assert g[f'w{li}_{pi}'].shape == g[f'gw{li}_{pi}'].shape == g[f'ga_w{li}_{pi}'].shape
    # the Hessian-vector product is not the force and not zero
    assert np.abs(g['Hg']).max() > 1e-3 and not np.allclose(g['Hg'], g['F'])


# ---------------------------------------------------------------- host side under AddressSanitizer + UBSan
@pytest.fixture(scope='module')
def san_runtime():
    import glob
    import shutil
    if torch.cuda.device_count() > 0:
        pytest.skip('the sanitizer walk passes made-up device pointers: CPU boxes only')
    if shutil.which('hipcc') is None and not os.path.exists('/opt/rocm/bin/hipcc'):
        pytest.skip('no hipcc: the sanitizer build needs the ROCm toolchain')
    hits = sorted(glob.glob('/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.so'))
    assert hits, 'libclang_rt.asan-x86_64.so not found under /opt/rocm/lib/llvm'
    r = subprocess.run(['make', '-C', os.path.join(ROOT, 'fthmc_amd', 'csrc'), 'san'], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return hits[-1]


def test_vjp_entry_points_walk_clean_under_asan_and_ubsan(san_runtime):
    env = dict(os.environ)
    env.update(LD_PRELOAD=san_runtime, FTHMC_LIB=os.path.join(ROOT, 'fthmc_amd', 'libfthmc_hip_san.so'), FTHMC_ALLOW_DRYRUN='1',
               PYTHONDONTWRITEBYTECODE='1', ASAN_OPTIONS='detect_leaks=0:abort_on_error=1:halt_on_error=1:detect_odr_violation=0',
               UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'san_walk_vjp.py')], capture_output=True, text=True, env=env,
                       timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert 'ERROR: AddressSanitizer' not in r.stderr and 'runtime error:' not in r.stderr, r.stderr[-6000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out['calls'] > 2000 and out['refusals'] > 1000 and 'DRYRUN' in out['library']
