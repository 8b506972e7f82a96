"""CPU-only: the HOST side of the force-norm training entry points (fthmc_train_force_grad, its size function, the dual-path
switch) under AddressSanitizer + UBSan, in the manner of test_sanitizer.py: tests/san_walk_force.py takes them through every
refusal and through shapes up to the limits against the `make san` build (launches are succeeding no-ops), in a subprocess that
has the sanitizer runtime preloaded.  Never on a GPU box."""
import glob
import json
import os
import shutil
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

CSRC = os.path.join(ROOT, 'fthmc_amd', 'csrc')
SAN = os.path.join(ROOT, 'fthmc_amd', 'libfthmc_hip_san.so')


def _stale():
    """the sanitizer build is absent or older than a source it is built from"""
    if not os.path.exists(SAN):
        return True
    t = os.path.getmtime(SAN)
    srcs = glob.glob(os.path.join(CSRC, '*.hip')) + glob.glob(os.path.join(CSRC, '*.h')) + [os.path.join(ROOT, 'include', 'fthmc_hip.h')]
    return any(os.path.getmtime(f) > t for f in srcs)


@pytest.fixture(scope='module')
def san_build():
    if torch.cuda.device_count() > 0:
        pytest.skip('the sanitizer walk passes made-up device pointers: CPU boxes only')
    if shutil.which('hipcc') is None and not os.path.exists('/opt/rocm/bin/hipcc'):
        pytest.skip('no hipcc: the sanitizer build needs the ROCm toolchain')
    hits = sorted(glob.glob('/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.so'))
    assert hits, 'libclang_rt.asan-x86_64.so not found under /opt/rocm/lib/llvm'
    if _stale():                       # test_sanitizer.py has usually just built it
        r = subprocess.run(['make', '-C', CSRC, 'san'], capture_output=True, text=True, timeout=1500)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    syms = subprocess.run(['nm', '-D', '--defined-only', SAN], capture_output=True, text=True).stdout
    assert 'fthmc_train_force_grad' in syms and 'fthmc_set_dual_path' in syms
    return hits[-1]


def test_force_training_entry_points_walk_clean_under_asan_and_ubsan(san_build):
    env = dict(os.environ)
    # the sanitizer runtime goes first; whatever the environment already preloads stays behind it
    pre = san_build + (':' + env['LD_PRELOAD'] if env.get('LD_PRELOAD') else '')
    env.update(LD_PRELOAD=pre, FTHMC_LIB=SAN, FTHMC_ALLOW_DRYRUN='1', PYTHONDONTWRITEBYTECODE='1',
               ASAN_OPTIONS='detect_leaks=0:abort_on_error=1:halt_on_error=1:detect_odr_violation=0',
               UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'san_walk_force.py')], capture_output=True, text=True, env=env,
                       timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert 'ERROR: AddressSanitizer' not in r.stderr and 'runtime error:' not in r.stderr, r.stderr[-6000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out['calls'] > 5000 and out['refusals'] > 2000 and 'DRYRUN' in out['library']
