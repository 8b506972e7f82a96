"""What every GPU test module shares: the guard for the library's process-global kernel-family switches, the module fixture that
holds a module's defaults open, the host <-> device helpers, the tolerance checks and the NaN-filled output buffers.  A plain module,
imported like the *_cases.py ones; importing it loads no library (fthmc_amd.ops and _lib load on first use)."""
import contextlib
import os

import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)

from fthmc_amd import _lib, ops  # noqa: F401
from fthmc_amd.graph_loop import capture  # noqa: F401  (torch.cuda.graph with the garbage collector held off, see there)
from oracle import ref_cpu as R  # noqa: F401

GUARD = 8


class _Library:
    """the loaded C ABI, looked up at the call: lib.fthmc_x(...) is _lib.load().fthmc_x(...)"""

    def __getattr__(self, name):
        return getattr(_lib.load(), name)


lib = _Library()


@contextlib.contextmanager
def switches(variant=None, small=None, dual=None, leap_rows=None):
    """The process-global switches that are named, set for the block; whatever the getters (and the environment) held before is
    put back afterwards, also after an exception; a switch that is not named is not written.  leap_rows sets FTHMC_LEAP_ROWS, which
    the library reads with the variant: set_variant(get_variant()) makes it read again, on entry and on exit, and a variable that
    was unset is deleted once the library has read the row strips on again, as it starts."""
    before = (ops.get_variant() if variant is not None else None, ops.get_small_path() if small is not None else None,
              ops.get_dual_path() if dual is not None else None, os.environ.get('FTHMC_LEAP_ROWS'))
    try:
        if leap_rows is not None:
            os.environ['FTHMC_LEAP_ROWS'] = '1' if leap_rows else '0'
            ops.set_variant(ops.get_variant())
        if variant is not None:
            ops.set_variant(variant)
        if small is not None:
            ops.set_small_path(small)
        if dual is not None:
            ops.set_dual_path(dual)
        yield
    finally:
        if dual is not None:
            ops.set_dual_path(before[2])
        if small is not None:
            ops.set_small_path(before[1])
        if variant is not None:
            ops.set_variant(before[0])
        if leap_rows is not None:
            os.environ['FTHMC_LEAP_ROWS'] = '1' if before[3] is None else before[3]
            ops.set_variant(ops.get_variant())
            if before[3] is None:
                del os.environ['FTHMC_LEAP_ROWS']


def defaults_held(variant=1, small=True, **more):
    """a device is there, and these switches are held for as long as the generator is open"""
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    with switches(variant=variant, small=small, **more):
        yield


def module_defaults(**defaults):
    """-> the module-scoped autouse fixture of a GPU test module: the module runs under defaults_held(**defaults)"""
    @pytest.fixture(scope='module', autouse=True)
    def _gpu_defaults():
        yield from defaults_held(**defaults)
    return _gpu_defaults


def H(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def D(a, dtype=torch.float64):
    """a tensor, an array (a longdouble one too) or a nested sequence -> a device tensor of `dtype`, always a copy of host data"""
    if not torch.is_tensor(a):
        a = np.array(a)
        a = torch.from_numpy(a.astype(np.float64) if a.dtype == np.longdouble else a)
    return a.to(dtype).cuda()


def close(a, b, rtol=1e-10, atol=1e-10):
    np.testing.assert_allclose(H(a), H(b), rtol=rtol, atol=atol)


def angle_close(a, b, atol=1e-9):
    d = (H(a) - H(b) + np.pi) % (2 * np.pi) - np.pi
    assert np.max(np.abs(d)) < atol, np.max(np.abs(d))


def bits(a):
    return np.ascontiguousarray(H(a)).view(np.int64)


class Poisoned:
    """n doubles at offset GUARD of a NaN-filled allocation with GUARD words behind them"""

    def __init__(self, n, init=None):
        self.n = n
        self.buf = torch.full((2 * GUARD + n,), float('nan'), dtype=torch.float64, device='cuda')
        self.t = self.buf[GUARD:GUARD + n]
        if init is not None:
            self.t.copy_(torch.as_tensor(np.asarray(init, dtype=np.float64)))
        self.before = self.guards()

    def guards(self):
        return np.concatenate([bits(self.buf[:GUARD]), bits(self.buf[GUARD + self.n:])])

    def intact(self):
        return np.array_equal(self.guards(), self.before)
