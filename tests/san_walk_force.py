#!/usr/bin/env python3
"""Walk of the HOST side of the force-norm training entry points (fthmc_train_force_grad, fthmc_train_force_ws_bytes,
fthmc_set_dual_path / fthmc_get_dual_path / fthmc_train_force_path) under AddressSanitizer + UBSan: valid calls over net shapes,
layer counts, small, ragged and the largest lattices, under every setting of the switch, and every refusal.  Run by
tests/test_sanitizer_force.py in a subprocess with the sanitizer runtime preloaded, against the `make san` build (launches are
succeeding no-ops); device pointers are made-up addresses nothing on the host dereferences.  Never on a GPU box (refused below).

Prints one JSON line {"calls": n, "refusals": m}; any sanitizer finding aborts the process (exit code != 0).
"""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

if torch.cuda.device_count() > 0:
    sys.exit('san_walk_force: a GPU is visible -- the walk passes made-up device pointers and must never run on a GPU box')
os.environ['FTHMC_ALLOW_DRYRUN'] = '1'
from fthmc_amd import _lib  # noqa: E402

OK, E_ARG, E_UNS, E_LAUNCH, E_WS = 0, -1, -2, -3, -4
MAX_B, MAX_L = 4194303, 32764
lib = _lib.load()
assert b'DRYRUN' in lib.fthmc_version(), lib.fthmc_version()

_next = [0x7E0000000000]       # made-up device addresses, 1 TB apart


def dev():
    p = _next[0]
    _next[0] += 1 << 40
    return p


WS = dev()
calls, refusals = [0], [0]


def arch(hidden=(8, 8), k=3, n_mix=2, tanh=0):
    if (tuple(hidden), k, n_mix, tanh) == ((8, 8), 3, 2, 0):
        return None
    a = _lib.ArchT()
    a.n_hidden, a.kernel_size, a.n_mix, a.final_tanh = len(hidden), k, n_mix, tanh
    for i, h in enumerate(hidden[:8]):
        a.hidden[i] = h
    return ctypes.pointer(a)


def expect(rc, want, what):
    calls[0] += 1
    if want != OK:
        refusals[0] += 1
    if rc != want:
        sys.exit(f'san_walk_force: {what}: rc {rc}, expected {want} ({lib.fthmc_strerror(rc).decode()})')


def wsb(A, B, L, nl):
    calls[0] += 1
    return int(lib.fthmc_train_force_ws_bytes(A, B, L, nl))


def grad(x, w, A, nl, B, L, act, F, fsq, gw, ws, nb):
    return lib.fthmc_train_force_grad(x, w, A, nl, B, L, act, 2.0, F, fsq, gw, ws, nb, None)


def walk(A, B, L, nl):
    x, w, F, fsq, gw = (dev() for _ in range(5))
    n = wsb(A, B, L, nl)
    assert n > int(lib.fthmc_ws_bytes(A, B, L, nl)) >= int(lib.fthmc_ws_head_bytes()), (B, L, nl, n)
    tag = f'B={B} L={L} nl={nl} path={lib.fthmc_get_dual_path()}'
    wp = w if nl else None
    for act in (0, 1, 2):
        for oF, ow in ((F, gw), (None, gw), (F, None), (None, None)):
            expect(grad(x, wp, A, nl, B, L, act, oF, fsq, ow, WS, n), OK, 'train_force_grad ' + tag)
    expect(grad(x, wp, A, nl, B, L, 0, F, fsq, gw, WS, n + (1 << 20)), OK, 'train_force_grad larger ws ' + tag)
    # refusals
    for B_, L_ in ((0, L), (-1, L), (MAX_B + 1, L), (B, 0), (B, 2), (B, 6), (B, -4), (B, MAX_L + 4)):
        expect(grad(x, w, A, nl, B_, L_, 0, F, fsq, gw, WS, n), E_ARG, f'train_force_grad B={B_} L={L_}')
        expect(0 if wsb(A, B_, L_, nl) == 0 else 1, 0, f'train_force_ws_bytes B={B_} L={L_}')
    expect(grad(None, w, A, nl, B, L, 0, F, fsq, gw, WS, n), E_ARG, 'train_force_grad xi')
    expect(grad(x, w, A, nl, B, L, 0, F, None, gw, WS, n), E_ARG, 'train_force_grad force_sq')
    expect(grad(x, w, A, -1, B, L, 0, F, fsq, gw, WS, n), E_ARG, 'train_force_grad nl')
    expect(0 if wsb(A, B, L, -1) == 0 else 1, 0, 'train_force_ws_bytes nl')
    if nl:
        expect(grad(x, None, A, nl, B, L, 0, F, fsq, gw, WS, n), E_ARG, 'train_force_grad w')
    for act in (-1, 3):
        expect(grad(x, wp, A, nl, B, L, act, F, fsq, gw, WS, n), E_UNS, 'train_force_grad act')
    for ws, nb in ((None, n), (WS, n - 1), (WS, 0), (WS, int(lib.fthmc_ws_bytes(A, B, L, nl)))):
        expect(grad(x, wp, A, nl, B, L, 0, F, fsq, gw, ws, nb), OK if ws and nb >= n else E_WS, 'train_force_grad ws')


def main():
    # the switch: its values, its refusals, and what serves a shape
    assert lib.fthmc_get_dual_path() == 1
    for v in (-1, 4, 100):
        expect(lib.fthmc_set_dual_path(v), E_ARG, f'set_dual_path {v}')
    assert lib.fthmc_get_dual_path() == 1
    shapes = [(1, 4), (2, 8), (3, 12), (2, 16), (5, 24), (7, 40), (2, 72), (1, 128), (65535, 8), (65536, 8), (1 << 20, 4), (1, MAX_L), (1, 8192),
              (3, 1032)]
    archs = [arch(), arch((4, 6), 5, 3), arch((8, 8), 3, 2, 1), arch((), 1, 1)]
    for path in (1, 0, 2, 3):
        expect(lib.fthmc_set_dual_path(path), OK, f'set_dual_path {path}')
        assert lib.fthmc_get_dual_path() == path
        for A in archs:
            for B, L in shapes:
                served = lib.fthmc_train_force_path(A, B, L)
                calls[0] += 1
                want = int(path != 0 and A is None and L % 8 == 0 and L <= 8192 and B <= 65535 and B * (L // 8) ** 2 < (1 << 30))
                assert served == want, (path, B, L, served, want)
                for nl in (0, 1, 2, 5, 70):
                    if wsb(A, B, L, nl) == 0:       # beyond size_t (the largest shapes with deep nets): refused
                        expect(grad(dev(), dev(), A, nl, B, L, 0, dev(), dev(), dev(), WS, 1 << 62), E_UNS,
                               f'train_force_grad overflowing B={B} L={L} nl={nl}')
                        continue
                    if nl and A is None and L > 8192:      # the tuned first-order sweep serves L <= 8192: its refusal comes back as it is
                        expect(grad(dev(), dev(), A, nl, B, L, 0, dev(), dev(), dev(), WS, wsb(A, B, L, nl)), E_ARG,
                               f'train_force_grad beyond the tuned kernels B={B} L={L} nl={nl}')
                        continue
                    walk(A, B, L, nl)
        # sizes never shrink as B, L or the depth grow
        for A in archs:
            prev = 0
            for B, L, nl in ((1, 8, 1), (2, 8, 1), (2, 16, 1), (2, 16, 3), (8, 64, 3), (8, 64, 8)):
                n = wsb(A, B, L, nl)
                assert n > prev, (B, L, nl, n, prev)
                prev = n
        # sizes beyond size_t
        for B, L, nl in ((MAX_B, MAX_L, 64), (1 << 20, MAX_L, 1 << 20), (MAX_B, MAX_L, (1 << 31) - 1)):
            expect(0 if wsb(None, B, L, nl) == 0 else 1, 0, f'train_force_ws_bytes overflowing B={B} L={L} nl={nl}')
            x = dev()
            expect(grad(x, x, None, nl, B, L, 0, x, x, x, WS, 1 << 62), E_UNS, f'train_force_grad overflowing B={B} L={L} nl={nl}')
        # net shapes the plain kernels refuse, and a circular pad wider than the lattice
        for A in (arch((8, 8), 4, 2), arch((8, 8), 17, 2), arch((8, 8), 3, 0), arch((300,), 3, 2), arch((8,) * 9, 3, 2)):
            x = dev()
            expect(grad(x, x, A, 2, 2, 8, 0, x, x, x, WS, 1 << 40), E_UNS, 'train_force_grad arch')
            expect(0 if wsb(A, 2, 8, 2) == 0 else 1, 0, 'train_force_ws_bytes arch')
            assert lib.fthmc_train_force_path(A, 2, 8) < 0
        A = arch((4,), 15, 2)
        x = dev()
        expect(grad(x, x, A, 2, 2, 4, 0, x, x, x, WS, 1 << 40), E_UNS, 'train_force_grad pad > L')
        expect(0 if wsb(A, 2, 4, 2) == 0 else 1, 0, 'train_force_ws_bytes pad > L')
        assert wsb(A, 2, 4, 0) > 0 and wsb(A, 2, 16, 2) > 0
    expect(lib.fthmc_set_dual_path(1), OK, 'set_dual_path 1')
    print(json.dumps({'calls': calls[0], 'refusals': refusals[0], 'library': lib.fthmc_version().decode()}), flush=True)


if __name__ == '__main__':
    main()
