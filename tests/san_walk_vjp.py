#!/usr/bin/env python3
"""Walk of the HOST side of the second-order entry points (fthmc_ft_action_vjp, fthmc_ft_force_vjp, fthmc_vjp_ws_bytes) under
AddressSanitizer + UBSan: valid calls over net shapes, layer counts, ragged and large lattices, every refusal.  Run by
tests/test_second_order.py in a subprocess with the sanitizer runtime preloaded, against the `make san` build (launches are
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
    sys.exit('san_walk_vjp: a GPU is visible -- the walk passes made-up device pointers and must never run on a GPU box')
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
        sys.exit(f'san_walk_vjp: {what}: rc {rc}, expected {want} ({lib.fthmc_strerror(rc).decode()})')


def wsb(A, B, L, nl):
    calls[0] += 1
    return int(lib.fthmc_vjp_ws_bytes(A, B, L, nl))


def walk(A, B, L, nl):
    x, w, g, gS, gld, gx, gw = (dev() for _ in range(7))
    n = wsb(A, B, L, nl)
    assert n > int(lib.fthmc_ws_head_bytes()), (B, L, nl, n)
    tag = f'B={B} L={L} nl={nl}'
    wp = w if nl else None
    for act in (0, 1, 2):
        for ox, ow in ((gx, gw), (gx, None), (None, gw)):
            expect(lib.fthmc_ft_action_vjp(x, wp, A, nl, B, L, act, 2.0, gS, gld, ox, ow, WS, n, None), OK, 'action_vjp ' + tag)
            expect(lib.fthmc_ft_action_vjp(x, wp, A, nl, B, L, act, 2.0, gS, None, ox, ow, WS, n, None), OK, 'action_vjp ' + tag)
            expect(lib.fthmc_ft_force_vjp(x, wp, A, nl, B, L, act, 2.0, g, ox, ow, WS, n, None), OK, 'force_vjp ' + tag)
    # refusals
    for B_, L_ in ((0, L), (-1, L), (MAX_B + 1, L), (B, 0), (B, 2), (B, 6), (B, -4), (B, MAX_L + 4)):
        expect(lib.fthmc_ft_action_vjp(x, w, A, nl, B_, L_, 0, 2.0, gS, gld, gx, gw, WS, n, None), E_ARG, f'action_vjp B={B_} L={L_}')
        expect(lib.fthmc_ft_force_vjp(x, w, A, nl, B_, L_, 0, 2.0, g, gx, gw, WS, n, None), E_ARG, f'force_vjp B={B_} L={L_}')
        expect(0 if wsb(A, B_, L_, nl) == 0 else 1, 0, f'vjp_ws_bytes B={B_} L={L_}')
    expect(lib.fthmc_ft_action_vjp(None, w, A, nl, B, L, 0, 2.0, gS, gld, gx, gw, WS, n, None), E_ARG, 'action_vjp x')
    expect(lib.fthmc_ft_action_vjp(x, w, A, nl, B, L, 0, 2.0, None, gld, gx, gw, WS, n, None), E_ARG, 'action_vjp gS')
    expect(lib.fthmc_ft_action_vjp(x, w, A, nl, B, L, 0, 2.0, gS, gld, None, None, WS, n, None), E_ARG, 'action_vjp outputs')
    expect(lib.fthmc_ft_action_vjp(x, w, A, -1, B, L, 0, 2.0, gS, gld, gx, gw, WS, n, None), E_ARG, 'action_vjp nl')
    expect(lib.fthmc_ft_force_vjp(None, w, A, nl, B, L, 0, 2.0, g, gx, gw, WS, n, None), E_ARG, 'force_vjp x')
    expect(lib.fthmc_ft_force_vjp(x, w, A, nl, B, L, 0, 2.0, None, gx, gw, WS, n, None), E_ARG, 'force_vjp g')
    expect(lib.fthmc_ft_force_vjp(x, w, A, nl, B, L, 0, 2.0, g, None, None, WS, n, None), E_ARG, 'force_vjp outputs')
    expect(lib.fthmc_ft_force_vjp(x, w, A, -2, B, L, 0, 2.0, g, gx, gw, WS, n, None), E_ARG, 'force_vjp nl')
    if nl:
        expect(lib.fthmc_ft_action_vjp(x, None, A, nl, B, L, 0, 2.0, gS, gld, gx, gw, WS, n, None), E_ARG, 'action_vjp w')
        expect(lib.fthmc_ft_force_vjp(x, None, A, nl, B, L, 0, 2.0, g, gx, gw, WS, n, None), E_ARG, 'force_vjp w')
    for act in (-1, 3):
        expect(lib.fthmc_ft_action_vjp(x, wp, A, nl, B, L, act, 2.0, gS, gld, gx, gw, WS, n, None), E_UNS, 'action_vjp act')
        expect(lib.fthmc_ft_force_vjp(x, wp, A, nl, B, L, act, 2.0, g, gx, gw, WS, n, None), E_UNS, 'force_vjp act')
    for ws, nb in ((None, n), (WS, n - 1), (WS, 0), (WS, int(lib.fthmc_ws_bytes(A, B, L, nl)) if nl else 0)):
        want = OK if ws and nb >= n else E_WS
        expect(lib.fthmc_ft_action_vjp(x, wp, A, nl, B, L, 0, 2.0, gS, gld, gx, gw, ws, nb, None), want, 'action_vjp ws')
        expect(lib.fthmc_ft_force_vjp(x, wp, A, nl, B, L, 0, 2.0, g, gx, gw, ws, nb, None), want, 'force_vjp ws')


def main():
    shapes = [(1, 4), (2, 8), (3, 12), (5, 20), (7, 36), (2, 68), (1, 128), (MAX_B, 4), (1, MAX_L), (3, 1028)]
    archs = [arch(), arch((4, 6), 5, 3), arch((16,), 3, 1), arch((8, 8), 3, 2, 1), arch((5, 7, 3), 7, 4, 1), arch((), 1, 1)]
    for A in archs:
        for B, L in shapes:
            for nl in (0, 1, 2, 5):
                if wsb(A, B, L, nl) == 0:       # beyond size_t (the largest shapes with deep nets): refused
                    for f in ('action', 'force'):
                        rc = (lib.fthmc_ft_action_vjp(dev(), dev(), A, nl, B, L, 0, 2.0, dev(), None, dev(), None, WS, 1 << 62, None)
                              if f == 'action' else lib.fthmc_ft_force_vjp(dev(), dev(), A, nl, B, L, 0, 2.0, dev(), dev(), None, WS, 1 << 62, None))
                        expect(rc, E_UNS, f'{f}_vjp overflowing B={B} L={L} nl={nl}')
                    continue
                walk(A, B, L, nl)
    # sizes never shrink as B, L or the depth grow
    for A in archs:
        prev = 0
        for B, L, nl in ((1, 8, 1), (2, 8, 1), (2, 16, 1), (2, 16, 3), (8, 64, 3), (8, 64, 8)):
            n = wsb(A, B, L, nl)
            assert n >= prev > -1, (B, L, nl, n, prev)
            prev = n
    # net shapes the plain kernels refuse, and a circular pad wider than the lattice
    for A in (arch((8, 8), 4, 2), arch((8, 8), 17, 2), arch((8, 8), 3, 0), arch((300,), 3, 2), arch((8,) * 9, 3, 2)):
        x = dev()
        expect(lib.fthmc_ft_force_vjp(x, x, A, 2, 2, 8, 0, 2.0, x, x, x, WS, 1 << 40, None), E_UNS, 'force_vjp arch')
        expect(lib.fthmc_ft_action_vjp(x, x, A, 2, 2, 8, 0, 2.0, x, None, x, x, WS, 1 << 40, None), E_UNS, 'action_vjp arch')
        expect(0 if wsb(A, 2, 8, 2) == 0 else 1, 0, 'vjp_ws_bytes arch')
    A = arch((4,), 15, 2)
    x = dev()
    expect(lib.fthmc_ft_force_vjp(x, x, A, 2, 2, 4, 0, 2.0, x, x, x, WS, 1 << 40, None), E_UNS, 'force_vjp pad > L')
    expect(lib.fthmc_ft_action_vjp(x, x, A, 2, 2, 4, 0, 2.0, x, None, x, x, WS, 1 << 40, None), E_UNS, 'action_vjp pad > L')
    expect(0 if wsb(A, 2, 4, 2) == 0 else 1, 0, 'vjp_ws_bytes pad > L')
    assert wsb(A, 2, 4, 0) > 0 and wsb(A, 2, 16, 2) > 0
    print(json.dumps({'calls': calls[0], 'refusals': refusals[0], 'library': lib.fthmc_version().decode()}), flush=True)


if __name__ == '__main__':
    main()
