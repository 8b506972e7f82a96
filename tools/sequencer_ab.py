#!/usr/bin/env python3
"""The two host sequencers of csrc/api.hip (hmc_trajectory_call, ft_trajectory_call; each with its optional bias) against the
parent commit's four, call for call.

    python tools/sequencer_ab.py --parent-tree DIR [--min-ms 1000] [--bench-steps 100] [--bench-rounds 2] [--out FILE]

DIR/fthmc_amd/libfthmc_hip.so, the parent commit's library, is loaded next to this tree's.  Prepared arguments go through the C ABI of
both, in five blocks of each ALTERNATING (HIP events around a block; at least --min-ms of calls per library and row, after a warm-up;
the two libraries write into the SAME scratch and outputs and take turns at going first -- with a scratch buffer each and a fixed
order, a copy of the parent's library measured 0.2 to 1.2 % slower than the parent's library itself):
  * fthmc_meta_trajectory, path 2, 128 chains at L = 64 (one shared table: nb = 81, qmax = 4, wall = 50), leapfrog;
  * fthmc_hmc_trajectory_int, 128 chains at L = 128 (beyond the one-launch kernel), omelyan;
  * fthmc_ft_trajectory_v and fthmc_ft_meta_trajectory_v at config 2 (32 chains, L = 16, 4 layers, beta = 4) with the small path off.
beta = 6 on the plain rows, 10 steps of 0.1.  The launches of the two libraries are the same, so the parent's own spread is the only
margin: pass = median(this) <= median(parent) + (max - min) of the parent's five blocks.
Then `bench.py --gpus 1` of DIR and of this tree alternately (child processes, first: this process has not opened the GPU yet).
Prints one JSON document (also to --out)."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import torch  # noqa: E402

from instanton_ab import blocks_of  # noqa: E402
from loops_ab import bench_ab  # noqa: E402

SEED = 31415
DT, NSTEP = 0.1, 10


def parent_lib(tree, _lib):
    lib = ctypes.CDLL(os.path.join(tree, 'fthmc_amd', 'libfthmc_hip.so'))
    for name in ('fthmc_meta_trajectory', 'fthmc_hmc_trajectory_int', 'fthmc_ft_trajectory_v', 'fthmc_ft_meta_trajectory_v', 'fthmc_set_small_path',
                 'fthmc_meta_ws_bytes', 'fthmc_ws_bytes', 'fthmc_ft_meta_ws_bytes'):
        getattr(lib, name).argtypes = _lib.SIGNATURES[name]
        getattr(lib, name).restype = _lib._RESTYPE.get(name, ctypes.c_int)
    lib.fthmc_version.restype = ctypes.c_char_p
    return lib


def rows(ops, _lib, libs, dev, min_ms):
    """libs: {'parent': lib, 'this': lib}"""
    p, gen = ops._p, torch.Generator().manual_seed(SEED)
    f64 = dict(dtype=torch.float64, device=dev)

    def fields(B, L, amp):
        x = ((torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * amp).to(dev)
        return x, torch.randn(B, 2, L, L, generator=gen, dtype=torch.float64).to(dev), torch.rand(B, generator=gen, dtype=torch.float64).to(dev)

    def scratch(query):
        """one scratch for both libraries, of the larger of their two sizes (the same memory under either: no placement effect)"""
        return torch.empty(max(max(int(query(lib)) for lib in libs.values()), 8) // 8, **f64)
    tab = (0.5 * torch.linspace(-4, 4, 81, dtype=torch.float64) ** 2).reshape(1, 81).to(dev)
    out = []

    def row(name, B, L, call_of):
        """call_of(lib) -> a closure of one call on the current stream"""
        fns = {k: call_of(lib) for k, lib in libs.items()}
        for fn in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        n = max(5, int(math.ceil(min_ms / max(blocks_of(fns['this'], 3), 1e-3) / 5)))
        blocks = {'parent': [], 'this': []}
        for i in range(5):
            for k in (('parent', 'this'), ('this', 'parent'))[i % 2]:
                blocks[k].append(blocks_of(fns[k], n))
        med = {k: statistics.median(v) for k, v in blocks.items()}
        spread = max(blocks['parent']) - min(blocks['parent'])
        out.append(dict(call=name, B=B, L=L, calls_per_block=n, ms_parent=blocks['parent'], ms_this=blocks['this'], median_parent=med['parent'],
                        median_this=med['this'], parent_spread=spread, passed=bool(med['this'] <= med['parent'] + spread)))

    s = torch.cuda.current_stream(dev).cuda_stream
    # ---- plain, biased, sequenced
    B, L = 128, 64
    x, v, u = fields(B, L, 0.3)
    xn = torch.empty_like(x)
    vec = [torch.empty(B, **f64) for _ in range(6)]
    ws = scratch(lambda lib: lib.fthmc_meta_ws_bytes(B, L, 2))

    def meta_call(lib):
        args = (p(x), p(v), p(u), B, L, 6.0, DT, NSTEP, 0, p(tab), 1, 81, 4.0, 50.0, 2, p(xn), *(p(t) for t in vec), p(ws), ws.numel() * 8, s)
        def fn():
            assert lib.fthmc_meta_trajectory(*args) == 0
        return fn
    row('fthmc_meta_trajectory path=2', B, L, meta_call)
    # ---- plain, beyond the one-launch kernel
    L = 128
    x2, v2, u2 = fields(B, L, 0.3)
    xn2 = torch.empty_like(x2)
    ws2 = scratch(lambda lib: lib.fthmc_ws_bytes(None, B, L, 0))

    def hmc_call(lib):
        args = (p(x2), p(v2), p(u2), B, L, 6.0, DT, NSTEP, _lib.INTEGRATORS['omelyan'], p(xn2), *(p(t) for t in vec[:4]), p(ws2), ws2.numel() * 8, s)
        def fn():
            assert lib.fthmc_hmc_trajectory_int(*args) == 0
        return fn
    row('fthmc_hmc_trajectory_int', B, L, hmc_call)
    # ---- flowed, config 2, small path off
    from oracle import ref_cpu as R
    B, L, nl, beta = 32, 16, 4, 4.0
    x3, v3, u3 = fields(B, L, 0.3)
    xn3 = torch.empty_like(x3)
    w = ops.pack_weights(R.default_flow(nl, torch.Generator().manual_seed(SEED)), device=dev)
    o = [torch.empty(B, **f64) for _ in range(8)]
    st = torch.empty(4, B, **f64)
    for lib in libs.values():
        assert lib.fthmc_set_small_path(0) == 0
    try:
        ws3 = scratch(lambda lib: lib.fthmc_ft_meta_ws_bytes(None, B, L, nl))        # serves the unbiased call too

        def ft_call(lib):
            args = (p(x3), p(v3), p(u3), p(w), None, nl, B, L, 0, beta, DT, NSTEP, 0, p(xn3), *(p(t) for t in o[:6]), None, p(st), p(ws3),
                    ws3.numel() * 8, s, 1)
            def fn():
                assert lib.fthmc_ft_trajectory_v(*args) == 0
            return fn
        row('fthmc_ft_trajectory_v (small path off)', B, L, ft_call)

        def ft_meta_call(lib):
            args = (p(x3), p(v3), p(u3), p(w), None, nl, B, L, 0, beta, DT, NSTEP, 0, p(tab), 1, 81, 4.0, 50.0, p(xn3), *(p(t) for t in o), None,
                    p(st), p(ws3), ws3.numel() * 8, s, 1)
            def fn():
                assert lib.fthmc_ft_meta_trajectory_v(*args) == 0
            return fn
        row('fthmc_ft_meta_trajectory_v (small path off)', B, L, ft_meta_call)
    finally:
        for lib in libs.values():
            lib.fthmc_set_small_path(1)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--parent-tree', required=True, help='a built checkout of the parent commit')
    ap.add_argument('--min-ms', type=float, default=1000.0, help='timed work per library and row, at least')
    ap.add_argument('--bench-steps', type=int, default=100)
    ap.add_argument('--bench-warmup', type=int, default=10)
    ap.add_argument('--bench-rounds', type=int, default=2)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    parent = os.path.abspath(args.parent_tree)
    doc = dict(tool='tools/sequencer_ab.py')
    if args.bench_rounds > 0:                                           # first, in child processes: this one has not opened the GPU yet
        b = doc['bench'] = bench_ab(parent, args.bench_steps, args.bench_warmup, args.bench_rounds)
        vp, vt = ([r['value'] for r in b[k]] for k in ('parent', 'this'))
        doc['bench_values'] = dict(parent=vp, this=vt, unit=b['this'][0].get('unit'), metric=b['this'][0].get('metric'))
    from fthmc_amd import _lib, ops
    assert torch.cuda.is_available(), 'needs the GPU'
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    this, par = _lib.load(), parent_lib(parent, _lib)
    doc['this'], doc['parent'] = this.fthmc_version().decode(), par.fthmc_version().decode()
    doc['device'] = torch.cuda.get_device_name(dev)
    doc['rows'] = rows(ops, _lib, {'parent': par, 'this': this}, dev, args.min_ms)
    doc['passed'] = all(r['passed'] for r in doc['rows'])
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
