#!/usr/bin/env python3
"""The one-launch plain trajectory kernels (csrc/traj_resident.h) timed against the parent commit's library, in alternating blocks.

    python tools/resident_ab.py --parent-tree DIR [--rounds 5] [--block-ms 200] [--out profiles/resident_plan_ab.json]

Both libraries are loaded side by side and entered through the C ABI with the SAME arguments: one field, one set of outputs and one
scratch for both, and the two take turns at going first (tools/sequencer_ab.py's method: with buffers of its own per library and a
fixed order a copy of the parent's library does not measure like the parent's library).  Per shape
(128 chains at L = 64, 32 chains at L = 16) and per kernel instance -- k_hmc_trajectory (leapfrog, scalar beta),
k_hmc_trajectory_sched<false> (Omelyan, scalar beta), k_hmc_trajectory_sched<true> (leapfrog, per-chain beta), k_meta_trajectory
(leapfrog under a table, path 1) -- --rounds blocks of the parent alternate with --rounds blocks of this tree, every block at least
--block-ms of calls between two HIP events (what a row of meta_ab / sequencer_ab gets: 1000 ms over five blocks).  beta = 6, 10
steps of 0.1, as there.
pass = the new mean <= the parent's mean + the parent's own spread (max - min of its block means).  Prints one JSON document."""
import argparse
import ctypes
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import torch  # noqa: E402

from instanton_ab import blocks_of  # noqa: E402

SEED = 31415
BETA, DT, NSTEP = 6.0, 0.1, 10
NB, QMAX, WALL = 81, 4.0, 50.0
LEAPFROG, OMELYAN = 0, 1


def library(path):
    lib = ctypes.CDLL(path)
    V, I, D, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_size_t
    lib.fthmc_hmc_trajectory_int.argtypes = [V, V, V, I, I, D, D, I, I, V, V, V, V, V, V, Z, V]
    lib.fthmc_hmc_trajectory_pb.argtypes = [V, V, V, I, I, V, D, I, I, V, V, V, V, V, V, Z, V]
    lib.fthmc_meta_trajectory.argtypes = [V, V, V, I, I, D, D, I, I, V, I, I, D, D, I, V, V, V, V, V, V, V, V, Z, V]
    lib.fthmc_version.restype = ctypes.c_char_p
    return lib


def calls_of(libs, dev, B, L, ws):
    """{library: {instance: a call of it}}: every call on the same field, momenta, uniforms, outputs and scratch"""
    gen = torch.Generator().manual_seed(SEED)
    x = ((torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * 0.3).to(dev)
    v = torch.randn(B, 2, L, L, generator=gen, dtype=torch.float64).to(dev)
    u = torch.rand(B, generator=gen, dtype=torch.float64).to(dev)
    bb = torch.full((B,), BETA, dtype=torch.float64, device=dev)
    q = -QMAX + torch.arange(NB, dtype=torch.float64) * (2 * QMAX / (NB - 1))
    table = (0.5 * q * q).reshape(1, NB).to(dev)
    xn = torch.empty_like(x)
    o = [torch.empty(B, dtype=torch.float64, device=dev) for _ in range(6)]
    s = torch.cuda.current_stream(dev).cuda_stream
    head, out = (x.data_ptr(), v.data_ptr(), u.data_ptr(), B, L), (xn.data_ptr(),) + tuple(t.data_ptr() for t in o[:4])
    keep = (x, v, u, bb, table, xn, o)

    def of(lib):
        def plain(integrator):
            def call(_keep=keep):
                assert lib.fthmc_hmc_trajectory_int(*head, BETA, DT, NSTEP, integrator, *out, None, 0, s) == 0
            return call

        def per_chain(_keep=keep):
            assert lib.fthmc_hmc_trajectory_pb(*head, bb.data_ptr(), DT, NSTEP, LEAPFROG, *out, None, 0, s) == 0

        def biased(_keep=keep):
            assert lib.fthmc_meta_trajectory(*head, BETA, DT, NSTEP, LEAPFROG, table.data_ptr(), 1, NB, QMAX, WALL, 1, *out, o[4].data_ptr(),
                                             o[5].data_ptr(), ws.data_ptr(), ws.numel(), s) == 0
        return {'k_hmc_trajectory': plain(LEAPFROG), 'k_hmc_trajectory_sched<false>': plain(OMELYAN), 'k_hmc_trajectory_sched<true>': per_chain,
                'k_meta_trajectory': biased}
    return {k: of(lib) for k, lib in libs.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--parent-tree', required=True, help='a built checkout of the parent commit')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--block-ms', type=float, default=200.0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available() and args.rounds >= 5, 'needs the GPU and at least five alternations'
    from fthmc_amd import _lib, ops
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    libs = dict(parent=library(os.path.join(os.path.abspath(args.parent_tree), 'fthmc_amd', 'libfthmc_hip.so')), new=library(_lib.LIB_PATH))
    doc = dict(tool='tools/resident_ab.py', device=torch.cuda.get_device_name(0), rounds=args.rounds, block_ms=args.block_ms,
               libraries={k: l.fthmc_version().decode() for k, l in libs.items()}, rows=[])
    for name, B, L in (('headline', 128, 64), ('config 2', 32, 16)):
        ws = torch.empty(max(ops.meta_ws_bytes(B, L, 1), 8), dtype=torch.uint8, device=dev)
        calls = calls_of(libs, dev, B, L, ws)
        for inst in calls['new']:
            fns = {k: calls[k][inst] for k in ('parent', 'new')}
            for f in fns.values():
                for _ in range(3):
                    f()
            torch.cuda.synchronize()
            n = max(5, int(math.ceil(args.block_ms / max(blocks_of(fns['parent'], 5), 1e-4))))
            t = {k: [] for k in fns}
            for r in range(args.rounds):
                for k in (('parent', 'new') if r % 2 == 0 else ('new', 'parent')):
                    t[k].append(blocks_of(fns[k], n))
            mean = {k: sum(val) / len(val) for k, val in t.items()}
            spread = max(t['parent']) - min(t['parent'])
            doc['rows'].append(dict(shape=name, B=B, L=L, kernel=inst, calls_per_block=n, blocks_us={k: [round(1e3 * b, 4) for b in val] for k, val in t.items()},
                                    mean_us={k: 1e3 * m for k, m in mean.items()}, parent_spread_us=1e3 * spread,
                                    new_minus_parent_us=1e3 * (mean['new'] - mean['parent']), passed=bool(mean['new'] <= mean['parent'] + spread)))
    doc['all_passed'] = all(r['passed'] for r in doc['rows'])
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
