#!/usr/bin/env python3
"""Cost of metadynamics HMC (fthmc_meta_*, csrc/meta.hip) next to the plain trajectory of the parent commit.

    python tools/meta_ab.py --parent-tree DIR [--min-ms 1000] [--bench-steps 100] [--bench-rounds 2] [--out FILE]

With HIP events around repeated calls (at least --min-ms of them per setting, after a warm-up), at the headline batch (128 chains,
L = 64) and at config 2 (32 chains, L = 16), beta = 6, 10 leapfrog steps of 0.1, on a field and a table left by 200 biased
trajectories with deposits (one shared table: nb = 81, qmax = 4, wall = 50, w = 0.0025) from a cold start:
  * the biased trajectory on the one-launch path and on the sequenced path, into preallocated outputs;
  * the criterion: five blocks of the biased one-launch trajectory ALTERNATING with five blocks of the plain trajectory
    (fthmc_hmc_trajectory_int, leapfrog, the same field, momenta and uniforms) from DIR/fthmc_amd/libfthmc_hip.so, the parent commit's
    library loaded next to this one (without --parent-tree: this library's, and the row says so);
    pass = median(biased) <= 2 x median(parent) + the spread (max - min) of the parent's blocks.
    (The 2: a stage goes from two barrier phases to at most four -- the block sum -- and adds no pass over memory.)
  * one meta_deposit call at B = 128 and B = 4096 walkers on one shared table of nb = 81, alternating with the parent's
    wilson_action_charge at the headline batch.
--parent-tree DIR also runs `bench.py --gpus 1` of DIR and of this tree alternately (child processes, --bench-rounds of each), their
result lines side by side: only a translation unit was added, they must agree.
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
from loops_ab import bench_ab, timed  # noqa: E402

SEED = 27182
NB, QMAX, WALL, W = 81, 4.0, 50.0, 0.0025
BETA, DT, NSTEP = 6.0, 0.1, 10


def parent_calls(ops, parent):
    """-> (trajectory(x, v, u, out), action_charge(x, obs), label): the parent library's entry points, or this one's"""
    if parent is None:
        return (lambda x, v, u, o: ops.hmc_trajectory(x, v, u, BETA, DT, NSTEP, out=o)), (lambda x, o: ops.wilson_action_charge(x, BETA, out=o)), \
            'this library (no --parent-tree)'
    lib = ctypes.CDLL(os.path.join(parent, 'fthmc_amd', 'libfthmc_hip.so'))
    V, I, Dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.fthmc_hmc_trajectory_int.argtypes = [V, V, V, I, I, Dbl, Dbl, I, I, V, V, V, V, V, V, ctypes.c_size_t, V]
    lib.fthmc_wilson_action_charge.argtypes = [V, I, I, Dbl, V, V, V, V]
    lib.fthmc_version.restype = ctypes.c_char_p

    def traj(x, v, u, o):                         # L <= 64 with x_new != x: one launch, no workspace
        s = torch.cuda.current_stream(x.device).cuda_stream
        assert lib.fthmc_hmc_trajectory_int(x.data_ptr(), v.data_ptr(), u.data_ptr(), x.shape[0], x.shape[2], BETA, DT, NSTEP, 0,
                                            o['x_new'].data_ptr(), o['dH'].data_ptr(), o['acc'].data_ptr(), o['H0'].data_ptr(),
                                            o['H1'].data_ptr(), None, 0, s) == 0

    def action(x, o):
        s = torch.cuda.current_stream(x.device).cuda_stream
        assert lib.fthmc_wilson_action_charge(x.data_ptr(), x.shape[0], x.shape[2], BETA, o['S'].data_ptr(), o['Q'].data_ptr(), o['plaq'].data_ptr(), s) == 0
    return traj, action, 'parent library ' + lib.fthmc_version().decode()


def alternate(fns, min_ms, first):
    """five blocks of every fn in turn -> (blocks, calls per block)"""
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    n = max(5, int(math.ceil(min_ms / 5 / max(blocks_of(fns[first], 5), 1e-3))))
    t = {k: [] for k in fns}
    for _ in range(5):
        for k, f in fns.items():
            t[k].append(blocks_of(f, n))
    return t, n


def built(ops, dev, B, L):
    """the field and the table 200 biased trajectories with deposits leave, from a cold start"""
    x, xn = torch.zeros(B, 2, L, L, dtype=torch.float64, device=dev), torch.empty(B, 2, L, L, dtype=torch.float64, device=dev)
    table = torch.zeros(1, NB, dtype=torch.float64, device=dev)
    acc = 0.0
    for t in range(200):
        seeds = ops.chain_seeds(SEED, 0, B, t, device=dev)
        v, u = ops.random_momenta(seeds, x.shape)
        r = ops.meta_trajectory(x, v, u, BETA, DT, NSTEP, table, QMAX, WALL, out={'x_new': xn})
        ops.meta_deposit(r['qm'], table, QMAX, W)
        x, xn = xn, x
        acc += float(r['acc'].mean())
    return x, table, acc / 200


def rows_for(ops, dev, name, B, L, min_ms, parent_traj):
    x, table, acc = built(ops, dev, B, L)
    seeds = ops.chain_seeds(SEED, 0, B, 1000, device=dev)
    v, u = ops.random_momenta(seeds, x.shape)
    vec = lambda: torch.empty(B, dtype=torch.float64, device=dev)
    o = {k: vec() for k in ('dH', 'acc', 'H0', 'H1', 'qm', 'vbias')}
    o['x_new'] = torch.empty_like(x)
    po = {k: vec() for k in ('dH', 'acc', 'H0', 'H1')}
    po['x_new'] = torch.empty_like(x)
    tab = table.cpu().numpy()
    rows = [dict(shape=name, B=B, L=L, kind='table after 200 biased trajectories with deposits', table_range=float(tab.max() - tab.min()),
                 acceptance=acc)]
    # both sides of the comparison enter through the C ABI with their arguments ready (the parent's has no wrapper here): at config 2 the
    # checks of ops.meta_trajectory cost the host more than the kernel costs the device
    from fthmc_amd import _lib
    lib, stream = _lib.load(), torch.cuda.current_stream(dev).cuda_stream

    def biased(path):
        need = ops.meta_ws_bytes(B, L, path)
        ws, nbytes = ops._meta_ws(x, need)
        args = (x.data_ptr(), v.data_ptr(), u.data_ptr(), B, L, BETA, DT, NSTEP, 0, table.data_ptr(), 1, NB, QMAX, WALL, path, o['x_new'].data_ptr(),
                o['dH'].data_ptr(), o['acc'].data_ptr(), o['H0'].data_ptr(), o['H1'].data_ptr(), o['qm'].data_ptr(), o['vbias'].data_ptr(), ws, nbytes,
                stream)

        def call():
            assert lib.fthmc_meta_trajectory(*args) == 0
        return call
    for path, pname in ((1, 'one launch'), (2, 'sequenced')):
        ms, blocks, calls = timed(biased(path), min_ms)
        rows.append(dict(shape=name, B=B, L=L, kind='biased trajectory', path=pname, ms_per_call=ms, ms_min=min(blocks), ms_max=max(blocks), calls=calls))
    ms, blocks, calls = timed(lambda: ops.meta_trajectory(x, v, u, BETA, DT, NSTEP, table, QMAX, WALL, path=1, out=o), min_ms)
    rows.append(dict(shape=name, B=B, L=L, kind='biased trajectory through ops.meta_trajectory (host-bound where the kernel is shorter than the wrapper)',
                     path='one launch', ms_per_call=ms, ms_min=min(blocks), ms_max=max(blocks), calls=calls))
    fns = dict(biased=biased(1), parent=lambda: parent_traj(x, v, u, po))
    t, n = alternate(fns, min_ms, 'biased')
    med = {k: statistics.median(val) for k, val in t.items()}
    limit = 2.0 * med['parent'] + (max(t['parent']) - min(t['parent']))
    rows.append(dict(shape=name, B=B, L=L, kind='biased one-launch trajectory against the plain one, alternating blocks', median_ms=med,
                     blocks_ms={k: [round(b, 6) for b in val] for k, val in t.items()}, ratio=med['biased'] / med['parent'], limit_ms=limit,
                     calls_per_block=n, passed=bool(med['biased'] <= limit)))
    return rows


def deposit_rows(ops, dev, min_ms, parent_action):
    gen = torch.Generator().manual_seed(SEED)
    x = ((torch.rand(128, 2, 64, 64, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi).to(dev)
    obs = {k: torch.empty(128, dtype=torch.float64, device=dev) for k in ('S', 'Q', 'plaq')}
    rows = []
    for B in (128, 4096):
        qm = ((torch.rand(B, generator=gen, dtype=torch.float64) * 2 - 1) * 3.0).to(dev)
        table = torch.zeros(1, NB, dtype=torch.float64, device=dev)
        t, n = alternate(dict(deposit=lambda: ops.meta_deposit(qm, table, QMAX, W), action_charge=lambda: parent_action(x, obs)), min_ms, 'deposit')
        rows.append(dict(kind='meta_deposit, one shared table of nb = 81, against wilson_action_charge at 128 x L = 64, alternating blocks', walkers=B,
                         median_ms={k: statistics.median(val) for k, val in t.items()},
                         blocks_ms={k: [round(b, 6) for b in val] for k, val in t.items()}, calls_per_block=n))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--min-ms', type=float, default=1000.0, help='timed work per setting, at least')
    ap.add_argument('--parent-tree', default=None, help='a built checkout of the parent commit (the plain trajectory, bench.py A/B)')
    ap.add_argument('--bench-steps', type=int, default=100)
    ap.add_argument('--bench-warmup', type=int, default=10)
    ap.add_argument('--bench-rounds', type=int, default=2)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    doc = dict(tool='tools/meta_ab.py')
    parent = os.path.abspath(args.parent_tree) if args.parent_tree else None
    if parent and args.bench_rounds > 0:                                # first, in child processes: this one has not opened the GPU yet
        doc['bench'] = bench_ab(parent, args.bench_steps, args.bench_warmup, args.bench_rounds)
    from fthmc_amd import _lib, ops
    assert torch.cuda.is_available(), 'needs the GPU'
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    ptraj, paction, label = parent_calls(ops, parent)
    doc.update(library=_lib.load().fthmc_version().decode(), device=torch.cuda.get_device_name(0), yardstick=label, rows=[])
    for name, B, L in (('headline', 128, 64), ('config 2', 32, 16)):
        doc['rows'] += rows_for(ops, dev, name, B, L, args.min_ms, ptraj)
    doc['deposit'] = deposit_rows(ops, dev, args.min_ms, paction)
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
