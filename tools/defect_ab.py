#!/usr/bin/env python3
"""Cost of boundary-condition tempering (fthmc_defect_*, csrc/defect.hip) next to the per-chain-beta trajectory of the parent commit.

    python tools/defect_ab.py --parent-lib FILE [--min-ms 1000] [--ntraj 200] [--out FILE]

With HIP events around repeated calls (at least --min-ms of them per setting, after a warm-up), at the headline batch (128 chains,
L = 64: 16 ladders of 8 rungs) and at config 2's shape (32 chains, L = 16: 4 ladders), beta = 6, 10 leapfrog steps of 0.1, c linear in
[0, 1], the default defect (0, 0, L / 4), on the fields, couplings and rungs 50 PTBC trajectories from a cold start leave:
  * the trajectory with a defect on the one-launch path and on the sequenced path, into preallocated outputs, through the C ABI;
  * five blocks of the one-launch trajectory with a defect ALTERNATING with five blocks of fthmc_hmc_trajectory_pb (beta_b = beta,
    leapfrog, the same field, momenta and uniforms: its one-launch kernel k_hmc_trajectory_sched<true>) from FILE, the parent commit's
    library loaded next to this one (without --parent-lib: this library's, and the document says so), and with five blocks of this
    library's biased trajectory under a zero table (k_meta_trajectory: the yardstick of DESIGN 4.15's overhead figure);
  * the translation and one swap round, each alternating with the one-launch trajectory;
  * run_ptbc against run_tempered(flow=None) over a ladder of beta of the same batch, --ntraj captured trajectories each, three runs of
    each in alternation, wall clock per trajectory (the whole driver: random numbers, swap round, translation, history rows).
Prints one JSON document (also to --out)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import torch  # noqa: E402

from loops_ab import timed  # noqa: E402
from meta_ab import alternate  # noqa: E402

SEED = 31415
BETA, DT, NSTEP, K = 6.0, 0.1, 10, 8
CS = [k / (K - 1) for k in range(K - 1)] + [1.0]


def parent_pb(ops, path):
    """-> (trajectory(x, v, u, beta_b, out), label): fthmc_hmc_trajectory_pb of the parent's library, or of this one"""
    from fthmc_amd import _lib
    if path is None:
        lib, label = _lib.load(), 'this library (no --parent-lib)'
    else:
        lib = ctypes.CDLL(os.path.abspath(path))
        V, I, Dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
        lib.fthmc_hmc_trajectory_pb.argtypes = [V, V, V, I, I, V, Dbl, I, I, V, V, V, V, V, V, ctypes.c_size_t, V]
        lib.fthmc_version.restype = ctypes.c_char_p
        label = 'parent library ' + lib.fthmc_version().decode()

    def traj(x, v, u, bb, o):                     # L <= 64 with x_new != x: one launch, no workspace
        s = torch.cuda.current_stream(x.device).cuda_stream
        assert lib.fthmc_hmc_trajectory_pb(x.data_ptr(), v.data_ptr(), u.data_ptr(), x.shape[0], x.shape[2], bb.data_ptr(), DT, NSTEP, 0,
                                           o['x_new'].data_ptr(), o['dH'].data_ptr(), o['acc'].data_ptr(), o['H0'].data_ptr(),
                                           o['H1'].data_ptr(), None, 0, s) == 0
    return traj, label


def param(L):
    from fthmc_amd.config import Param
    return Param(beta=BETA, L=L, tau=DT * NSTEP, nstep=NSTEP, seed=SEED)


def rows_for(ops, dev, name, B, L, min_ms, ntraj, ptraj):
    from fthmc_amd import _lib
    from fthmc_amd.defect import default_defect, run_ptbc
    from fthmc_amd.tempering import run_tempered
    M, df = B // K, default_defect(L)
    h = run_ptbc(param(L), CS, M, 50, defect=df)
    x, g_b, rung = h['x'], h['g_b'], h['rung_last']
    seeds = ops.chain_seeds(SEED, 0, B, 1000, device=dev)
    v, u = ops.random_momenta(seeds, x.shape)
    vec = lambda: torch.empty(B, dtype=torch.float64, device=dev)
    o = {k: vec() for k in ('dH', 'acc', 'H0', 'H1', 'csum', 'dsum', 'Q')}
    o['x_new'] = torch.empty_like(x)
    po = {k: vec() for k in ('dH', 'acc', 'H0', 'H1')}
    po['x_new'] = torch.empty_like(x)
    mo = {k: vec() for k in ('dH', 'acc', 'H0', 'H1', 'qm', 'vbias')}
    mo['x_new'] = torch.empty_like(x)
    bb = torch.full((B,), BETA, dtype=torch.float64, device=dev)
    table = torch.zeros(1, 81, dtype=torch.float64, device=dev)
    rows = [dict(shape=name, B=B, L=L, ladders=M, defect=list(df), kind='fields after 50 PTBC trajectories', acceptance=float(h['acc'].mean()),
                 swap_acc=[round(float(a), 3) for a in h['swap_acc']])]
    lib, stream = _lib.load(), torch.cuda.current_stream(dev).cuda_stream

    def defect(path):                             # through the C ABI with the arguments ready, as the parent's side enters
        need = ops.defect_ws_bytes(B, L, path)
        ws, nbytes = ops._stream_buffer(x, need, 'defect') if need else (None, 0)
        args = (x.data_ptr(), v.data_ptr(), u.data_ptr(), B, L, BETA, g_b.data_ptr(), *df, DT, NSTEP, 0, path, o['x_new'].data_ptr(),
                *(o[k].data_ptr() for k in ('dH', 'acc', 'H0', 'H1', 'csum', 'dsum', 'Q')), ws, nbytes, stream)

        def call():
            assert lib.fthmc_defect_trajectory(*args) == 0
        return call
    for path, pname in ((1, 'one launch'), (2, 'sequenced')):
        ms, blocks, calls = timed(defect(path), min_ms)
        rows.append(dict(shape=name, B=B, L=L, kind='trajectory with a defect', path=pname, ms_per_call=ms, ms_min=min(blocks), ms_max=max(blocks), calls=calls))
    meta_args = (x.data_ptr(), v.data_ptr(), u.data_ptr(), B, L, BETA, DT, NSTEP, 0, table.data_ptr(), 1, 81, 4.0, 0.0, 1, mo['x_new'].data_ptr(),
                 *(mo[k].data_ptr() for k in ('dH', 'acc', 'H0', 'H1', 'qm', 'vbias')), None, 0, stream)

    def meta():
        assert lib.fthmc_meta_trajectory(*meta_args) == 0
    fns = dict(defect=defect(1), parent_pb=lambda: ptraj(x, v, u, bb, po), meta_zero_table=meta)
    t, n = alternate(fns, min_ms, 'defect')
    med = {k: statistics.median(val) for k, val in t.items()}
    rows.append(dict(shape=name, B=B, L=L, kind='one-launch trajectory with a defect against the per-chain-beta one and the biased one, alternating blocks',
                     median_ms=med, blocks_ms={k: [round(b, 6) for b in val] for k, val in t.items()}, ratio_to_parent=med['defect'] / med['parent_pb'],
                     meta_ratio_to_parent=med['meta_zero_table'] / med['parent_pb'], calls_per_block=n))
    # the translation and a swap round next to a trajectory
    shift = torch.randint(0, L, (B, 2), dtype=torch.int32, device=dev)
    xt = torch.empty_like(x)
    lad = ops.ladder_init([BETA * c for c in CS], M, device=dev)
    us = torch.rand(M, K - 1, dtype=torch.float64, device=dev)
    so = {'swap_acc': torch.empty(M, K - 1, dtype=torch.float64, device=dev), 'd': torch.empty(M, K - 1, dtype=torch.float64, device=dev)}
    dsum = o['dsum']
    fns = dict(trajectory=defect(1), translate=lambda: ops.defect_translate(x, rung, K - 1, shift, out=xt),
               swap_round=lambda: ops.replica_swap(lad['betas'], dsum, us, lad['beta_b'], lad['rung'], lad['chain_of'], 0, out=so))
    t, n = alternate(fns, min_ms, 'trajectory')
    rows.append(dict(shape=name, B=B, L=L, kind='the translation and a swap round next to the one-launch trajectory, alternating blocks (through ops)',
                     median_ms={k: statistics.median(val) for k, val in t.items()},
                     blocks_ms={k: [round(b, 6) for b in val] for k, val in t.items()}, calls_per_block=n))
    # the drivers
    betas = [BETA - 0.25 * (K - 1 - k) for k in range(K)]
    wall = {'run_ptbc': [], 'run_tempered': []}
    for _ in range(3):
        for key, run in (('run_ptbc', lambda: run_ptbc(param(L), CS, M, ntraj, defect=df)),
                         ('run_tempered', lambda: run_tempered(param(L), None, betas, M, ntraj))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hh = run()
            hh['x']                                # reads the history back: the loop has ended
            torch.cuda.synchronize()
            wall[key].append((time.perf_counter() - t0) * 1e3 / ntraj)
    med = {k: statistics.median(val) for k, val in wall.items()}
    rows.append(dict(shape=name, B=B, L=L, kind=f'run_ptbc against run_tempered(flow=None), {ntraj} captured trajectories, wall clock per trajectory',
                     median_ms=med, runs_ms={k: [round(b, 6) for b in val] for k, val in wall.items()}, ratio=med['run_ptbc'] / med['run_tempered']))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--min-ms', type=float, default=1000.0, help='timed work per setting, at least')
    ap.add_argument('--parent-lib', default=None, help="the parent commit's libfthmc_hip.so (the per-chain-beta trajectory)")
    ap.add_argument('--ntraj', type=int, default=200)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from fthmc_amd import _lib, ops
    assert torch.cuda.is_available(), 'needs the GPU'
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    ptraj, label = parent_pb(ops, args.parent_lib)
    doc = dict(tool='tools/defect_ab.py', library=_lib.load().fthmc_version().decode(), device=torch.cuda.get_device_name(0), yardstick=label, rows=[])
    for name, B, L in (('headline', 128, 64), ('config 2', 32, 16)):
        doc['rows'] += rows_for(ops, dev, name, B, L, args.min_ms, args.ntraj, ptraj)
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
