#!/usr/bin/env python3
"""Cost of ftHMC with a defect (fthmc_ft_defect_trajectory_v) next to the flowed trajectory of the parent commit.

    python tools/ft_defect_ab.py --parent-tree DIR [--min-ms 1000] [--bench-steps 100] [--bench-rounds 2] [--out FILE]

With HIP events around repeated calls (at least --min-ms of them per setting, after a warm-up), beta = 6, 10 leapfrog steps of 0.1, a
default-init flow, ladders of K = 8 couplings linear in c and a defect of L / 4 plaquettes, on the latent fields that 50 flowed PTBC
trajectories (a swap round and a translation of the top rung by multiples of 4 behind each) leave from a cold start, at config 2
(32 chains, L = 16, 4 layers: the one-launch kernel) and at the headline (128 chains, L = 64, 8 layers: the sequenced path; one chain
group on either side):
  * five blocks of this build's flowed trajectory with the defect ALTERNATING with five blocks of fthmc_ft_trajectory_int_v (leapfrog,
    the same field, momenta, uniforms and weights, a workspace of its own) from DIR/fthmc_amd/libfthmc_hip.so, the parent commit's
    library loaded next to this one (without --parent-tree: this library's, and the row says so); both enter through the C ABI with a
    stated weights version, so neither expands its weights per call;
  * in the same call what the defect already costs plain HMC in the parent at the same (B, L), on the physical field:
    D = the parent's fthmc_defect_trajectory - the parent's fthmc_hmc_trajectory_pb, alternating blocks -- both one launch (path 1)
    for the one-launch column, both sequenced (path 2 and x_new == x) for the headline column;
  * the criterion: median(defect) <= median(parent) + 2 D + the spread (max - min) of the parent's blocks.  The flowed call adds the
    same launches and the same block sums as the plain one; the factor 2 covers the barriers of a longer kernel and launches inside a
    longer sequence.
--parent-tree DIR also runs `bench.py --gpus 1` of DIR and of this tree alternately (child processes, --bench-rounds of each).
Prints one JSON document (also to --out; default profiles/ft_defect_ab.json) and the table of DESIGN 4.19."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import torch  # noqa: E402

from integrator_ab import make_flow  # noqa: E402
from loops_ab import bench_ab  # noqa: E402
from meta_ab import alternate  # noqa: E402

SEED = 27182
BETA, DT, NSTEP, K = 6.0, 0.1, 10, 8
WVER = 4243
PARENT_CALLS = ('fthmc_ft_trajectory_int_v', 'fthmc_defect_trajectory', 'fthmc_hmc_trajectory_pb')


def parent_library(parent):
    """-> (the parent commit's library typed for the three calls this tool makes, or this one's; label)"""
    from fthmc_amd import _lib
    if parent is None:
        return _lib.load(), 'this library (no --parent-tree)'
    lib = ctypes.CDLL(os.path.join(parent, 'fthmc_amd', 'libfthmc_hip.so'))
    for name in PARENT_CALLS:
        getattr(lib, name).argtypes = _lib.SIGNATURES[name]
    lib.fthmc_ws_bytes.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.fthmc_defect_ws_bytes.argtypes = [ctypes.c_int] * 3
    lib.fthmc_ws_bytes.restype = lib.fthmc_defect_ws_bytes.restype = ctypes.c_size_t
    lib.fthmc_version.restype = ctypes.c_char_p
    return lib, 'parent library ' + lib.fthmc_version().decode()


def ptbc_fields(ops, dev, B, L, nl, w, df):
    """the latent fields and the ladder that 50 flowed PTBC trajectories leave from a cold start -> (x, g_b, acceptance)"""
    M = B // K
    lad = ops.ladder_init([BETA * k / (K - 1) for k in range(K)], M, device=dev)
    g_b, rung, chain_of = lad['beta_b'], lad['rung'], lad['chain_of']
    x, xn = torch.zeros(B, 2, L, L, dtype=torch.float64, device=dev), torch.empty(B, 2, L, L, dtype=torch.float64, device=dev)
    acc = 0.0
    for t in range(50):
        v, u = ops.random_momenta(ops.chain_seeds(SEED, 0, B, t, device=dev), x.shape)
        r = ops.ft_defect_trajectory(x, v, u, w, nl, BETA, g_b, df, DT, NSTEP, out={'x_new': xn})
        us = ops.random_uniform(ops.chain_seeds(SEED + 1, 0, M, t, device=dev), (M, K - 1), 0.0, 1.0)
        ops.replica_swap(lad['betas'], r['dsum'], us, g_b, rung, chain_of, t % 2)
        ush = ops.random_uniform(ops.chain_seeds(SEED + 2, 0, B, t, device=dev), (B, 2), 0.0, 1.0)
        ops.defect_translate(xn, rung, K - 1, (torch.floor(ush * float(L // 4)) * 4.0).to(torch.int32), out=x)
        acc += float(r['acc'].mean()) / 50
    return x, g_b, acc


def rows_for(ops, dev, name, B, L, nl, min_ms, plib):
    from fthmc_amd import _lib
    lib, stream = _lib.load(), torch.cuda.current_stream(dev).cuda_stream
    one = L <= 16
    df = (0, 0, L // 4)
    w = ops.pack_weights(make_flow(torch.Generator().manual_seed(SEED), nl), device=dev)
    x, g_b, acc = ptbc_fields(ops, dev, B, L, nl, w, df)
    v, u = ops.random_momenta(ops.chain_seeds(SEED, 0, B, 1000, device=dev), x.shape)
    vec = lambda: torch.empty(B, dtype=torch.float64, device=dev)
    P = lambda t: t.data_ptr()
    o = {k: vec() for k in ('dH', 'acc', 'H0', 'H1', 'plaq', 'Q', 'dsum')}
    o.update(x_new=torch.empty_like(x), state=torch.empty(4, B, dtype=torch.float64, device=dev))
    ws, nbytes = ops._ws(x, B, L, nl, defect=True)
    args = (P(x), P(v), P(u), P(w), None, nl, B, L, 0, BETA, P(g_b), *df, DT, NSTEP, 0, P(o['x_new']), P(o['dH']), P(o['acc']), P(o['H0']),
            P(o['H1']), P(o['plaq']), P(o['Q']), P(o['dsum']), None, P(o['state']), ws, nbytes, stream, WVER)

    def defect():
        assert lib.fthmc_ft_defect_trajectory_v(*args) == 0
    # the yardstick: the parent's flowed trajectory, a workspace of its own
    po = {k: vec() for k in ('dH', 'acc', 'H0', 'H1', 'plaq', 'Q')}
    po.update(x_new=torch.empty_like(x), state=torch.empty(3, B, dtype=torch.float64, device=dev))
    pws = torch.zeros((int(plib.fthmc_ws_bytes(None, B, L, nl)) + 7) // 8, dtype=torch.float64, device=dev)
    pargs = (P(x), P(v), P(u), P(w), None, nl, B, L, 0, BETA, DT, NSTEP, ops.MODE_MD, P(po['x_new']), P(po['dH']), P(po['acc']), P(po['H0']),
             P(po['H1']), P(po['plaq']), P(po['Q']), None, P(po['state']), P(pws), pws.numel() * 8, stream, 0, WVER)

    def parent():
        assert plib.fthmc_ft_trajectory_int_v(*pargs) == 0
    # what the defect costs plain HMC in the parent at the same (B, L), on the physical field: one launch on either side (path 1), or both
    # sequenced (path 2 / x_new == x)
    y = ops.flow_forward(x, w, nl)[0]
    ya, yb = y.clone(), y.clone()
    bb = torch.full((B,), BETA, dtype=torch.float64, device=dev)
    mo = {k: vec() for k in ('dH', 'acc', 'H0', 'H1', 'csum', 'dsum', 'Q')}
    mo['x_new'] = torch.empty_like(x)
    dws = torch.zeros((int(plib.fthmc_defect_ws_bytes(B, L, 2)) + 7) // 8, dtype=torch.float64, device=dev)
    hws = torch.zeros((int(plib.fthmc_ws_bytes(None, B, L, 0)) + 7) // 8, dtype=torch.float64, device=dev)
    dargs = (P(ya), P(v), P(u), B, L, BETA, P(g_b), *df, DT, NSTEP, 0, 1 if one else 2, P(mo['x_new']) if one else P(ya), P(mo['dH']), P(mo['acc']),
             P(mo['H0']), P(mo['H1']), P(mo['csum']), P(mo['dsum']), P(mo['Q']), P(dws), dws.numel() * 8, stream)
    hargs = (P(yb), P(v), P(u), B, L, P(bb), DT, NSTEP, 0, P(mo['x_new']) if one else P(yb), P(mo['dH']), P(mo['acc']), P(mo['H0']), P(mo['H1']),
             P(hws), hws.numel() * 8, stream)

    def plain_defect():
        assert plib.fthmc_defect_trajectory(*dargs) == 0

    def plain():
        assert plib.fthmc_hmc_trajectory_pb(*hargs) == 0
    t, n = alternate(dict(defect=defect, parent=parent), min_ms, 'defect')
    t2, n2 = alternate(dict(plain_defect=plain_defect, plain=plain), min_ms, 'plain_defect')
    t.update(t2)
    med = {k: statistics.median(val) for k, val in t.items()}
    delta = med['plain_defect'] - med['plain']
    spread = max(t['parent']) - min(t['parent'])
    limit = med['parent'] + 2.0 * delta + spread
    return dict(shape=name, B=B, L=L, n_layers=nl, path='one launch' if one else 'sequenced', defect=df, acceptance=acc, median_ms=med,
                blocks_ms={k: [round(b, 6) for b in val] for k, val in t.items()}, calls_per_block=n, calls_per_block_plain=n2, delta_ms=delta,
                parent_spread_ms=spread, limit_ms=limit, ratio=med['defect'] / med['parent'], passed=bool(med['defect'] <= limit))


def markdown(doc):
    rows = doc['rows']
    head = '| quantity | ' + ' | '.join(f"{r['shape']}, {r['B']} × L = {r['L']}, {r['n_layers']} layers ({r['path']})" for r in rows) + ' |'
    line = lambda name, f: f'| {name} | ' + ' | '.join(f(r) for r in rows) + ' |'
    rng = lambda r, k: f"{r['median_ms'][k]:.4f} ms ({min(r['blocks_ms'][k]):.4f} … {max(r['blocks_ms'][k]):.4f})"
    return '\n'.join([
        head, '|' + '---|' * (len(rows) + 1),
        line('acceptance of the 50 trajectories before', lambda r: f"{r['acceptance']:.2f}"),
        line('flowed trajectory with the defect', lambda r: rng(r, 'defect')),
        line("the parent's `fthmc_ft_trajectory_int_v`", lambda r: rng(r, 'parent')),
        line('ratio', lambda r: f"**{r['ratio']:.3f}**"),
        line("plain HMC in the parent: `defect_trajectory` / `hmc_trajectory_pb`", lambda r: f"{r['median_ms']['plain_defect']:.5f} / {r['median_ms']['plain']:.5f} ms"),
        line('Δ = their difference', lambda r: f"{r['delta_ms'] * 1e3:.2f} µs"),
        line("limit = parent + 2Δ + spread of the parent's blocks", lambda r: f"{r['limit_ms']:.4f} ms"),
        line('criterion: defect ≤ limit', lambda r: '**passed**' if r['passed'] else '**failed**')])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--min-ms', type=float, default=1000.0, help='timed work per setting, at least')
    ap.add_argument('--parent-tree', default=None, help='a built checkout of the parent commit (its library, bench.py A/B)')
    ap.add_argument('--bench-steps', type=int, default=100)
    ap.add_argument('--bench-warmup', type=int, default=10)
    ap.add_argument('--bench-rounds', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ft_defect_ab.json'))
    args = ap.parse_args()
    doc = dict(tool='tools/ft_defect_ab.py')
    parent = os.path.abspath(args.parent_tree) if args.parent_tree else None
    if parent and args.bench_rounds > 0:                                # first, in child processes: this one has not opened the GPU yet
        doc['bench'] = bench_ab(parent, args.bench_steps, args.bench_warmup, args.bench_rounds)
    from fthmc_amd import _lib, ops
    assert torch.cuda.is_available(), 'needs the GPU'
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    plib, label = parent_library(parent)
    doc.update(library=_lib.load().fthmc_version().decode(), device=torch.cuda.get_device_name(0), yardstick=label, rows=[])
    for name, B, L, nl in (('config 2', 32, 16, 4), ('headline', 128, 64, 8)):
        doc['rows'].append(rows_for(ops, dev, name, B, L, nl, args.min_ms, plib))
    doc['markdown'] = markdown(doc)
    text = json.dumps(doc, indent=1, ensure_ascii=False)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(text)
    print(doc['markdown'])


if __name__ == '__main__':
    main()
