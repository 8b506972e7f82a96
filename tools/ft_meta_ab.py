#!/usr/bin/env python3
"""Cost of metadynamics ftHMC (fthmc_ft_meta_trajectory_v) next to the unbiased flowed trajectory of the parent commit.

    python tools/ft_meta_ab.py --parent-tree DIR [--min-ms 1000] [--bench-steps 100] [--bench-rounds 2] [--out FILE]

With HIP events around repeated calls (at least --min-ms of them per setting, after a warm-up), beta = 6, 10 leapfrog steps of 0.1,
a default-init flow, on a latent field and a table left by 100 biased flowed trajectories with deposits (one shared table: nb = 81,
qmax = 4, wall = 50, w = 0.0025) from a cold start, at config 2 (32 chains, L = 16, 4 layers: the one-launch kernel) and at the
headline (128 chains, L = 64, 8 layers: the sequenced path; one chain group on either side):
  * five blocks of this build's biased flowed trajectory ALTERNATING with five blocks of fthmc_ft_trajectory_int_v (leapfrog, the
    same field, momenta, uniforms and weights, a workspace of its own) from DIR/fthmc_amd/libfthmc_hip.so, the parent commit's
    library loaded next to this one (without --parent-tree: this library's, and the row says so); both enter through the C ABI
    with a stated weights version, so neither expands its weights per call;
  * in the same call the per-stage cost the bias already has in plain HMC at the same (B, L):
    d = (fthmc_meta_trajectory - fthmc_hmc_trajectory_int) / stages, both one launch, alternating blocks;
  * the criterion: median(biased) <= median(parent) + (stages + 2) 2 d + the spread (max - min) of the parent's blocks -- two of
    the plain bias's stage costs per sweep (stages force sweeps and two energy sweeps): k_ft_small sums with ft_block_sum on fewer
    threads than k_meta_trajectory's DPP sum, and the sequenced path pays two launches a sweep where the plain one pays none.
--parent-tree DIR also runs `bench.py --gpus 1` of DIR and of this tree alternately (child processes, --bench-rounds of each).
Prints one JSON document (also to --out; default profiles/ft_meta_ab.json) and the table of DESIGN 4.16."""
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

SEED = 31415
NB, QMAX, WALL, W = 81, 4.0, 50.0, 0.0025
BETA, DT, NSTEP = 6.0, 0.1, 10
WVER = 4242


def parent_trajectory(ops, parent, dev):
    """-> (call(x, v, u, w, nl, out), label): fthmc_ft_trajectory_int_v of the parent's library (or this one's), a workspace of its own"""
    from fthmc_amd import _lib
    lib = _lib.load() if parent is None else ctypes.CDLL(os.path.join(parent, 'fthmc_amd', 'libfthmc_hip.so'))
    V, I, Dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    f = lib.fthmc_ft_trajectory_int_v
    if parent is not None:
        f.argtypes = [V, V, V, V, V, I, I, I, I, Dbl, Dbl, I, I] + [V] * 9 + [V, ctypes.c_size_t, V, I, ctypes.c_uint64]
        lib.fthmc_ws_bytes.argtypes = [V, I, I, I]
        lib.fthmc_ws_bytes.restype = ctypes.c_size_t
        lib.fthmc_version.restype = ctypes.c_char_p
    ws = {}

    def call(x, v, u, w, nl, o):
        B, L = x.shape[0], x.shape[2]
        if (B, L, nl) not in ws:
            ws[(B, L, nl)] = torch.zeros((int(lib.fthmc_ws_bytes(None, B, L, nl)) + 7) // 8, dtype=torch.float64, device=dev)
        buf = ws[(B, L, nl)]
        s = torch.cuda.current_stream(dev).cuda_stream
        assert f(x.data_ptr(), v.data_ptr(), u.data_ptr(), w.data_ptr(), None, nl, B, L, 0, BETA, DT, NSTEP, ops.MODE_MD, o['x_new'].data_ptr(),
                 o['dH'].data_ptr(), o['acc'].data_ptr(), o['H0'].data_ptr(), o['H1'].data_ptr(), o['plaq'].data_ptr(), o['Q'].data_ptr(), None,
                 o['state'].data_ptr(), buf.data_ptr(), buf.numel() * 8, s, 0, WVER) == 0
    return call, ('this library (no --parent-tree)' if parent is None else 'parent library ' + lib.fthmc_version().decode())


def rows_for(ops, dev, name, B, L, nl, min_ms, ptraj):
    from fthmc_amd import _lib
    lib, stream = _lib.load(), torch.cuda.current_stream(dev).cuda_stream
    w = ops.pack_weights(make_flow(torch.Generator().manual_seed(SEED), nl), device=dev)
    x, xn = torch.zeros(B, 2, L, L, dtype=torch.float64, device=dev), torch.empty(B, 2, L, L, dtype=torch.float64, device=dev)
    table = torch.zeros(1, NB, dtype=torch.float64, device=dev)
    acc = 0.0
    for t in range(100):                                                 # the field and the table of a short build phase
        seeds = ops.chain_seeds(SEED, 0, B, t, device=dev)
        v, u = ops.random_momenta(seeds, x.shape)
        r = ops.ft_meta_trajectory(x, v, u, w, nl, BETA, DT, NSTEP, table, QMAX, WALL, out={'x_new': xn})
        ops.meta_deposit(r['qm'], table, QMAX, W)
        x, xn = xn, x
        acc += float(r['acc'].mean()) / 100
    v, u = ops.random_momenta(ops.chain_seeds(SEED, 0, B, 1000, device=dev), x.shape)
    vec = lambda: torch.empty(B, dtype=torch.float64, device=dev)
    o = {k: vec() for k in ('dH', 'acc', 'H0', 'H1', 'plaq', 'Q', 'qm', 'vbias')}
    o.update(x_new=torch.empty_like(x), state=torch.empty(4, B, dtype=torch.float64, device=dev))
    po = {k: vec() for k in ('dH', 'acc', 'H0', 'H1', 'plaq', 'Q')}
    po.update(x_new=torch.empty_like(x), state=torch.empty(3, B, dtype=torch.float64, device=dev))
    ws, nbytes = ops._ws(x, B, L, nl, meta=True)
    args = (x.data_ptr(), v.data_ptr(), u.data_ptr(), w.data_ptr(), None, nl, B, L, 0, BETA, DT, NSTEP, 0, table.data_ptr(), 1, NB, QMAX, WALL,
            o['x_new'].data_ptr(), o['dH'].data_ptr(), o['acc'].data_ptr(), o['H0'].data_ptr(), o['H1'].data_ptr(), o['plaq'].data_ptr(),
            o['Q'].data_ptr(), o['qm'].data_ptr(), o['vbias'].data_ptr(), None, o['state'].data_ptr(), ws, nbytes, stream, WVER)

    def biased():
        assert lib.fthmc_ft_meta_trajectory_v(*args) == 0
    # the plain bias at the same (B, L): the physical field, one launch on either side
    y = ops.flow_forward(x, w, nl)[0]
    mo = {k: vec() for k in ('dH', 'acc', 'H0', 'H1', 'qm', 'vbias')}
    mo['x_new'] = torch.empty_like(x)
    margs = (y.data_ptr(), v.data_ptr(), u.data_ptr(), B, L, BETA, DT, NSTEP, 0, table.data_ptr(), 1, NB, QMAX, WALL, 1, mo['x_new'].data_ptr(),
             mo['dH'].data_ptr(), mo['acc'].data_ptr(), mo['H0'].data_ptr(), mo['H1'].data_ptr(), mo['qm'].data_ptr(), mo['vbias'].data_ptr(), None, 0, stream)
    hargs = (y.data_ptr(), v.data_ptr(), u.data_ptr(), B, L, BETA, DT, NSTEP, 0, mo['x_new'].data_ptr(), mo['dH'].data_ptr(), mo['acc'].data_ptr(),
             mo['H0'].data_ptr(), mo['H1'].data_ptr(), None, 0, stream)

    def plain_biased():
        assert lib.fthmc_meta_trajectory(*margs) == 0

    def plain():
        assert lib.fthmc_hmc_trajectory_int(*hargs) == 0
    t, n = alternate(dict(biased=biased, parent=lambda: ptraj(x, v, u, w, nl, po)), min_ms, 'biased')
    t2, n2 = alternate(dict(plain_biased=plain_biased, plain=plain), min_ms, 'plain_biased')
    t.update(t2)
    med = {k: statistics.median(val) for k, val in t.items()}
    stages = ops.integrator_forces('leapfrog', NSTEP)
    d = (med['plain_biased'] - med['plain']) / stages
    spread = max(t['parent']) - min(t['parent'])
    limit = med['parent'] + (stages + 2) * 2.0 * d + spread
    tab = table.cpu().numpy()
    return dict(shape=name, B=B, L=L, n_layers=nl, path='one launch' if L <= 16 else 'sequenced', table_range=float(tab.max() - tab.min()),
                acceptance=acc, median_ms=med, blocks_ms={k: [round(b, 6) for b in val] for k, val in t.items()}, calls_per_block=n, calls_per_block_plain=n2, stages=stages,
                d_ms=d, parent_spread_ms=spread, limit_ms=limit, ratio=med['biased'] / med['parent'], passed=bool(med['biased'] <= limit))


def markdown(doc):
    rows = doc['rows']
    head = '| quantity | ' + ' | '.join(f"{r['shape']}, {r['B']} × L = {r['L']}, {r['n_layers']} layers ({r['path']})" for r in rows) + ' |'
    line = lambda name, f: f'| {name} | ' + ' | '.join(f(r) for r in rows) + ' |'
    rng = lambda r, k: f"{r['median_ms'][k]:.4f} ms ({min(r['blocks_ms'][k]):.4f} … {max(r['blocks_ms'][k]):.4f})"
    return '\n'.join([
        head, '|' + '---|' * (len(rows) + 1),
        line('table range / acceptance after the build', lambda r: f"{r['table_range']:.2f} / {r['acceptance']:.2f}"),
        line('biased flowed trajectory', lambda r: rng(r, 'biased')),
        line("the parent's `fthmc_ft_trajectory_int_v`", lambda r: rng(r, 'parent')),
        line('ratio', lambda r: f"**{r['ratio']:.3f}**"),
        line('plain HMC: `meta_trajectory` / `hmc_trajectory_int`', lambda r: f"{r['median_ms']['plain_biased']:.5f} / {r['median_ms']['plain']:.5f} ms"),
        line('d = their difference per stage', lambda r: f"{r['d_ms'] * 1e3:.3f} µs ({r['stages']} stages)"),
        line("limit = parent + (stages + 2)·2d + spread of the parent's blocks", lambda r: f"{r['limit_ms']:.4f} ms"),
        line('criterion: biased ≤ limit', lambda r: '**passed**' if r['passed'] else '**failed**')])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--min-ms', type=float, default=1000.0, help='timed work per setting, at least')
    ap.add_argument('--parent-tree', default=None, help='a built checkout of the parent commit (its flowed trajectory, bench.py A/B)')
    ap.add_argument('--bench-steps', type=int, default=100)
    ap.add_argument('--bench-warmup', type=int, default=10)
    ap.add_argument('--bench-rounds', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ft_meta_ab.json'))
    args = ap.parse_args()
    doc = dict(tool='tools/ft_meta_ab.py')
    parent = os.path.abspath(args.parent_tree) if args.parent_tree else None
    if parent and args.bench_rounds > 0:                                # first, in child processes: this one has not opened the GPU yet
        doc['bench'] = bench_ab(parent, args.bench_steps, args.bench_warmup, args.bench_rounds)
    from fthmc_amd import _lib, ops
    assert torch.cuda.is_available(), 'needs the GPU'
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    ptraj, label = parent_trajectory(ops, parent, dev)
    doc.update(library=_lib.load().fthmc_version().decode(), device=torch.cuda.get_device_name(0), yardstick=label, rows=[])
    for name, B, L, nl in (('config 2', 32, 16, 4), ('headline', 128, 64, 8)):
        doc['rows'].append(rows_for(ops, dev, name, B, L, nl, args.min_ms, ptraj))
    doc['markdown'] = markdown(doc)
    text = json.dumps(doc, indent=1, ensure_ascii=False)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(text)
    print(doc['markdown'])


if __name__ == '__main__':
    main()
