#!/usr/bin/env python3
"""Writes tests/golden/ws_sizes.json: what every workspace size query of libfthmc_hip.so answers over a grid of net shapes and
(B, L, n_layers).  The committed file was recorded from the library of the commit before csrc/api.hip was split into api_call.h /
api.hip / api_second_order.hip / api_diag.hip, so that tests/test_ws_sizes.py holds the layouts to the sizes they had: the scratch
contract tests run in scratch of exactly the queried size, and a query and a layout that shrank together would pass them.  The
metadynamics columns (fthmc_meta_ws_bytes on its three paths, fthmc_ft_meta_ws_bytes) were recorded from the library of the commit
before their two layouts became one (meta_layout).

    python tests/golden/make_ws_sizes.py [path/to/libfthmc_hip.so]      (default: the library of this tree)

No GPU is needed: the queries are host arithmetic."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

BS = (1, 3, 64, 65, 1 << 20)
LS = (4, 8, 16, 20, 64, 68, 132, 256)
NLS = (0, 1, 8, 64, 65, 66)
COLUMNS = ('ws', 'train_ws', 'vjp_ws', 'force_ws_path0', 'force_ws_path1', 'force_ws_path2', 'force_ws_path3', 'layer_stash_valu',
           'layer_stash_mfma', 'meta_ws_path0', 'meta_ws_path1', 'meta_ws_path2', 'ft_meta_ws')


def archs():
    """the default net (None) and the net shapes of tests/net_shape_cases.py, as fthmc_amd.ops names them"""
    import net_shape_cases as NS
    return [None] + [NS.arch(c) for c in NS.CASES]


def grid():
    """[(arch index, B, L, n_layers)]: the default net on every other point of the product, each further net shape on a twelfth of
    it, shifted from shape to shape -- every B, L and n_layers meets every shape's neighbours, in a few hundred rows"""
    out = []
    for ia in range(len(archs())):
        for ib, B in enumerate(BS):
            for il, L in enumerate(LS):
                for inl, nl in enumerate(NLS):
                    if (ib + il + inl) % 2 == 0 if ia == 0 else (ib + 2 * il + 3 * inl + ia) % 12 == 0:
                        out.append((ia, B, L, nl))
    return out


def query(lib, ops, arch, B, L, nl):
    """the COLUMNS of one grid point; leaves the variant and the dual path as it found them"""
    ap = ops._arch(arch)
    row = [int(lib.fthmc_ws_bytes(ap, B, L, nl)), int(lib.fthmc_train_ws_bytes(ap, B, L, nl)), int(lib.fthmc_vjp_ws_bytes(ap, B, L, nl))]
    path, variant = lib.fthmc_get_dual_path(), lib.fthmc_get_variant()
    try:
        for p in range(4):
            assert lib.fthmc_set_dual_path(p) == 0
            row.append(int(lib.fthmc_train_force_ws_bytes(ap, B, L, nl)))
        for v in (0, 1):
            assert lib.fthmc_set_variant(v) == 0
            row.append(int(lib.fthmc_layer_stash_bytes(ap, B, L)))
    finally:
        lib.fthmc_set_dual_path(path)
        lib.fthmc_set_variant(variant)
    row += [int(lib.fthmc_meta_ws_bytes(B, L, p)) for p in range(3)]              # no net, no layers: the same on every row of a (B, L)
    row.append(int(lib.fthmc_ft_meta_ws_bytes(ap, B, L, nl)))
    return row


def record(lib, ops):
    A = archs()
    return {'head_bytes': int(lib.fthmc_ws_head_bytes()), 'archs': A, 'columns': ['arch', 'B', 'L', 'n_layers'] + list(COLUMNS),
            'rows': [[ia, B, L, nl] + query(lib, ops, A[ia], B, L, nl) for ia, B, L, nl in grid()]}


if __name__ == '__main__':
    from fthmc_amd import _lib, ops
    lib = _lib.load(*sys.argv[1:2])
    doc = record(lib, ops)
    with open(os.path.join(HERE, 'ws_sizes.json'), 'w') as f:
        f.write('{"head_bytes": %d,\n "archs": %s,\n "columns": %s,\n "rows": [\n  ' % (
            doc['head_bytes'], json.dumps(doc['archs']), json.dumps(doc['columns'])))
        f.write(',\n  '.join(json.dumps(r) for r in doc['rows']))
        f.write('\n ]}\n')
    print(len(doc['rows']), 'rows from', lib.fthmc_version().decode())
