"""CPU: the workspace size queries of include/fthmc_hip.h at every case of tests/workspace_cases.py, and that the case table
reaches what it claims.  The size queries are host code (tests/test_index_limits.py calls the library the same way); nothing here
needs a GPU.

Sizes: multiples of 256 bytes, the same when asked twice, independent of fthmc_set_variant / fthmc_set_small_path /
fthmc_set_dual_path -- but for fthmc_train_force_ws_bytes, which follows the dual path and nothing else: with the plain dual
kernels it is the first-order workspace, the force and the regions of fthmc_vjp_ws_bytes behind its head, to the byte; with a
setting under which fthmc_train_force_path says the plain kernels serve the shape it is that same size.  The training and the
force-training workspaces hold a first-order one, and the head is at most every first-order size.

The table: 'small', 'fused' and 'two-kernel' training launches, a launch in which a workgroup of k_flow_wgrad and of
k_flow_bwd_train walks more than one item (tests/walk_model.py), ragged and exact lattices, a flow deeper than the head.  The
65-layer case is held to the oracle at 1e-9 on the GPU; here its conditioning is asserted the way tests/test_first_order_hard.py
does: pytest -s prints the figure (scale 1: 1.7e-14 at worst, S_eff of chain 0, against SENS_BOUND = 1e-12)."""
import itertools

import pytest
import torch

import first_order_cases as FC
import walk_model as M
import workspace_cases as W
from conftest import ROOT  # noqa: F401
from fthmc_amd import _lib, ops

DEFAULT_CASES = [c for c in W.CASES if c.arch is None]


@pytest.fixture()
def lib():
    lib = _lib.load()
    saved = lib.fthmc_get_variant(), lib.fthmc_get_small_path(), lib.fthmc_get_dual_path()
    yield lib
    assert lib.fthmc_set_variant(saved[0]) == 0 and lib.fthmc_set_small_path(saved[1]) == 0 and lib.fthmc_set_dual_path(saved[2]) == 0


def queries(lib, c):
    """every size query at the case -> {name: bytes}"""
    a = ops._arch(c.arch)
    return {'ws': lib.fthmc_ws_bytes(a, c.B, c.L, c.nl), 'train_ws': lib.fthmc_train_ws_bytes(a, c.B, c.L, c.nl),
            'ws_one_layer': lib.fthmc_ws_bytes(a, c.B, c.L, 1), 'train_ws_one_layer': lib.fthmc_train_ws_bytes(a, c.B, c.L, 1),
            'ws_plain': lib.fthmc_ws_bytes(None, c.B, c.L, 0),
            'vjp_ws': lib.fthmc_vjp_ws_bytes(a, c.B, c.L, c.nl), 'train_force_ws': lib.fthmc_train_force_ws_bytes(a, c.B, c.L, c.nl),
            'wilson_loops_ws': lib.fthmc_wilson_loops_ws_bytes(c.B, c.L, max(1, c.L // 2), c.L),
            'instanton_ws': lib.fthmc_instanton_ws_bytes(c.B, c.L, 2)}


@pytest.mark.parametrize('case', W.CASES, ids=[c.name for c in W.CASES])
def test_size_queries(lib, case):
    head = lib.fthmc_ws_head_bytes()
    assert head % 256 == 0 and head > 0
    base, force = None, {}
    for variant, small, dual in itertools.product((1, 0), (1, 0), (1, 0, 2, 3)):
        assert lib.fthmc_set_variant(variant) == 0 and lib.fthmc_set_small_path(small) == 0 and lib.fthmc_set_dual_path(dual) == 0
        q = queries(lib, case)
        assert q == queries(lib, case), 'asked twice'
        tf = q.pop('train_force_ws')
        force.setdefault(dual, (tf, lib.fthmc_train_force_path(ops._arch(case.arch), case.B, case.L)))
        assert force[dual][0] == tf, f'fthmc_train_force_ws_bytes moves with variant {variant} / small path {small}'
        base = q if base is None else base
        assert q == base, f'a size moves with variant {variant} / small path {small} / dual path {dual}'
    for name, n in dict(base, **{f'train_force_ws_dual{d}': v[0] for d, v in force.items()}).items():
        assert n > 0 and n % 256 == 0, (name, n)
    assert base['train_ws'] >= base['ws'] >= head and base['train_ws_one_layer'] >= base['ws_one_layer'] >= head
    assert base['ws_plain'] >= head and base['vjp_ws'] > head
    # force training: a first-order workspace first; with the plain dual kernels then the force and the regions of the second-order
    # layout that lie behind its head, to the byte; any setting that leaves the shape to the plain kernels asks for the same
    n2 = 8 * 2 * case.B * case.L * case.L
    plain = base['ws'] + (n2 + 255) // 256 * 256 + base['vjp_ws'] - head
    assert force[0] == (plain, 0), (force[0], plain)
    for dual, (n, path) in force.items():
        assert n >= base['ws'] and path in (0, 1)
        assert path == 1 or n == plain, (dual, n, plain)
        assert path == 0 or case.arch is None, 'the fused dual kernels serve the default net only'


def test_the_table_reaches_what_it_claims():
    paths = {M.train_launch(c.B, c.L, c.nl)[0] for c in DEFAULT_CASES if c.nl >= 1}
    assert paths == {'small', 'fused', 'two-kernel'}, paths
    assert {c.L for c in DEFAULT_CASES if M.ft_small_shape(c.L, c.nl)} == {8, 12, 16}
    assert any(c.L % 16 for c in DEFAULT_CASES) and any(c.L % 16 == 0 and c.L >= 32 for c in DEFAULT_CASES)       # ragged, exact
    assert {c.L for c in DEFAULT_CASES} == {4, 8, 12, 16, 20, 32, 64, 68}
    for L in (4, 8, 12, 16, 20, 32):
        assert {c.B for c in DEFAULT_CASES if c.L == L} >= {1, 3}
        assert {c.nl & 1 for c in DEFAULT_CASES if c.L == L and c.nl > 0} == {0, 1}, 'the gP ping-pong ends in either field'
    assert {c.nl for c in DEFAULT_CASES} >= {0, 1, 3, 8, 65}
    assert W.DEEP.nl > W.HEAD_LAYERS and (W.DEEP.L, W.DEEP.B, W.DEEP.nl) == (8, 2, 65)
    # the walked launch: one layer through flow_layer_bwd(need_gw) walks k_flow_wgrad, train_grad walks k_flow_bwd_train
    c = W.WALKED
    assert (c.L, c.B) in M.LAYER_SHAPES and max(M.wgrad_histogram(c.B, c.L, 1)) > 1
    path, (items, tpw, ns, rows) = M.train_launch(c.B, c.L, c.nl)
    assert path == 'fused' and tpw > 1 and max(M.fused_histogram(c.B, c.L)) > 1 and rows < items
    assert set(c.only) <= set(W.ROW)
    # the generic nets: the shape of second_order_cases L8_net and the kernel_size > L case of net_shape_cases
    import net_shape_cases as NS
    import second_order_cases as SC
    assert W.NET.arch == SC.BY_NAME['L8_net'].arch and W.K15.arch == NS.BY_NAME['k15_L8'].arch and W.K15.arch[1] > W.K15.L
    # a stash whose last 16 doubles are live and cut by a workspace 64 doubles short (the first experiment of the GPU file)
    assert any(c.B * 19 * c.L * c.L % 32 for c in DEFAULT_CASES if c.nl > 0)


def test_every_row_and_case_is_served():
    t = W.table()
    assert len(set(W.table_ids(t))) == len(t)
    for row in W.ROWS:
        for s in W.SETTINGS:
            served = [c for c in W.CASES if W.serves(row, c, s)]
            assert len(served) != 1, f'{row.name} under {s.name}: a single case has no donor of stale scratch'
            for c in served:
                assert W.donor(row, c, s) not in (None, c)
        assert any(r is row and s.name == 'default' for r, _, s in t), row.name
    for c in W.CASES:
        assert any(cc is c for _, cc, _ in t), c.name
    # every setting that changes what a row launches serves it somewhere
    for row in W.ROWS:
        names = {s.name for r, _, s in t if r is row}
        assert ('tiled' in names) == row.small and ('valu' in names) == row.valu, (row.name, names)
    assert {s.name for r, _, s in t if r.name == 'train_force_grad'} == {s.name for s in W.SETTINGS}
    # the inputs are made once and are plain: links inside (-pi, pi), weights of the default init
    h = W.host_inputs(W.CASES[0])
    assert h is W.host_inputs(W.CASES[0]) and float(h['x'].abs().max()) < 3.1416
    assert all(W.host_inputs(c)['w'].numel() == max(c.nl, 1) * ops.arch_params(c.arch) for c in W.CASES)
    master = W.pack(W._master())
    assert all(torch.equal(W.host_inputs(c)['w'], master[:max(c.nl, 1) * 955]) for c in DEFAULT_CASES if c.nl <= 8)


def test_deep_case_is_well_conditioned():
    """the oracle at the 65-layer case moves by at most SENS_BOUND = 1e-12 per tensor and per chain when every link and weight is
    nudged by one relative 2^-52, for three sets of signs"""
    ref = W.deep_oracle()
    assert all(torch.isfinite(ref[k]).all() for k in ('y', 'logdet', 'S_eff', 'F', 'logq', 'logp'))
    errs = W.deep_sensitivity()
    assert len(errs) == 6 * W.DEEP.nl + 6 * W.DEEP.B, len(errs)
    name, e = FC.worst(errs)
    print(f'{W.DEEP.name} at scale {W.DEEP_SCALE}: sensitivity {e:.1e} ({name})')
    FC.hold(errs, FC.SENS_BOUND, W.DEEP.name)
