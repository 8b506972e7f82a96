"""CPU-only: how k_flow_wgrad (csrc/flow_wgrad.hip) and k_flow_bwd_train (csrc/flow_bwd_train.hip) share the (chain, tile) items
of a launch among their workgroups, and the rows the host reserves for what they write.

A workgroup of either kernel WALKS several items and writes one row of partial weight gradients; the host sizes those rows, the
layer stride of the small path's one launch and the reduction from flow_wgrad_tpw / _ns / _nparts and flow_bwd_train_tpw / _ns /
_nparts (csrc/kernels.h: one WalkPlan computation with two sets of constants) without asking the kernel.  tests/walk_model.py
restates both sides; here
  * the restated lines are pinned to the source text (an edit there fails until the model follows),
  * over a sweep of shapes every item is walked exactly once, nothing beyond the items is walked, and the rows the workgroups
    write are exactly 0 .. nparts - 1 (the claim "valid groups are a prefix of this numbering"),
  * those rows and the reduction's fit the workspace (csrc/api_call.h ws_layout),
  * the shapes of tests/test_walked_wgrad_gpu.py walk as that module says -- a change of the heuristics that takes the walks
    out of a GPU case fails here, without a GPU.
"""
import functools
import os

import pytest

import walk_model as M
from conftest import ROOT

CSRC = os.path.join(ROOT, 'fthmc_amd', 'csrc')


def src(name):
    """a source's text; api.hip: with api_call.h in front of it, where its layouts live"""
    return ''.join(open(os.path.join(CSRC, n)).read() for n in (('api_call.h', name) if name == 'api.hip' else (name,)))


# ---------------------------------------------------------------- the model is the source
KERNELS_H_BODIES = (
    # the one computation ...
    '''inline long walk_items(int B, int L) { return (long)B * FlowGeom{MG_TR, MG_TC}.ntiles(L); }''',
    '''inline int walk_tpw(const WalkPlan& p, long items) {
    const long t = (items + (p.round_up ? p.slots - 1 : 0)) / p.slots;
    return t < 1 ? 1 : t > p.max_tpw ? p.max_tpw : (int)t;
}''',
    '''inline int walk_ns(const WalkPlan& p, long items, int tpw) {
    const long n = (items + 8 * tpw - 1) / (8 * tpw);
    return n < 1 ? 1 : n > p.max_ns ? p.max_ns : (int)n;
}''',
    '''inline long walk_nparts(const WalkPlan& p, long items, int tpw) {
    const long ns = walk_ns(p, items, tpw), k0 = items / (tpw * ns), rem = items - k0 * tpw * ns;
    return k0 * ns + (rem < ns ? rem : ns);
}''',
    '''inline long walk_grid_x(long items, int tpw, int ns) {
    const long KR = (items + (long)tpw * ns - 1) / ((long)tpw * ns), R = (KR + 7) / 8;
    return 8 * R * ns;
}''',
    # ... its two sets of constants { slots, max_tpw, max_ns, round_up } (walk_model.py spells them out as numbers) ...
    'struct WalkPlan { int slots, max_tpw, max_ns; bool round_up; };',
    'constexpr WalkPlan WALK_WGRAD = {512, 8, 64, false};',
    'constexpr WalkPlan WALK_BWD_TRAIN = {256, 64, 32, true};',
    # ... and the six names the callers use
    'inline int flow_wgrad_tpw(int B, int L, int nlayers) { return walk_tpw(WALK_WGRAD, walk_items(B, L) * (nlayers > 0 ? nlayers : 1)); }',
    'inline int flow_wgrad_ns(int B, int L, int tpw) { return walk_ns(WALK_WGRAD, walk_items(B, L), tpw); }',
    'inline int flow_wgrad_nparts(int B, int L, int tpw) { return (int)walk_nparts(WALK_WGRAD, walk_items(B, L), tpw); }',
    'inline int flow_bwd_train_tpw(int B, int L) { return walk_tpw(WALK_BWD_TRAIN, walk_items(B, L)); }',
    'inline int flow_bwd_train_ns(int B, int L, int tpw) { return walk_ns(WALK_BWD_TRAIN, walk_items(B, L), tpw); }',
    'inline long flow_bwd_train_nparts(int B, int L) { return walk_nparts(WALK_BWD_TRAIN, walk_items(B, L), flow_bwd_train_tpw(B, L)); }',
)
KERNELS_H_LINES = (
    'int nti(int L) const { return (L + tr - 1) / tr; }',
    'int ntj(int L) const { return (L + tc - 1) / tc; }',
    'int ntiles(int L) const { return nti(L) * ntj(L); }',
    'constexpr int MG_TR = 16, MG_TC = 16;',
    'inline bool flow_bwd_train_shape(int L) { return L >= 32 && (L & (L - 1)) == 0; }',
    # the rows of the workspace
    'size_t a = flow_geom(false).ntiles(L), b = 2 * FlowGeom{16, 16}.ntiles(L);',
    'inline FlowGeom flow_geom(bool) { return FlowGeom{FLOW_TILE, FLOW_TILE}; }',
    'constexpr int FLOW_TILE = 16;',
    'constexpr int FLOW_REDUCE_GROUPS = 128;',
    '''inline int flow_reduce_groups(int nparts) {
    if (nparts <= 64) return 0;
    int groups = (nparts + 31) / 32; if (groups > FLOW_REDUCE_GROUPS) groups = FLOW_REDUCE_GROUPS;
    const int chunk = (nparts + groups - 1) / groups;
    return (nparts + chunk - 1) / chunk;
}''',
)
# the walk of k_flow_wgrad and k_flow_bwd_train, stated once (csrc/flow_bwd_common.h walk_of_block)
KERNEL_MAP_LINES = (
    'const int items = A.B * ntiles, tpw = A.tpw, ns = A.wg_ns;',
    'const int KR = (items + tpw * ns - 1) / (tpw * ns), R = (KR + 7) >> 3;',
    'const int idx = (int)blockIdx.x >> 3, r_ = idx / ns, s_ = idx - r_ * ns, kr = ((int)blockIdx.x & 7) * R + r_;',
    'const int first = kr * tpw * ns + s_;',
    'if (r_ >= R || first >= items) return false;',
    'const int grp = kr * ns + s_;',
    'const int nwalk = min(tpw, (items - first + ns - 1) / ns);',
)
# both kernels take their walk from it
KERNEL_USE_LINES = (
    'if (!walk_of_block(A, ntiles, wk)) return;',
    'const int first = wk.first, grp = wk.grp, nwalk = wk.nwalk, ns = wk.ns;',
)
WGRAD_LINES = (
    'const int nti_ = (L + TR - 1) / TR, ntj_ = (L + TC - 1) / TC, ntiles = nti_ * ntj_;',
    'item_coords(first + (it + 1 < nwalk ? it + 1 : it) * ns, ntiles, ntj_, nb, nti, ntj);',   # the walk's stride
    'double* gw0 = A.gw_part + (size_t)lz * A.gwp_lstride + (size_t)grp * FLOW_GW_STRIDE;',
    'b.tpw = a.tpw > 0 ? a.tpw : 1;',
    'b.wg_ns = flow_wgrad_ns(a.B, a.L, b.tpw);',
    'const dim3 grid((unsigned)walk_grid_x(walk_items(a.B, a.L), b.tpw, b.wg_ns), a.nlb > 0 ? a.nlb : 1, 1);',
)
FUSED_LINES = (
    'b.tpw = flow_bwd_train_tpw(a.B, a.L);',
    'b.wg_ns = flow_bwd_train_ns(a.B, a.L, b.tpw);',
    'const int nti_ = L / TR, ntj_ = L / TC, ntiles = nti_ * ntj_;',
    'const int item = first + (k < nwalk ? k : nwalk - 1) * ns;',                                 # the walk's stride
    'item_coords(item, ntiles, ntj_, q.b, ti, tj);',
    'double* gw0 = A.gw_part + (size_t)grp * FLOW_GW_STRIDE;',
    'const dim3 grid((unsigned)walk_grid_x(walk_items(a.B, a.L), b.tpw, b.wg_ns), 1, 1);',
)
API_LINES = (
    'const size_t nt = flow_ntiles_max(L);',
    'const size_t nlw = train && A.is_default() && ft_small_shape(L, nl) ? (size_t)nl : 1;',
    'w.gw_rows = nl > 0 ? nlw * B * nt : 0;',
    'w.gw_tmp_rows = nl > 0 ? nlw * FLOW_REDUCE_GROUPS : 0;',
    'if (train && nl > 0 && fused_train_bwd(A, B, L)) {',
    'const size_t np = (size_t)flow_bwd_train_nparts(B, L), ng = (size_t)flow_reduce_groups((int)np);',
    'if (w.gw_rows < (size_t)nl * np) w.gw_rows = (size_t)nl * np;',
    'if (w.gw_tmp_rows < (size_t)nl * ng) w.gw_tmp_rows = (size_t)nl * ng;',
    'inline bool fused_train_bwd(const FlowArch& A, int B, int L) { return A.is_default() && flow_bwd_train_shape(L) && flow_stash_fits32(B, L, true); }',
    # the callers of the two-kernel form: one layer, and every layer of the small path in one launch
    'a.tpw = flow_wgrad_tpw(a.B, a.L, 1);',
    'FT_TRY(launch_reduce_gw(W.gw_part, flow_wgrad_nparts(a.B, a.L, a.tpw), 1.0, 0, gw, W.gw_tmp, s));',
    'f.tpw = flow_wgrad_tpw(B, L, n_layers);',
    'f.gwp_lstride = (size_t)flow_wgrad_nparts(B, L, f.tpw) * FLOW_GW_STRIDE;',
    'return launch_reduce_gw(W.gw_part, flow_wgrad_nparts(B, L, f.tpw), 1.0, 0, gw, W.gw_tmp, s, n_layers, f.gwp_lstride);',
    # the fused form: every layer's rows side by side where the workspace has them
    'const int npf = fused ? (int)flow_bwd_train_nparts(B, L) : 0;',
    'const bool one_reduction = fused && (size_t)nl * npf <= w.gw_rows && (size_t)nl * flow_reduce_groups(npf) <= w.gw_tmp_rows;',
)


def missing_lines(text, lines):
    return [line for line in lines if line not in text]


def test_the_restated_functions_are_the_ones_in_kernels_h():
    text = src('kernels.h')
    assert missing_lines(text, KERNELS_H_BODIES) == []
    assert missing_lines(text, KERNELS_H_LINES) == []


@pytest.mark.parametrize('name,own', [('flow_wgrad.hip', WGRAD_LINES), ('flow_bwd_train.hip', FUSED_LINES)])
def test_the_restated_walk_is_the_one_in_the_kernel(name, own):
    text, shared = src(name), src('flow_bwd_common.h')
    assert missing_lines(shared, KERNEL_MAP_LINES) == []
    assert missing_lines(text, KERNEL_USE_LINES) == []
    assert missing_lines(text, own) == []
    for line in KERNEL_MAP_LINES:                          # once, in the shared header: no second map the model would not know of
        assert shared.count(line) == 1 and line not in text, line


def test_the_restated_workspace_rows_are_the_ones_in_ws_layout():
    assert missing_lines(src('api.hip'), API_LINES) == []
    assert 'bool ft_small_shape(int L, int nl) { return nl >= 1 && (L == 8 || L == 12 || L == 16); }' in src('flow_small.hip')
    red = src('flow.hip')
    for line in ('const int groups = flow_reduce_groups(nparts), g0 = (nparts + 31) / 32 > FLOW_REDUCE_GROUPS ? FLOW_REDUCE_GROUPS : (nparts + 31) / 32;',
                 'const size_t tmp_l = (size_t)groups * FLOW_GW_STRIDE;',
                 'if (nparts <= 4 * RG_SL || !tmp) {', 'static_assert(4 * RG_SL == 64,'):
        assert line in red, line


def test_a_pin_notices_an_edit():
    """the pins compare text: one character of a pinned line changed, and the line counts as missing"""
    text = src('flow_bwd_common.h')
    line = 'const int nwalk = min(tpw, (items - first + ns - 1) / ns);'
    assert missing_lines(text.replace(line, line.replace('ns - 1', 'ns')), KERNEL_MAP_LINES) == [line]


# ---------------------------------------------------------------- properties over a sweep of shapes
LS = list(range(8, 128 + 4, 4))
BS = list(range(1, 200)) + [255, 256, 257, 511, 512, 513, 1000, 1024, 1025, 2047, 4096, 4100]


@functools.lru_cache(maxsize=None)                         # lattices with the same tile count repeat each other's launches
def walk_violations(items, tpw, ns, nparts):
    """-> what is wrong with the walks of one launch (an empty list: nothing)"""
    bad = []
    ws = M.walks(items, tpw, ns)
    seen = bytearray(items)
    total = 0
    for grp, first, nwalk in ws:
        if nwalk < 1 or first + (nwalk - 1) * ns >= items:
            bad.append(('walks past the items', grp, first, nwalk))
            continue
        seen[first:first + nwalk * ns:ns] = b'\1' * nwalk
        total += nwalk
    if seen.count(1) != items:
        bad.append(('items nobody walks', items - seen.count(1)))
    if total != items:
        bad.append(('items walked more than once', total - items))
    if sorted(g for g, _, _ in ws) != list(range(nparts)):
        bad.append(('rows written are not 0 .. nparts - 1', nparts, len(ws)))
    return bad


def wgrad_points():
    for L in LS:
        for B in BS:
            for nl in ((1, 2, 8, 16) if L <= 16 else (1,)):
                yield B, L, nl


def test_two_kernel_form_walks_every_item_once_into_a_prefix_of_rows():
    npoints = 0
    for B, L, nl in wgrad_points():
        items, tpw, ns, nparts = M.wgrad_launch(B, L, nl)
        assert walk_violations(items, tpw, ns, nparts) == [], (B, L, nl, tpw, ns)
        assert 1 <= tpw <= 8 and 1 <= ns <= 64 and nparts <= items
        npoints += 1
    assert npoints == len(BS) * (len(LS) + 3 * 3)


def test_fused_form_walks_every_item_once_into_a_prefix_of_rows():
    npoints = 0
    for L in LS:
        if not M.flow_bwd_train_shape(L):
            continue
        for B in BS:
            items, tpw, ns, nparts = M.fused_launch(B, L)
            assert walk_violations(items, tpw, ns, nparts) == [], (B, L, tpw, ns)
            assert 1 <= tpw <= 64 and 1 <= ns <= 32 and nparts <= items
            npoints += 1
    assert npoints == 3 * len(BS)                          # L = 32, 64, 128


def test_the_violation_check_sees_a_short_or_shifted_walk():
    """what the sweep would report if the host's formulas and the kernel's map disagreed: rows sized for another stride,
    and a walk one item short"""
    items, tpw, ns, nparts = M.wgrad_launch(257, 32, 1)
    assert walk_violations(items, tpw, ns, nparts) == []
    assert walk_violations(items, tpw, ns - 1, nparts) != []            # nparts of ns = 64 against the map of ns = 63
    assert walk_violations(items, tpw - 1, ns, nparts) != []
    assert walk_violations(items + 1, tpw, ns, nparts) != []


# ---------------------------------------------------------------- the rows fit the workspace
def test_partial_rows_and_reduction_rows_fit_the_training_workspace():
    for B, L, nl in wgrad_points():
        # one layer through layer_backward_stash: a workspace of one layer (fthmc_flow_layer_bwd) or of the sweep's nl layers
        # (force_gp on the shapes the fused kernel does not serve) -- either has at least the rows of one
        items, tpw, ns, nparts = M.wgrad_launch(B, L, 1)
        for layers in (1, nl, 24):
            gw_rows, gw_tmp_rows = M.ws_rows(B, L, layers)
            assert nparts <= gw_rows and M.flow_reduce_groups(nparts) <= gw_tmp_rows, (B, L, layers)
        # every layer of the small path in one launch: layer l writes rows l * nparts .. (l + 1) * nparts - 1
        if M.ft_small_shape(L, nl):
            items, tpw, ns, nparts = M.wgrad_launch(B, L, nl)
            gw_rows, gw_tmp_rows = M.ws_rows(B, L, nl)
            assert nl * nparts <= gw_rows and nl * M.flow_reduce_groups(nparts) <= gw_tmp_rows, (B, L, nl)
    for L in (32, 64, 128):
        for B in BS:
            npf = M.flow_bwd_train_nparts(B, L)
            for nl in (1, 2, 8, 24):
                gw_rows, gw_tmp_rows = M.ws_rows(B, L, nl)                # one reduction behind the sweep
                assert nl * npf <= gw_rows and nl * M.flow_reduce_groups(npf) <= gw_tmp_rows, (B, L, nl)


def test_the_reduction_covers_its_rows():
    """launch_reduce_gw: `groups` first-level sums of `chunk` rows each reach every partial row, none beyond"""
    for nparts in range(1, 8300):
        groups = M.flow_reduce_groups(nparts)
        if nparts <= 64:
            assert groups == 0
            continue
        g0 = min((nparts + 31) // 32, M.FLOW_REDUCE_GROUPS)
        chunk = (nparts + g0 - 1) // g0
        assert 1 <= groups <= M.FLOW_REDUCE_GROUPS and (groups - 1) * chunk < nparts <= groups * chunk, nparts


# ---------------------------------------------------------------- the shapes of tests/test_walked_wgrad_gpu.py
@pytest.mark.parametrize('L,B', sorted(M.LAYER_SHAPES))
def test_walks_of_the_one_layer_gpu_shapes(L, B):
    stripes, items, tpw, rows, hist = M.LAYER_SHAPES[(L, B)]
    assert M.wgrad_launch(B, L, 1) == (items, tpw, 64, rows)
    assert M.wgrad_histogram(B, L, 1) == hist and max(hist) == tpw > 1
    assert M.grid_x(items, tpw, 64) == 8 * 2 * 64          # two rounds per XCD, the last one ragged
    assert set(stripes) <= set(M.ALL_STRIPES) and len(M.ALL_STRIPES) == 8


@pytest.mark.parametrize('L,B,nl', sorted(M.TRAIN_SHAPES))
def test_walks_of_the_training_gpu_shapes(L, B, nl):
    beta, path, tpw, ns, rows, hist = M.TRAIN_SHAPES[(L, B, nl)]
    got, (items, tpw_, ns_, rows_) = M.train_launch(B, L, nl)
    assert (got, tpw_, ns_, rows_) == (path, tpw, ns, rows)
    assert M.histogram(items, tpw, ns) == hist and max(hist) == tpw > 1


def test_the_cases_the_gpu_shapes_are_there_for():
    assert M.TRAIN_SHAPES[(8, 130, 8)][4] < 130                                  # the layer stride of the partials is NOT the item count
    assert {n & 1 for n in M.TRAIN_SHAPES[(32, 129, 2)][5]} == {0, 1}            # the last item's conv3 sum from either buffer
    assert min(M.TRAIN_SHAPES[(32, 129, 2)][5]) >= 2 and max(M.TRAIN_SHAPES[(32, 193, 2)][5]) == 4
    assert M.ntiles(20) == 4 and M.ntiles(40) == 9 and M.ntiles(16) == M.ntiles(8) == 1


def test_the_small_path_switched_off_does_not_walk_at_config_2():
    """512 chains of L = 16 layer by layer (ops.set_small_path(False)): 512 items a launch, one per workgroup -- the unwalked
    twin the GPU test compares the walk of 8 with"""
    assert M.wgrad_launch(512, 16, 1) == (512, 1, 64, 512) and M.wgrad_histogram(512, 16, 1) == {1: 512}


def test_fused_cases_of_the_earlier_suite_walk_two_items_everywhere():
    """tests/test_training_gpu.py (20, 64, 2): 320 items on 160 workgroups, every one walks exactly two -- no ragged round"""
    assert M.fused_launch(20, 64) == (320, 2, 20, 160) and M.fused_histogram(20, 64) == {2: 160}
