"""Pure Python restatement of how the two weight-gradient kernels share (chain, tile) items among their workgroups.

  * csrc/kernels.h: flow_wgrad_tpw / _ns / _nparts (k_flow_wgrad, csrc/flow_wgrad.hip) and flow_bwd_train_tpw / _ns / _nparts
    (k_flow_bwd_train, csrc/flow_bwd_train.hip) -- there walk_tpw / _ns / _nparts with the plans WALK_WGRAD = {512, 8, 64, round
    down} and WALK_BWD_TRAIN = {256, 64, 32, round up}, here the two parameter sets spelled out as numbers: items a workgroup
    walks, workgroups of one XCD that walk side by side, rows of the partial buffer;
  * both kernels (csrc/flow_bwd_common.h walk_of_block): blockIdx.x -> (r_, s_, kr, first, grp, nwalk) with the early return, and
    the launchers' grid = 8 * R * ns (csrc/kernels.h walk_grid_x);
  * csrc/api_call.h ws_layout / csrc/kernels.h: the rows a training workspace has for the partials and for the reduction.

tests/test_walk_maps.py pins every line restated here to the source text and checks the properties the host code relies on;
tests/test_walked_wgrad_gpu.py asserts through this model that each of its shapes (LAYER_SHAPES, TRAIN_SHAPES below) walks as
claimed.  No GPU, no torch.
"""
from collections import Counter

TILE = 16                       # MG_TR = MG_TC: both kernels walk 16 x 16 tiles
FLOW_REDUCE_GROUPS = 128


def ntiles(L, tr=TILE, tc=TILE):
    """FlowGeom{tr, tc}.ntiles(L)"""
    return ((L + tr - 1) // tr) * ((L + tc - 1) // tc)


# ---- k_flow_wgrad
def flow_wgrad_tpw(B, L, nlayers):
    items = B * ntiles(L) * (nlayers if nlayers > 0 else 1)
    t = items // 512
    return 1 if t < 1 else 8 if t > 8 else t


def flow_wgrad_ns(B, L, tpw):
    items = B * ntiles(L)
    n = (items + 8 * tpw - 1) // (8 * tpw)
    return 1 if n < 1 else 64 if n > 64 else n


def flow_wgrad_nparts(B, L, tpw):
    items, ns = B * ntiles(L), flow_wgrad_ns(B, L, tpw)
    k0 = items // (tpw * ns)
    rem = items - k0 * tpw * ns
    return k0 * ns + (rem if rem < ns else ns)


# ---- k_flow_bwd_train
def flow_bwd_train_shape(L):
    return L >= 32 and (L & (L - 1)) == 0


def flow_bwd_train_tpw(B, L):
    items = B * ntiles(L)
    t = (items + 255) // 256
    return 1 if t < 1 else 64 if t > 64 else t


def flow_bwd_train_ns(B, L, tpw):
    items = B * ntiles(L)
    n = (items + 8 * tpw - 1) // (8 * tpw)
    return 1 if n < 1 else 32 if n > 32 else n


def flow_bwd_train_nparts(B, L):
    tpw = flow_bwd_train_tpw(B, L)
    ns = flow_bwd_train_ns(B, L, tpw)
    items = B * ntiles(L)
    k0 = items // (tpw * ns)
    rem = items - k0 * tpw * ns
    return k0 * ns + (rem if rem < ns else ns)


# ---- the kernels' own map (walk_of_block: one statement for both)
def grid_x(items, tpw, ns):
    """launch_flow_wgrad / launch_flow_bwd_train through walk_grid_x: grid.x = 8 * R * ns"""
    KR = (items + tpw * ns - 1) // (tpw * ns)
    R = (KR + 7) // 8
    return 8 * R * ns


def walks(items, tpw, ns):
    """Every workgroup of a launch that does not return before it touches memory, in blockIdx.x order: [(grp, first, nwalk)];
    it walks the items first, first + ns, ..., first + (nwalk - 1) * ns and writes row grp of the partial buffer."""
    KR = (items + tpw * ns - 1) // (tpw * ns)
    R = (KR + 7) >> 3
    out = []
    for bx in range(grid_x(items, tpw, ns)):
        idx = bx >> 3
        r_ = idx // ns
        s_ = idx - r_ * ns
        kr = (bx & 7) * R + r_
        first = kr * tpw * ns + s_
        if r_ >= R or first >= items:
            continue
        grp = kr * ns + s_
        nwalk = min(tpw, (items - first + ns - 1) // ns)
        out.append((grp, first, nwalk))
    return out


def histogram(items, tpw, ns):
    """{walk length: workgroups}"""
    return dict(Counter(nwalk for _, _, nwalk in walks(items, tpw, ns)))


def wgrad_launch(B, L, nlayers=1):
    """k_flow_wgrad as the host launches it (api.hip layer_backward_stash: nlayers = 1; fthmc_train_grad on the small path: every
    layer in one launch, blockIdx.y = layer) -> (items per layer, tpw, ns, rows per layer)"""
    tpw = flow_wgrad_tpw(B, L, nlayers)
    return B * ntiles(L), tpw, flow_wgrad_ns(B, L, tpw), flow_wgrad_nparts(B, L, tpw)


def fused_launch(B, L):
    """k_flow_bwd_train as launch_flow_bwd_train launches it -> (items, tpw, ns, rows)"""
    tpw = flow_bwd_train_tpw(B, L)
    return B * ntiles(L), tpw, flow_bwd_train_ns(B, L, tpw), flow_bwd_train_nparts(B, L)


def wgrad_histogram(B, L, nlayers=1):
    items, tpw, ns, _ = wgrad_launch(B, L, nlayers)
    return histogram(items, tpw, ns)


def fused_histogram(B, L):
    items, tpw, ns, _ = fused_launch(B, L)
    return histogram(items, tpw, ns)


# ---- the rows of a training workspace (api_call.h ws_layout, default net shape)
def flow_ntiles_max(L):
    a, b = ntiles(L), 2 * ntiles(L)
    return a if a > b else b


def flow_reduce_groups(nparts):
    if nparts <= 64:
        return 0
    groups = (nparts + 31) // 32
    if groups > FLOW_REDUCE_GROUPS:
        groups = FLOW_REDUCE_GROUPS
    chunk = (nparts + groups - 1) // groups
    return (nparts + chunk - 1) // chunk


def ft_small_shape(L, nl):
    return nl >= 1 and L in (8, 12, 16)


def ws_rows(B, L, nl, train=True):
    """-> (gw_rows, gw_tmp_rows) of ws_layout(default net, B, L, nl, train); flow_stash_fits32 holds for every shape asked here"""
    nt = flow_ntiles_max(L)
    nlw = nl if train and ft_small_shape(L, nl) else 1
    gw_rows = nlw * B * nt if nl > 0 else 0
    gw_tmp_rows = nlw * FLOW_REDUCE_GROUPS if nl > 0 else 0
    if train and nl > 0 and flow_bwd_train_shape(L):
        assert B * 35 * L * L < 1 << 32
        npf = flow_bwd_train_nparts(B, L)
        gw_rows = max(gw_rows, nl * npf)
        gw_tmp_rows = max(gw_tmp_rows, nl * flow_reduce_groups(npf))
    return gw_rows, gw_tmp_rows


def train_launch(B, L, nl):
    """the weight-gradient launches of fthmc_train_grad (default net, MFMA variant, small path on) -> (path, (items, tpw, ns, rows))
    per layer: 'small' k_flow_wgrad over every layer in one launch, 'fused' k_flow_bwd_train, 'two-kernel' k_flow_wgrad per layer"""
    if ft_small_shape(L, nl):
        return 'small', wgrad_launch(B, L, nl)
    if flow_bwd_train_shape(L):
        return 'fused', fused_launch(B, L)
    return 'two-kernel', wgrad_launch(B, L, 1)


# ---- the shapes of tests/test_walked_wgrad_gpu.py and the walks they are there for ({walk length: workgroups})
# one layer through ops.flow_layer_bwd(need_gw=True): (L, B) -> ((mu, off) cases, items, tpw, rows, walks)
ALL_STRIPES = tuple((mu, off) for off in range(4) for mu in range(2))
LAYER_SHAPES = {
    (32, 257): (ALL_STRIPES, 1028, 2, 516, {2: 512, 1: 4}),      # exact tiles, the fast-wrap instance, two rounds per XCD, the last ragged
    (32, 385): (((0, 1),), 1540, 3, 516, {3: 512, 1: 4}),        # two prefetches per walk
    (20, 257): (((1, 3),), 1028, 2, 516, {2: 512, 1: 4}),        # L < 24: the FASTW = false instance, ragged 16 + 4 tiles
    (40, 114): (((0, 2),), 1026, 2, 514, {2: 512, 1: 2}),        # 3 x 3 tiles with 8-wide edges, walks that cross chains and tile rows
    (16, 1030): (((0, 3),), 1030, 2, 518, {2: 512, 1: 6}),       # one exact tile per chain
    (8, 2050): (((1, 0),), 2050, 4, 514, {4: 512, 1: 2}),        # a window that wraps onto itself
}
# ops.train_grad: (L, B, nl) -> (beta, path, tpw, ns, rows per layer, walks per layer)
TRAIN_SHAPES = {
    (8, 130, 8): (2.0, 'small', 2, 9, 67, {2: 63, 1: 4}),             # layer stride of 67 rows, fewer than the 130 items
    (16, 512, 8): (4.0, 'small', 8, 8, 64, {8: 64}),                  # the config-2 training shape
    (12, 500, 9): (3.0, 'small', 8, 8, 64, {8: 56, 7: 4, 6: 4}),      # ragged walks of 7 and 6
    (24, 260, 3): (2.5, 'two-kernel', 2, 64, 528, {2: 512, 1: 16}),   # layer_backward_stash inside force_gp, on a sweep's stash
    (32, 129, 2): (3.0, 'fused', 3, 22, 176, {3: 164, 2: 12}),        # a third item reuses a double buffer; last items in buffer 0 and in 1
    (32, 193, 2): (3.0, 'fused', 4, 25, 200, {4: 175, 3: 22, 2: 3}),  # walk lengths of both parities
}
