"""Tensor-level operators over the C ABI (one function per entry point of
include/fthmc_hip.h).  Inputs must be fp64 tensors on a HIP device; PyTorch only
provides device memory and the current stream."""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import ACT_CODES, INTEGRATORS, MODE_LITERAL, MODE_MD, W_PER_LAYER, FthmcError, check

# up to here a chain's links stay in one workgroup's LDS for a whole launch (csrc/kernels.h HMC_RESIDENT_MAXL, LU_MAXL)
RESIDENT_MAXL = 64

# The one scratch cache: (device index, stream) -> the flow workspace, (device index, stream, family) -> the buffer of a call
# family that keeps its own ('train_force', 'loops', 'instanton', 'meta', 'defect'); all grown on demand by _stream_buffer
_WS = {}
_WS_CAPTURED = set()   # keys whose CURRENT buffer was handed out during a graph capture
_WS_RETIRED = []   # superseded buffers a captured hipGraph may still point into, kept alive


def _dev(t: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f'{name}: expected a torch.Tensor')
    if not t.is_cuda:
        raise FthmcError(f'{name}: tensor lives on {t.device}; fthmc_amd runs on the MI355X only '
                         f'(no CPU fallback) -- move it with .cuda()')
    if t.dtype != torch.float64:
        raise FthmcError(f'{name}: dtype {t.dtype}; the HIP path computes in float64')
    return t.contiguous()


def _field(t, name='x'):
    t = _dev(t, name)
    if t.dim() != 4 or t.shape[1] != 2 or t.shape[2] != t.shape[3]:
        raise FthmcError(f'{name}: expected [B, 2, L, L], got {tuple(t.shape)}')
    if t.shape[2] % 4 != 0:
        raise FthmcError(f'{name}: L={t.shape[2]} must be a multiple of 4 (stripe masks have period 4)')
    return t


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _stream(t: torch.Tensor):
    return torch.cuda.current_stream(t.device).cuda_stream


def _expect(t, n: int, name: str, dtype=torch.float64):
    """a caller-supplied tensor the library reads or writes IN PLACE: on the device, contiguous, of `dtype`, n entries"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or t.numel() != n:
        raise FthmcError(f'{name}: expected a contiguous {dtype} device tensor of {n} entries')
    return t


def _out(t, shape: tuple, name: str, device, dtype=torch.float64):
    """the caller's output tensor `t` after the check (written in place: no copy launches behind the kernel in a captured
    loop), or a fresh one of `shape`"""
    return torch.empty(shape, dtype=dtype, device=device) if t is None else _expect(t, math.prod(shape), name, dtype)


def _out_like(t, x, name: str):
    """as _out for an output that has the shape of the field `x`"""
    if t is None:
        return torch.empty_like(x)
    if t.shape != x.shape:
        raise FthmcError(f'{name}: expected the shape of x {tuple(x.shape)}, got {tuple(t.shape)}')
    return _expect(t, x.numel(), name)


def _seeds(seeds, B: int):
    """per-chain seeds as the library reads them: int64 [B] on the device, made contiguous; None stays None"""
    if seeds is None:
        return None
    if not seeds.is_cuda or seeds.dtype != torch.int64 or seeds.numel() != B:
        raise FthmcError(f'seeds: expected an int64 tensor of {B} entries on the HIP device')
    return seeds.contiguous()


def ws_bytes(B: int, L: int, n_layers: int, arch=None) -> int:
    return int(_lib.load().fthmc_ws_bytes(_arch(arch), B, L, n_layers))


def ft_meta_ws_bytes(B: int, L: int, n_layers: int, arch=None) -> int:
    """Scratch of ft_meta_trajectory / ft_meta_force / ft_meta_action: ws_bytes and the two rows of chain sums behind it"""
    return int(_lib.load().fthmc_ft_meta_ws_bytes(_arch(arch), B, L, n_layers))


def ft_defect_ws_bytes(B: int, L: int, n_layers: int, arch=None) -> int:
    """Scratch of ft_defect_trajectory / ft_defect_force / ft_defect_action: ws_bytes and the three rows of chain sums behind it"""
    return int(_lib.load().fthmc_ft_defect_ws_bytes(_arch(arch), B, L, n_layers))


def vjp_ws_bytes(B: int, L: int, n_layers: int, arch=None) -> int:
    """Scratch of the second-order calls (ft_action_vjp, ft_force_vjp); 0 for a refused shape."""
    return int(_lib.load().fthmc_vjp_ws_bytes(_arch(arch), B, L, n_layers))


def train_force_ws_bytes(B: int, L: int, n_layers: int, arch=None) -> int:
    """Scratch of train_force_grad under the current `set_dual_path` setting; 0 for a refused shape."""
    return int(_lib.load().fthmc_train_force_ws_bytes(_arch(arch), B, L, n_layers))


def _stream_buffer(t: torch.Tensor, need: int, family=None, zero_head: bool = False):
    """-> (pointer, bytes) of the scratch of the current stream of t's device that serves `need` bytes, grown where it is too
    small.  One buffer per (device, stream): chain groups running on concurrent streams must not share scratch; a `family`
    keeps a buffer of its own beside the flow workspace.  zero_head: the first fthmc_ws_head_bytes() of a fresh buffer are
    zeroed."""
    key = (t.device.index, torch.cuda.current_stream(t.device).cuda_stream) + (() if family is None else (family,))
    buf, capturing = _WS.get(key), torch.cuda.is_current_stream_capturing()
    if buf is None or buf.numel() * 8 < need:
        if capturing:
            # an allocation made here would come from the graph's private pool and the pointer would be
            # baked into the graph while later eager calls keep using (or replace) the buffer
            raise FthmcError(f'the {family or "flow"} workspace of this stream would have to be '
                             f'{"allocated" if buf is None else "grown"} ({need} bytes) during graph capture: run the same call '
                             f'once eagerly on this stream first (warm-up), then capture')
        if buf is not None and key in _WS_CAPTURED:
            _WS_RETIRED.append(buf)        # a graph captured on this stream replays into it: keep it alive
        # (a buffer no capture ever saw is simply dropped: the allocator orders its reuse behind this stream's work)
        _WS_CAPTURED.discard(key)
        buf = torch.empty((need + 7) // 8, dtype=torch.float64, device=t.device)
        if zero_head:
            # the head holds the weight expansions and their stamps (include/fthmc_hip.h, "Weight versions"): fresh memory
            # may carry the stamps of an earlier life of the same address
            buf[:min(buf.numel(), int(_lib.load().fthmc_ws_head_bytes()) // 8)].zero_()
        _WS[key] = buf
    if capturing:
        _WS_CAPTURED.add(key)
    return buf.data_ptr(), buf.numel() * 8


def _ws(t: torch.Tensor, B: int, L: int, nl: int, train: bool = False, arch=None, vjp: bool = False, force: bool = False,
        meta: bool = False, defect: bool = False):
    if meta:                                             # the flow workspace with the chain sums behind it: the same buffer, grown
        need = ft_meta_ws_bytes(B, L, nl, arch)
    elif defect:                                         # likewise, with the defect calls' three rows
        need = ft_defect_ws_bytes(B, L, nl, arch)
    elif force:
        need = train_force_ws_bytes(B, L, nl, arch)
        if need == 0:
            raise FthmcError(f'train_force_grad: shape B={B}, L={L}, {nl} layers is refused (fthmc_train_force_ws_bytes = 0)')
    elif vjp:
        need = vjp_ws_bytes(B, L, nl, arch)
    else:
        need = int(_lib.load().fthmc_train_ws_bytes(_arch(arch), B, L, nl)) if train else ws_bytes(B, L, nl, arch)
    # train_force: a buffer of its own, the dual regions would otherwise stay with every later sampling call
    return _stream_buffer(t, need, 'train_force' if force else None, zero_head=True)


def release_workspaces():
    """Drop every cached workspace (current and superseded, of every family).  Only when no captured graph that used them
    will be replayed again."""
    _WS.clear()
    _WS_CAPTURED.clear()
    _WS_RETIRED.clear()


def weights_version(wkey) -> int:
    """The caller's statement of the weights' CONTENT version (`wkey`: any hashable -- FieldTransformation: parameter
    versions + the flat buffer's generation, utils/layers.py weights_generation) as the 64-bit number of the C ABI's `_v`
    entry points; None -> 0 = no statement: the call expands its weights.  The library compares it ON THE DEVICE with the
    stamps the last expansion left in the workspace (include/fthmc_hip.h, "Weight versions"): nothing is recorded here."""
    if wkey is None:
        return 0
    if isinstance(wkey, int) and 0 < wkey < (1 << 64):
        return wkey
    return (hash(('fthmc-weights', wkey)) & 0xFFFFFFFFFFFFFFFF) or 1


def _group_edges(groups, B: int):
    if isinstance(groups, (list, tuple)):
        if sum(groups) != B or min(groups) < 1:
            raise FthmcError(f'groups: sizes {tuple(groups)} do not add up to {B} chains')
        return [sum(groups[:k]) for k in range(len(groups) + 1)]
    G = max(1, min(int(groups), B))
    return [k * B // G for k in range(G + 1)]


def trajectory_workspaces(x: torch.Tensor, w, n_layers: int, groups=1, arch=None, side_streams=None, wkey=None):
    """Make sure the workspace of every stream an `ft_trajectory(x, ..., groups=groups)` call from the current stream runs on
    (the current stream and the side streams of the chain groups) exists at its final size, holding the expansion of `w`
    -> a token (the workspaces' addresses): a captured sequence stays valid while the token does."""
    x = _field(x); B, _, L, _ = x.shape
    token = []
    for lo, hi, st in _chain_groups(x.device, _group_edges(groups, B), side_streams):
        with torch.cuda.stream(st):
            pack_workspace(x, w, n_layers, hi - lo, L, wkey=wkey, arch=arch)
            token.append(_WS[(x.device.index, st.cuda_stream)].data_ptr())
    return tuple(token)


def pack_workspace(t: torch.Tensor, w, n_layers: int, B: int, L: int, wkey=None, arch=None):
    """Expand `w` into the workspace of the current stream (grown to serve [B, 2, L, L] calls with n_layers layers) under the
    version `wkey` states (C ABI fthmc_pack_weights): later calls on this stream with the same `wkey` find the stamps."""
    w, ap, a = _wall(w, n_layers, arch)
    ws, nb = _ws(t, B, L, n_layers, arch=a)
    check(_lib.load().fthmc_pack_weights(_p(w), ap, n_layers, weights_version(wkey), ws, nb, _stream(t)), 'fthmc_pack_weights')


# ---------------------------------------------------------------- s/t net shape
# The shape of the s/t conv net is an ARGUMENT of every call that runs the net (C ABI: fthmc_arch_t; the library keeps no
# shape between calls).  On this side it is a tuple (hidden_sizes, kernel_size, n_mixture_comps) -- with a fourth entry True for a
# net that ends in a tanh (make_conv_net(use_final_tanh=True)) --; it comes, in this order,
# from the `arch=` argument of an op, from the tag `pack_weights` leaves on a packed weight tensor (`arch_of`), or it is
# the reference default.
DEFAULT_ARCH = ((8, 8), 3, 2)          # hidden_sizes, kernel_size, n_mixture_comps: the reference default (tuned kernels)


def norm_arch(arch) -> tuple:
    if arch is None:
        return DEFAULT_ARCH
    a = (tuple(int(h) for h in arch[0]), int(arch[1]), int(arch[2]))
    return a + (True,) if len(arch) > 3 and arch[3] else a


def arch_params(arch=DEFAULT_ARCH) -> int:
    """Doubles per layer of the canonical weight layout [w0 b0 w1 b1 ...] for a net 2 -> hidden... -> n_mix + 1."""
    hidden, k, n_mix = norm_arch(arch)[:3]
    chans = [2, *hidden, n_mix + 1]
    return sum(co * ci * k * k + co for ci, co in zip(chans[:-1], chans[1:]))


def _arch(arch):
    """-> the fthmc_arch_t* of a call (None = NULL = the default shape)"""
    arch = norm_arch(arch)
    if arch == DEFAULT_ARCH:
        return None
    hidden, k, n_mix = arch[:3]
    if len(hidden) > 8:
        raise FthmcError(f'net shape {arch}: at most 8 hidden layers')
    a = _lib.ArchT()
    a.n_hidden, a.kernel_size, a.n_mix, a.final_tanh = len(hidden), k, n_mix, int(len(arch) > 3)
    for i, h in enumerate(hidden):
        a.hidden[i] = h
    import ctypes
    return ctypes.pointer(a)


def arch_of(w, arch=None) -> tuple:
    """The net shape of a call: the explicit `arch`, else the one recorded on the packed weight tensor `w` by pack_weights
    (a plain attribute: it does not survive .to() / .clone() / arithmetic -- pass `arch=` then), else the default."""
    if arch is not None:
        return norm_arch(arch)
    return getattr(w, '_fthmc_arch', DEFAULT_ARCH)


def _tag(t, like, arch=None):
    """carry the net shape of `like` (or `arch`) over to a tensor derived from it"""
    a = arch_of(like, arch)
    if a != DEFAULT_ARCH and t is not None:
        t._fthmc_arch = a
    return t


def set_variant(v: int):
    """1: MFMA conv kernels (default), 0: VALU conv kernels."""
    check(_lib.load().fthmc_set_variant(int(v)), 'fthmc_set_variant')


def get_variant() -> int:
    return int(_lib.load().fthmc_get_variant())


def set_small_path(on: bool):
    """Lattices of L = 8, 12, 16: one fused launch per trajectory / force / action (default) or the tiled kernels."""
    check(_lib.load().fthmc_set_small_path(int(bool(on))), 'fthmc_set_small_path')


def get_small_path() -> bool:
    return bool(_lib.load().fthmc_get_small_path())


def set_dual_path(on):
    """The dual sweep behind train_force_grad: True / 1 (default) the fused tile kernels where they serve the shape, False / 0
    the plain dual kernels always, 2 / 3 the fused kernels with 8 x 8 tiles always / 8 x 16 tiles wherever those divide L (the
    A/B of the tile shapes)."""
    check(_lib.load().fthmc_set_dual_path(int(on)), 'fthmc_set_dual_path')


def get_dual_path() -> int:
    return int(_lib.load().fthmc_get_dual_path())


def train_force_path(B: int, L: int, arch=None) -> int:
    """1: the fused dual kernels serve a train_force_grad call of this shape under the current setting, 0: the plain ones."""
    return int(_lib.load().fthmc_train_force_path(_arch(arch), B, L))


def act_code(act) -> int:
    key = act.lower() if isinstance(act, str) else act
    if key not in ACT_CODES:
        key = 'silu'                  # reference falls back to SiLU (layers.py:127-133)
    return ACT_CODES[key]


def pack_weights(nets: Sequence[Sequence[torch.Tensor]], device=None, final_tanh: bool = False) -> torch.Tensor:
    """[(w0, b0, w1, b1, ...), ...] -> flat [n_layers * params] fp64 (PyTorch order).  The conv nets may have any
    hidden sizes / odd kernel size / number of mixture components (all layers alike); the shape is recorded on the
    result (`arch_of`) and selects the kernels: the tuned ones for the reference default 2 -> 8 -> 8 -> 3, k = 3."""
    rows, arch = [], None
    for w in nets:
        w = list(w)
        shapes = [tuple(t.shape) for t in w]
        ok = len(w) >= 2 and len(w) % 2 == 0
        ci, k = 2, (shapes[0][-1] if ok and len(shapes[0]) == 4 else 0)
        for wi, bi in zip(shapes[0::2], shapes[1::2]):
            ok = ok and len(wi) == 4 and wi[1] == ci and wi[2] == wi[3] == k and bi == (wi[0],)
            ci = wi[0] if len(wi) == 4 else 0
        if not ok or k % 2 == 0 or ci < 2:
            raise FthmcError(f'unsupported s/t net {shapes}: expected Conv2d weights (c1, 2, k, k), (c1,), (c2, c1, k, k), ... '
                             f'with one odd kernel size and n_mix + 1 >= 2 output channels')
        a = (tuple(s_[0] for s_ in shapes[0:-2:2]), k, ci - 1)
        if arch is not None and a != arch:
            raise FthmcError(f'layers of one flow must share the net shape: {arch} vs {a}')
        arch = a
        rows.append(torch.cat([t.detach().reshape(-1).to(torch.float64) for t in w]))
    if arch is not None and (len(arch[0]) > 8 or max(arch[0] + (1,)) > 256 or arch[1] > 15 or arch[2] > 64):
        raise FthmcError(f'net shape {arch} beyond the limits of the HIP kernels (8 hidden layers of <= 256 channels, '
                         f'kernel_size <= 15, 64 mixture components)')
    out = torch.stack(rows).contiguous() if rows else torch.zeros(0, W_PER_LAYER, dtype=torch.float64)
    if device is not None:
        out = out.to(device)
    out = out.reshape(-1)
    if arch is not None and final_tanh:
        arch = arch + (True,)                  # a tanh behind the last conv: not visible in the weights, the caller says so
    if arch is not None and arch != DEFAULT_ARCH:
        out._fthmc_arch = arch
    return out


def unpack_weight_grads(gw: torch.Tensor, n_layers: int, arch=None):
    """flat [n_layers * params] -> list of tuples shaped like the conv parameters (w0, b0, w1, b1, ...)."""
    hidden, k, n_mix = (arch if arch is not None else arch_of(gw))[:3]
    chans = [2, *hidden, n_mix + 1]
    sizes = []
    for ci, co in zip(chans[:-1], chans[1:]):
        sizes += [(co, ci, k, k), (co,)]
    out = []
    g = gw.reshape(n_layers, -1)
    for l in range(n_layers):
        o, row = 0, []
        for s in sizes:
            n = 1
            for d in s:
                n *= d
            row.append(g[l, o:o + n].reshape(s))
            o += n
        out.append(tuple(row))
    return out


# ---------------------------------------------------------------- angle maps
def wrap(x):
    x = _dev(x, 'x'); out = torch.empty_like(x)
    check(_lib.load().fthmc_wrap(_p(x), _p(out), x.numel(), _stream(x)), 'fthmc_wrap')
    return out


def regularize(x):
    x = _dev(x, 'x'); out = torch.empty_like(x)
    check(_lib.load().fthmc_regularize(_p(x), _p(out), x.numel(), _stream(x)), 'fthmc_regularize')
    return out


# ---------------------------------------------------------------- Wilson
def plaquettes(x):
    x = _field(x); B, _, L, _ = x.shape
    P = torch.empty(B, L, L, dtype=x.dtype, device=x.device)
    check(_lib.load().fthmc_plaquettes(_p(x), _p(P), B, L, _stream(x)), 'fthmc_plaquettes')
    return P


def _out_vec(out, key, B, like, dtype=torch.float64):
    """out[key] when the caller supplies it (a vector of B entries), else a fresh one; on the path of every eager call: no
    name is formatted where nothing is wrong"""
    t = None if out is None else out.get(key)
    return torch.empty(B, dtype=dtype, device=like.device) if t is None else _expect(t, B, f'out[{key!r}]', dtype)


def wilson_action_charge(x, beta: float, out=None):
    """-> (S, Q, plaq) per chain; out: optional dict with any of 'S', 'Q', 'plaq' to write into"""
    x = _field(x); B, _, L, _ = x.shape
    S, Q, plaq = (_out_vec(out, k, B, x) for k in ('S', 'Q', 'plaq'))
    check(_lib.load().fthmc_wilson_action_charge(_p(x), B, L, float(beta), _p(S), _p(Q), _p(plaq), _stream(x)),
          'fthmc_wilson_action_charge')
    return S, Q, plaq


def wilson_loops_ws_bytes(B: int, L: int, Rmax: int, Tmax: int) -> int:
    """Scratch of wilson_loops; 0 for a refused shape."""
    return int(_lib.load().fthmc_wilson_loops_ws_bytes(B, L, Rmax, Tmax))


def _loops_ws(t: torch.Tensor, need: int):
    return _stream_buffer(t, need, 'loops')           # a small buffer of its own: never the flow workspaces of _ws


def wilson_loops(x, Rmax: int, Tmax: Optional[int] = None, out=None, mean_out=None):
    """The table of rectangular Wilson loops of every chain (C ABI fthmc_wilson_loops) -> W [B, Rmax, Tmax]:
    W[b, R-1, T-1] = mean over the L^2 corners of cos(angle of the R x T loop), extent R along x0's direction (axis 2 of x) and T
    along x1's (axis 3), wrapping around the torus.  W[:, 0, 0] is the mean of cos P; the column T = L is the Polyakov-loop
    correlator at distance R.  Tmax = None: Rmax.  `out` [B, Rmax, Tmax] and `mean_out` [Rmax, Tmax] (the mean over the chains,
    added in index order) are written in place when given (contiguous float64 device tensors: a captured loop passes both).
    Not differentiable: an observable of finished configurations."""
    x = _field(x); B, _, L, _ = x.shape
    Rmax = int(Rmax); Tmax = Rmax if Tmax is None else int(Tmax)
    if not (1 <= Rmax <= L and 1 <= Tmax <= L):
        raise ValueError(f'wilson_loops: 1 <= Rmax, Tmax <= L = {L} expected, got {Rmax}, {Tmax}')
    W = _out(out, (B, Rmax, Tmax), 'out', x.device)
    if mean_out is not None:
        _expect(mean_out, Rmax * Tmax, 'mean_out')
    need = wilson_loops_ws_bytes(B, L, Rmax, Tmax)
    if need == 0:
        raise FthmcError(f'wilson_loops: shape B={B}, L={L}, Rmax={Rmax}, Tmax={Tmax} is refused (fthmc_wilson_loops_ws_bytes = 0)')
    with torch.cuda.device(x.device):
        ws, nb = _loops_ws(x, need)
        check(_lib.load().fthmc_wilson_loops(_p(x), B, L, Rmax, Tmax, _p(W), _p(mean_out), ws, nb, _stream(x)), 'fthmc_wilson_loops')
    return W.view(B, Rmax, Tmax)


def local_update(x, beta, seeds=None, n_hb: int = 1, n_or: int = 0, nsweep: int = 1, sweep0: int = 0, classes: int = 0xF, out=None):
    """Heatbath and overrelaxation sweeps of the plain Wilson action (C ABI fthmc_local_update) -> the updated field: `nsweep`
    compound sweeps, each `n_hb` heatbath sweeps (an exact draw of every link from its conditional von Mises distribution) followed by
    `n_or` overrelaxation sweeps (the reflection of every link about its conditional mode: the action does not change).
    beta: a number, or a device tensor of B doubles -- per-chain beta.  seeds: int64 [B] on the device (ops.chain_seeds), needed for
    heatbath only; `sweep0` is the index of the call's first heatbath sweep in the random stream: a caller that keeps one seed per
    chain moves it on by nsweep * n_hb per call, one that draws fresh seeds per call leaves it 0.  classes: mask of the link classes
    (bit 2 mu + parity) a sweep touches.  out: written in place when given (may be x).  Not differentiable."""
    x = _field(x); B, _, L, _ = x.shape
    n_hb, n_or, nsweep, sweep0, classes = int(n_hb), int(n_or), int(nsweep), int(sweep0), int(classes)
    if min(n_hb, n_or, nsweep, sweep0) < 0 or not 1 <= classes <= 15:
        raise ValueError(f'local_update: counts and sweep0 >= 0 and classes in 1 .. 15 expected, got n_hb={n_hb}, n_or={n_or}, '
                         f'nsweep={nsweep}, sweep0={sweep0}, classes={classes}')
    if n_hb > 0 and seeds is None:
        raise ValueError('local_update: heatbath sweeps need per-chain seeds')
    seeds, bb, out = _seeds(seeds, B), _beta_b(beta, B), _out_like(out, x, 'out')
    check(_lib.load().fthmc_local_update(_p(x), B, L, 0.0 if bb is not None else float(beta), _p(bb), _p(seeds), n_hb, n_or, nsweep,
                                         sweep0, classes, _p(out), _stream(x)), 'fthmc_local_update')
    return out


def anneal(x, betas, seeds=None, n_hb: int = 1, n_or: int = 0, nsweep: int = 1, sweep0: int = 0, work=None, trace=False, path: int = 0,
           out=None):
    """An annealing ramp through the local updates with the work of every chain (C ABI fthmc_anneal) -> dict(x, work, trace).
    betas: the schedule beta_0 .. beta_n, n + 1 entries: a float64 device tensor, read by the kernels when they run (a captured call
    follows what the tensor holds at replay; finite entries >= 0 are then the caller's promise), or a sequence of numbers, checked
    and uploaded once.  Step k adds (beta_k - beta_{k+1}) sum cos P(x_k) to the work and runs `nsweep` compound sweeps (`n_hb`
    heatbath, `n_or` overrelaxation) at beta_{k+1}; the heatbath sweeps are those of local_update(..., sweep0 = sweep0 + k nsweep n_hb).
    work: the work the chains arrive with, [B] (None: 0).  trace: True (or a [B, n + 1] tensor to write) for sum cos P of x_0 .. x_n.
    path: 0 the library chooses, 1 the whole ramp in one launch (L <= 64), 2 per step a work kernel and the class kernels; the
    same bits.  out: optional dict with 'x' (may be x) and 'work' (may be `work`) to write into.  exp(-work) is the importance
    weight of x as a sample at beta_n when the start was drawn at beta_0.  Not differentiable."""
    x = _field(x); B, _, L, _ = x.shape
    if isinstance(betas, torch.Tensor):
        bt = _dev(betas, 'betas').reshape(-1)
        if bt.device != x.device:
            raise FthmcError(f'betas: tensor lives on {bt.device}, x on {x.device}')
    else:
        host = [float(b) for b in betas]
        if not all(math.isfinite(b) and b >= 0.0 for b in host):
            raise ValueError('anneal: finite betas >= 0 expected')
        bt = torch.tensor(host, dtype=torch.float64, device=x.device)
    n_step = bt.numel() - 1
    n_hb, n_or, nsweep, sweep0, path = int(n_hb), int(n_or), int(nsweep), int(sweep0), int(path)
    if n_step < 0 or n_step > 65536 or min(n_hb, n_or, nsweep, sweep0) < 0 or path not in (0, 1, 2) or (n_step > 0 and n_hb + n_or == 0):
        raise ValueError(f'anneal: 1 .. 65537 betas, counts and sweep0 >= 0, n_hb + n_or > 0 and path in 0 .. 2 expected, got {n_step + 1} '
                         f'betas, n_hb={n_hb}, n_or={n_or}, nsweep={nsweep}, sweep0={sweep0}, path={path}')
    if sweep0 + n_step * nsweep * n_hb > 2 ** 32:
        raise ValueError(f'anneal: sweep0 + n_step nsweep n_hb = {sweep0 + n_step * nsweep * n_hb} is beyond 2^32')
    if path == 1 and L > RESIDENT_MAXL:
        raise ValueError(f'anneal: path 1 serves L <= {RESIDENT_MAXL}')
    if n_hb > 0 and seeds is None:
        raise ValueError('anneal: heatbath sweeps need per-chain seeds')
    seeds = _seeds(seeds, B)
    if work is not None:
        _expect(work, B, 'work')
    out = {} if out is None else out
    xo = _out_like(out.get('x'), x, "out['x']")
    wo = _out_vec(out, 'work', B, x)
    tr = None
    if isinstance(trace, torch.Tensor):
        tr = _expect(trace, B * (n_step + 1), 'trace')
    elif trace:
        tr = torch.empty(B, n_step + 1, dtype=torch.float64, device=x.device)
    check(_lib.load().fthmc_anneal(_p(x), B, L, _p(bt), n_step, _p(seeds), n_hb, n_or, nsweep, sweep0, path, _p(work), _p(xo), _p(wo),
                                   _p(tr), _stream(x)), 'fthmc_anneal')
    return {'x': xo, 'work': wo, 'trace': None if tr is None else tr.view(B, n_step + 1)}


def instanton_ws_bytes(B: int, L: int, path: int = 0) -> int:
    """Scratch of instanton_hit: 0 where the path that (B, L, path) selects needs none."""
    return int(_lib.load().fthmc_instanton_ws_bytes(B, L, path))


def _inst_ws(t: torch.Tensor, need: int):
    """the scratch of instanton_hit's split path (a small buffer of its own, as _loops_ws); no scratch where none is needed"""
    return _stream_buffer(t, need, 'instanton') if need else (None, 0)


def _instanton_call(x, beta, seeds, n_hit, hit0, path, out, want_cs):
    x = _field(x); B, _, L, _ = x.shape
    n_hit, hit0, path = int(n_hit), int(hit0), int(path)
    if not 0 <= n_hit <= 1024 or hit0 < 0 or hit0 + n_hit > 2 ** 32 or path not in (0, 1, 2):
        raise ValueError(f'instanton_hit: n_hit in 0 .. 1024, hit0 >= 0 with hit0 + n_hit <= 2^32 and path in 0 .. 2 expected, got '
                         f'n_hit={n_hit}, hit0={hit0}, path={path}')
    if n_hit > 0 and seeds is None:
        raise ValueError('instanton_hit: hits need per-chain seeds')
    seeds, bb = _seeds(seeds, B), _beta_b(beta, B)
    if isinstance(out, torch.Tensor):
        out = {'x': out}
    out = {} if out is None else out
    xo = _out_like(out.get('x'), x, 'out')
    k, nacc = (_out_vec(out, key, B, x, torch.int32) for key in ('k', 'nacc'))
    cs = out.get('cs')
    if cs is not None or want_cs:
        cs = _out(cs, (B, 2), "out['cs']", x.device)
    with torch.cuda.device(x.device):
        ws, nb = _inst_ws(x, instanton_ws_bytes(B, L, path))
        check(_lib.load().fthmc_instanton_hit(_p(x), B, L, 0.0 if bb is not None else float(beta), _p(bb), _p(seeds), n_hit, hit0, path,
                                              _p(xo), _p(k), _p(nacc), _p(cs), ws, nb, _stream(x)), 'fthmc_instanton_hit')
    return xo, k, nacc, cs


def instanton_hit(x, beta, seeds, n_hit: int = 1, hit0: int = 0, path: int = 0, out=None):
    """`n_hit` instanton hits of the plain Wilson action (C ABI fthmc_instanton_hit) -> (x_new, k, nacc): Metropolis steps k -> k +- 1
    in the net charge of the proposal x + k A, A the constant-field-strength configuration of charge 1, accepted with
    min(1, exp(-dS)), dS in closed form from sum cos P and sum sin P of x; then x + k A for the k the steps end with (int32 [B]);
    nacc (int32 [B]): the accepted steps.  The update that changes the topological charge where HMC and local updates freeze.
    beta: a number, or a device tensor of B doubles -- per-chain beta.  seeds: int64 [B] on the device (ops.chain_seeds; None with
    n_hit = 0); `hit0` is the index of the call's first hit in the random stream: a caller that keeps one seed per chain moves it on by
    n_hit per call, one that draws fresh seeds per call leaves it 0.  path: 0 the library chooses, 1 one workgroup per chain, 2 the
    split form for a few chains of a large lattice; the same bits.  out: the field to write (may be x), or a dict with any of 'x',
    'k', 'nacc', 'cs' ([B, 2]: sum cos P, sum sin P of x) to write into.  Not differentiable."""
    return _instanton_call(x, beta, seeds, n_hit, hit0, path, out, False)[:3]


def instanton_sums(x, path: int = 0):
    """(sum cos P, sum sin P) per chain as instanton_hit reduces them -> [B, 2] (the cs_out of an n_hit = 0 call)."""
    return _instanton_call(x, 0.0, None, 0, 0, path, None, True)[3]


# ---------------------------------------------------------------- metadynamics HMC (csrc/meta.hip)
def meta_ws_bytes(B: int, L: int, path: int = 0) -> int:
    """Scratch of meta_trajectory: 0 for path 1 (the one-launch path needs none)."""
    return int(_lib.load().fthmc_meta_ws_bytes(B, L, path))


def _meta_ws(t: torch.Tensor, need: int):
    """the scratch of meta_trajectory's sequenced path (a buffer of its own, as _loops_ws); no scratch where none is needed"""
    return _stream_buffer(t, need, 'meta') if need else (None, 0)


def _meta_table(table, B: int, qmax, wall):
    """the bias table as the library reads it -> (pointer, G, nb, qmax, wall): a contiguous float64 device tensor [G, nb] (or [nb]:
    G = 1), used IN PLACE (meta_deposit updates it between calls)"""
    if not isinstance(table, torch.Tensor) or table.dim() not in (1, 2):
        raise FthmcError('table: expected a device tensor [G, nb] (or [nb])')
    G, nb = (1, table.shape[0]) if table.dim() == 1 else table.shape
    _expect(table, G * nb, 'table')
    qmax, wall = float(qmax), float(wall)
    if G < 1 or B % G or not 2 <= nb <= 65536 or not (math.isfinite(qmax) and qmax > 0) or not (math.isfinite(wall) and wall >= 0):
        raise ValueError(f'meta table: G dividing B = {B}, 2 <= nb <= 65536, finite qmax > 0 and wall >= 0 expected, got G={G}, nb={nb}, '
                         f'qmax={qmax}, wall={wall}')
    return (_p(table), int(G), int(nb), qmax, wall)


def meta_trajectory(x, v, u, beta: float, dt: float, nstep: int, table, qmax: float, wall: float = 0.0, integrator='leapfrog',
                    path: int = 0, out=None):
    """One HMC trajectory under the bias potential V(Q_m), Q_m = sum sin P / 2 pi (C ABI fthmc_meta_trajectory) -> dict(x_new, dH,
    acc, H0, H1, qm, vbias) per chain; qm, vbias: Q_m and V(Q_m) of the field x_new holds.  table: V on the nodes
    -qmax .. qmax, a float64 device tensor [G, nb] read in place (chain b reads row b // (B // G)); wall: the stiffness of the
    quadratic wall outside.  path: 0 the library chooses, 1 one launch per trajectory (L <= 64, x_new must not be x), 2 the
    sequenced path (any L; out['x_new'] may be x).  out: optional dict with any of the result keys to write into.  With an all-zero
    table and wall = 0 the result is hmc_trajectory's.  Not differentiable."""
    ic, path = integrator_code(integrator), int(path)
    x, v, u, B, L, xn, r = _plain_trajectory_args(x, v, u, out, ('dH', 'acc', 'H0', 'H1', 'qm', 'vbias'))
    if path not in (0, 1, 2) or int(nstep) < 1:
        raise ValueError(f'meta_trajectory: path in 0 .. 2 and nstep >= 1 expected, got path={path}, nstep={nstep}')
    tab = _meta_table(table, B, qmax, wall)
    if path == 1 and (L > RESIDENT_MAXL or xn.data_ptr() == x.data_ptr()):
        raise ValueError(f"meta_trajectory: path 1 serves L <= {RESIDENT_MAXL} with out['x_new'] other than x")
    with torch.cuda.device(x.device):
        # path 0 takes the one-launch kernel where fthmc_meta_trajectory says it does: no scratch is asked for there
        seq = path == 2 or (path == 0 and (L > RESIDENT_MAXL or xn.data_ptr() == x.data_ptr() or get_variant() != 1))
        ws, nb = _meta_ws(x, meta_ws_bytes(B, L, 2) if seq else 0)
        check(_lib.load().fthmc_meta_trajectory(_p(x), _p(v), _p(u), B, L, float(beta), float(dt), int(nstep), ic, *tab, path, _p(xn),
                                                *(_p(r[k]) for k in ('dH', 'acc', 'H0', 'H1', 'qm', 'vbias')), ws, nb, _stream(x)),
              'fthmc_meta_trajectory')
    return r


def meta_deposit(qm, table, qmax: float, w: float):
    """One hill of height w per walker at qm[b], added to `table` IN PLACE (C ABI fthmc_meta_deposit): inside the table node i
    gains w (1 - f) and node i + 1 gains w f, outside nothing; the walkers of a row are added in chain order.  -> table"""
    B = qm.numel() if isinstance(qm, torch.Tensor) else 0
    _expect(qm, max(B, 1), 'qm')
    w = float(w)
    if not (math.isfinite(w) and w >= 0):
        raise ValueError(f'meta_deposit: a finite w >= 0 expected, got {w}')
    ptr, G, nb, qmax, _ = _meta_table(table, B, qmax, 0.0)
    check(_lib.load().fthmc_meta_deposit(_p(qm), B, G, nb, qmax, w, ptr, _stream(qm)), 'fthmc_meta_deposit')
    return table


def meta_force(x, beta: float, table, qmax: float, wall: float = 0.0):
    """F = dS_b / dx of the biased action S_b = -beta sum cos P + V(Q_m) (C ABI fthmc_meta_force), wilson_force's sign"""
    x = _field(x); B, _, L, _ = x.shape
    F = torch.empty_like(x)
    check(_lib.load().fthmc_meta_force(_p(x), B, L, float(beta), *_meta_table(table, B, qmax, wall), _p(F), _stream(x)), 'fthmc_meta_force')
    return F


def meta_action(x, beta: float, table, qmax: float, wall: float = 0.0, out=None):
    """-> (S_b, Q_m, V(Q_m)) per chain (C ABI fthmc_meta_action); out: optional dict with any of 'S', 'qm', 'vbias' to write into"""
    x = _field(x); B, _, L, _ = x.shape
    S, qm, vb = (_out_vec(out, k, B, x) for k in ('S', 'qm', 'vbias'))
    check(_lib.load().fthmc_meta_action(_p(x), B, L, float(beta), *_meta_table(table, B, qmax, wall), _p(S), _p(qm), _p(vb), _stream(x)),
          'fthmc_meta_action')
    return S, qm, vb


# ---------------------------------------------------------------- boundary-condition tempering (csrc/defect.hip)
def defect_ws_bytes(B: int, L: int, path: int = 0) -> int:
    """Scratch of defect_trajectory: 0 for path 1 (the one-launch path needs none)."""
    return int(_lib.load().fthmc_defect_ws_bytes(B, L, path))


def _defect_args(beta, g_b, defect, B: int, L: int):
    """the defect of a call as the library reads it -> (beta, pointer of g_b, i0, j0, Ld): g_b a float64 device tensor of B entries
    used IN PLACE (a replica exchange updates it between calls), defect = (i0, j0, Ld)"""
    g_b = _expect(g_b, B, 'g_b (per chain)').view(-1)
    try:
        i0, j0, Ld = (int(t) for t in defect)
    except (TypeError, ValueError):
        raise ValueError(f'defect: expected (i0, j0, Ld), got {defect!r}') from None
    beta = float(beta)
    if not (0 <= Ld <= L and 0 <= i0 < L and 0 <= j0 < L and math.isfinite(beta)):
        raise ValueError(f'defect: 0 <= Ld <= L = {L}, 0 <= i0, j0 < L and a finite beta expected, got {(i0, j0, Ld)}, beta={beta}')
    return (beta, _p(g_b), i0, j0, Ld)


def defect_trajectory(x, v, u, beta: float, g_b, defect, dt: float, nstep: int, integrator='leapfrog', path: int = 0, out=None):
    """One HMC trajectory of every chain under S_d = -beta sum cos P + (beta - g_b) sum over the defect of cos P (C ABI
    fthmc_defect_trajectory) -> dict(x_new, dH, acc, H0, H1, csum, dsum, Q) per chain; csum, dsum, Q: sum cos P, its part on the defect
    and the integer charge of the field x_new holds.  g_b: the defect coupling per chain, a float64 device tensor [B] read in place;
    defect = (i0, j0, Ld): the plaquettes ((i0 + a) mod L, j0), a < Ld.  path: 0 the library chooses, 1 one launch per trajectory
    (L <= 64, x_new must not be x), 2 the sequenced path (any L; out['x_new'] may be x).  out: optional dict with any of the result
    keys to write into.  With g_b = beta everywhere the result is hmc_trajectory's with a beta tensor.  Not differentiable."""
    ic, path = integrator_code(integrator), int(path)
    x, v, u, B, L, xn, r = _plain_trajectory_args(x, v, u, out, ('dH', 'acc', 'H0', 'H1', 'csum', 'dsum', 'Q'))
    if path not in (0, 1, 2) or int(nstep) < 1:
        raise ValueError(f'defect_trajectory: path in 0 .. 2 and nstep >= 1 expected, got path={path}, nstep={nstep}')
    df = _defect_args(beta, g_b, defect, B, L)
    if path == 1 and (L > RESIDENT_MAXL or xn.data_ptr() == x.data_ptr()):
        raise ValueError(f"defect_trajectory: path 1 serves L <= {RESIDENT_MAXL} with out['x_new'] other than x")
    with torch.cuda.device(x.device):
        # path 0 takes the one-launch kernel where fthmc_defect_trajectory says it does: no scratch is asked for there
        seq = path == 2 or (path == 0 and (L > RESIDENT_MAXL or xn.data_ptr() == x.data_ptr() or get_variant() != 1))
        ws, nb = _stream_buffer(x, defect_ws_bytes(B, L, 2), 'defect') if seq else (None, 0)
        check(_lib.load().fthmc_defect_trajectory(_p(x), _p(v), _p(u), B, L, *df, float(dt), int(nstep), ic, path, _p(xn),
                                                  *(_p(r[k]) for k in ('dH', 'acc', 'H0', 'H1', 'csum', 'dsum', 'Q')), ws, nb, _stream(x)),
              'fthmc_defect_trajectory')
    return r


def defect_force(x, beta: float, g_b, defect):
    """F = dS_d / dx of the action with a defect (C ABI fthmc_defect_force), wilson_force's sign"""
    x = _field(x); B, _, L, _ = x.shape
    F = torch.empty_like(x)
    check(_lib.load().fthmc_defect_force(_p(x), B, L, *_defect_args(beta, g_b, defect, B, L), _p(F), _stream(x)), 'fthmc_defect_force')
    return F


def defect_action(x, beta: float, g_b, defect, out=None):
    """-> (S_d, csum, dsum, Q) per chain (C ABI fthmc_defect_action); out: optional dict with any of 'S', 'csum', 'dsum', 'Q' to write into"""
    x = _field(x); B, _, L, _ = x.shape
    S, cs, ds, Q = (_out_vec(out, k, B, x) for k in ('S', 'csum', 'dsum', 'Q'))
    check(_lib.load().fthmc_defect_action(_p(x), B, L, *_defect_args(beta, g_b, defect, B, L), _p(S), _p(cs), _p(ds), _p(Q), _stream(x)),
          'fthmc_defect_action')
    return S, cs, ds, Q


def defect_translate(x, rung, top: int, shift, out=None):
    """The chains on rung `top` translated by shift[b] = (s0, s1), x_out[b, mu, (i + s0) % L, (j + s1) % L] = x[b, mu, i, j], every other
    chain copied (C ABI fthmc_defect_translate): bit for bit torch.roll(x[b], (s0, s1), (1, 2)).  rung: int32 [B], shift: int32 [B, 2],
    both on the device and read there; out (a field other than x) or a fresh one -> x_out"""
    x = _field(x); B, _, L, _ = x.shape
    _expect(rung, B, 'rung', torch.int32); _expect(shift, 2 * B, 'shift', torch.int32)
    xo = _out_like(out, x, 'out')
    if xo.data_ptr() == x.data_ptr():
        raise FthmcError('defect_translate: out must not be x')
    with torch.cuda.device(x.device):
        check(_lib.load().fthmc_defect_translate(_p(x), B, L, _p(rung), int(top), _p(shift), _p(xo), _stream(x)), 'fthmc_defect_translate')
    return xo


def wilson_force(x, beta: float):
    x = _field(x); B, _, L, _ = x.shape
    F = torch.empty_like(x)
    check(_lib.load().fthmc_wilson_force(_p(x), B, L, float(beta), _p(F), _stream(x)), 'fthmc_wilson_force')
    return F


def kinetic(v):
    v = _field(v, 'v'); B, _, L, _ = v.shape
    K = torch.empty(B, dtype=v.dtype, device=v.device)
    check(_lib.load().fthmc_kinetic(_p(v), B, L, _p(K), _stream(v)), 'fthmc_kinetic')
    return K


def stats_accumulate(acc, plaq, Q, qold, dH, vec):
    """vec[8] += sums over the chains of (1, acc, plaq, Q, Q^2, |Q - qold|, dH, exp(-dH)); qold <- Q (in place)."""
    B = acc.numel()
    for t, n, name in ((acc, B, 'acc'), (plaq, B, 'plaq'), (Q, B, 'Q'), (qold, B, 'qold'), (dH, B, 'dH'), (vec, 8, 'vec')):
        _expect(t, n, 'stats_accumulate: ' + name)
    check(_lib.load().fthmc_stats_accumulate(_p(acc), _p(plaq), _p(Q), _p(qold), _p(dH), B, _p(vec), _stream(acc)),
          'fthmc_stats_accumulate')


def random_momenta(seeds, shape, need_u=True, out_v=None, out_u=None):
    """v ~ N(0,1) of `shape` = (B, 2, L, L) and u ~ U[0,1) [B] from per-chain int64 seeds
    (written into out_v / out_u when given: contiguous float64 device tensors of those shapes)."""
    shape = tuple(int(d) for d in shape); B = shape[0]
    seeds = _seeds(seeds, B)
    v = _out(out_v, shape, 'random_momenta: out_v', seeds.device)
    u = _out(out_u, (B,), 'random_momenta: out_u', seeds.device) if need_u or out_u is not None else None
    check(_lib.load().fthmc_random_momenta(_p(seeds), B, math.prod(shape[1:]), _p(v), _p(u), _stream(v)), 'fthmc_random_momenta')
    return v, u


def chain_seeds(seed: int, lo: int, B: int, traj: int = 0, counter: Optional[torch.Tensor] = None, advance: bool = False,
                out: Optional[torch.Tensor] = None, device=None):
    """Per-chain int64 seeds of trajectory / step `traj (+ counter[0])` for the global chain ids lo .. lo + B - 1, formed on
    the device (C ABI fthmc_chain_seeds): the same numbers as parallel.chain_seeds.  `counter`: a device int64 scalar added
    to `traj`; advance=True adds 1 to it behind the read, so that a captured launch draws fresh seeds at every replay."""
    if out is None:                     # checked like a caller's: `device` may name the host
        out = torch.empty(B, dtype=torch.int64, device=device if device is not None else counter.device)
    _expect(out, B, 'chain_seeds: out', torch.int64)
    if counter is not None:
        _expect(counter, 1, 'chain_seeds: counter', torch.int64)
    check(_lib.load().fthmc_chain_seeds(int(seed), int(lo), int(B), int(traj), _p(counter), int(bool(advance)), _p(out),
                                        _stream(out)), 'fthmc_chain_seeds')
    return out


def random_uniform(seeds, shape, lo: float, hi: float, out=None):
    """U[lo, hi) of `shape` = (B, ...) from per-chain int64 seeds: the prior draw of a training step on the device.
    Half-open on (0, 1) and (-pi, pi); on a range whose width is not above |hi| the last rounding can return hi itself
    (include/fthmc_hip.h, fthmc_random_uniform)."""
    shape = tuple(int(d) for d in shape); B = shape[0]
    seeds = _seeds(seeds, B)
    out = _out(out, shape, 'random_uniform: out', seeds.device)
    check(_lib.load().fthmc_random_uniform(_p(seeds), B, math.prod(shape[1:]), float(lo), float(hi), _p(out), _stream(out)),
          'fthmc_random_uniform')
    return out


def train_metrics(xi, x, logq, logp, beta: float, dkl_factor: float = 1.0, out=None):
    """-> row [2 + 5 B] = (loss_dkl, ess, logp[B], logq[B], q[B], dq[B], plaq[B]) of one rank's training batch, on the
    device (C ABI fthmc_train_metrics): everything train_step reports, in one buffer."""
    xi = _field(xi, 'xi'); x = _field(x); B, _, L, _ = x.shape
    logq = _dev(logq, 'logq').reshape(-1); logp = _dev(logp, 'logp').reshape(-1)
    if logq.numel() != B or logp.numel() != B or xi.shape != x.shape:
        raise FthmcError(f'train_metrics: expected logq, logp of {B} entries and xi shaped like x')
    out = _out(out, (2 + 5 * B,), 'train_metrics: out', x.device)
    ws, nb = _ws(x, B, L, 0)
    check(_lib.load().fthmc_train_metrics(_p(xi), _p(x), _p(logq), _p(logp), B, L, float(beta), float(dkl_factor),
                                          _p(out), ws, nb, _stream(x)), 'fthmc_train_metrics')
    return out


def adam_step(w, gw, exp_avg, exp_avg_sq, hyper, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
              decoupled: bool = False):
    """One Adam (AdamW: decoupled=True) step on flat fp64 device buffers, in place, ONE launch (C ABI fthmc_adam_step).
    `hyper` = [steps taken, learning rate, 0] on the device: the launch reads both from there and moves the count on."""
    n = w.numel()
    for t, want, name in ((w, n, 'w'), (gw, n, 'gw'), (exp_avg, n, 'exp_avg'), (exp_avg_sq, n, 'exp_avg_sq'), (hyper, 3, 'hyper')):
        _expect(t, want, 'adam_step: ' + name)
    check(_lib.load().fthmc_adam_step(_p(w), _p(gw), _p(exp_avg), _p(exp_avg_sq), _p(hyper), n, float(betas[0]), float(betas[1]),
                                      float(eps), float(weight_decay), int(bool(decoupled)), _stream(w)), 'fthmc_adam_step')


def split_metrics(row, B: int) -> dict:
    """views of a train_metrics row (device or host tensor / array) under train_step's keys"""
    r = row[2:].reshape(5, B)
    return {'loss_dkl': row[0], 'ess': row[1], 'logp': r[0], 'logq': r[1], 'q': r[2], 'dq': r[3], 'plaq': r[4]}


def integrator_code(name) -> int:
    """'leapfrog' | 'omelyan' | 'force_gradient' -> FTHMC_INT_* (include/fthmc_hip.h); anything else raises ValueError"""
    try:
        return INTEGRATORS[name]
    except (KeyError, TypeError):
        raise ValueError(f'integrator: expected one of {sorted(INTEGRATORS)}, got {name!r}') from None


def integrator_forces(name, nstep: int) -> int:
    """force evaluations of one trajectory of `nstep` steps (host only: fthmc_integrator_forces)"""
    n = _lib.load().fthmc_integrator_forces(integrator_code(name), int(nstep))
    if n < 0:
        raise ValueError(f'integrator_forces({name!r}, {nstep}): nstep must be >= 1')
    return n


def integrator_schedule(name, dt: float, nstep: int):
    """-> (b0, [(kind, a, b), ...]): the MD as the library runs it (csrc/integrator.h) -- x += b0 v, then per stage
    ('kick', a, b): v -= a g(x*); x += b v, or ('shift', c, 0.0): x* = x - c g(x) for the next stage.  Host only."""
    import ctypes
    n = integrator_forces(name, nstep)
    b0 = ctypes.c_double()
    kind, a, b = (ctypes.c_int * n)(), (ctypes.c_double * n)(), (ctypes.c_double * n)()
    m = _lib.load().fthmc_integrator_schedule(integrator_code(name), float(dt), int(nstep), ctypes.byref(b0), kind, a, b, n)
    if m != n:
        raise FthmcError(f'fthmc_integrator_schedule: {m} stages where {n} were expected')
    return b0.value, [('shift' if kind[i] == _lib.STAGE_SHIFT else 'kick', a[i], b[i]) for i in range(n)]


def leapfrog(x, p, beta: float, dt: float, nstep: int, integrator='leapfrog'):
    """the plain Wilson MD -> (x', p'); integrator: 'leapfrog' | 'omelyan' | 'force_gradient' (csrc/integrator.h)"""
    ic = integrator_code(integrator)
    x = _field(x); p = _field(p, 'p'); B, _, L, _ = x.shape
    xo, po = torch.empty_like(x), torch.empty_like(p)
    ws, nb = _ws(x, B, L, 0)
    lib, head, tail = _lib.load(), (_p(x), _p(p), B, L, float(beta), float(dt), int(nstep)), (_p(xo), _p(po), ws, nb, _stream(x))
    if ic:                                        # 'leapfrog' keeps its own entry point (the fused leap steps)
        check(lib.fthmc_md(*head, ic, *tail), 'fthmc_md')
    else:
        check(lib.fthmc_leapfrog(*head, *tail), 'fthmc_leapfrog')
    return xo, po


def _beta_b(beta, B: int):
    """beta as the per-chain device array of the `_pb` entry points (a tensor of B doubles, used IN PLACE: a replica exchange
    updates it between calls), or None for a Python number: the scalar entry points, untouched."""
    return _expect(beta, B, 'beta (per chain)').view(-1) if isinstance(beta, torch.Tensor) else None


def _plain_trajectory_args(x, v, u, out, keys):
    """what hmc_trajectory and meta_trajectory open with -> (x, v, u, B, L, x_new, results): the fields, the B uniforms, out['x_new']
    (or a fresh field) and the result dict: x_new and the per-chain vector of every key, from `out` where it carries one"""
    x = _field(x); v = _field(v, 'v'); u = _dev(u, 'u').reshape(-1); B, _, L, _ = x.shape
    if u.numel() != B:
        raise FthmcError(f'u: expected {B} uniforms, got {u.numel()}')
    xn = _out_like(None if out is None else out.get('x_new'), x, "out['x_new']")
    return x, v, u, B, L, xn, {'x_new': xn, **{k: _out_vec(out, k, B, x) for k in keys}}


def hmc_trajectory(x, v, u, beta, dt: float, nstep: int, out=None, integrator='leapfrog'):
    """-> dict(x_new, dH, acc, H0, H1), per chain; out: optional dict with any of these to write into (x_new must not be x).
    beta: a number, or a device tensor of B doubles -- per-chain beta (C ABI fthmc_hmc_trajectory_pb)."""
    ic = integrator_code(integrator)
    x, v, u, B, L, xn, r = _plain_trajectory_args(x, v, u, out, ('dH', 'acc', 'H0', 'H1'))
    bb = _beta_b(beta, B)
    if xn.data_ptr() == x.data_ptr():
        raise FthmcError("out['x_new']: must not be x")
    ws, nb = _ws(x, B, L, 0)
    lib, head, step = _lib.load(), (_p(x), _p(v), _p(u), B, L), (float(dt), int(nstep))
    tail = (_p(xn), _p(r['dH']), _p(r['acc']), _p(r['H0']), _p(r['H1']), ws, nb, _stream(x))
    # the entry point decides which kernel instance runs: a tensor beta -> _pb, 'leapfrog' with a number -> the old one, else _int
    if bb is not None:
        check(lib.fthmc_hmc_trajectory_pb(*head, _p(bb), *step, ic, *tail), 'fthmc_hmc_trajectory_pb')
    elif ic:
        check(lib.fthmc_hmc_trajectory_int(*head, float(beta), *step, ic, *tail), 'fthmc_hmc_trajectory_int')
    else:
        check(lib.fthmc_hmc_trajectory(*head, float(beta), *step, *tail), 'fthmc_hmc_trajectory')
    return r


# ---------------------------------------------------------------- replica exchange (parallel tempering)
def ladder_init(betas, n_ladders: int, device=None):
    """M = n_ladders ladders of K = len(betas) consecutive chains, every ladder in order (C ABI fthmc_ladder_init) ->
    dict(betas [K], beta_b [M K], rung [M K] int32, chain_of [M K] int32) on the device.  betas: strictly increasing."""
    import ctypes
    bl = [float(b) for b in betas]
    K, M = len(bl), int(n_ladders)
    if K < 2 or M < 1 or any(not (bl[k] < bl[k + 1]) for k in range(K - 1)):
        raise ValueError(f'ladder_init: at least two strictly increasing betas and one ladder expected, got {bl}, {M}')
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    r = {'betas': torch.empty(K, dtype=torch.float64, device=dev), 'beta_b': torch.empty(M * K, dtype=torch.float64, device=dev),
         'rung': torch.empty(M * K, dtype=torch.int32, device=dev), 'chain_of': torch.empty(M * K, dtype=torch.int32, device=dev)}
    host = (ctypes.c_double * K)(*bl)
    with torch.cuda.device(dev):
        check(_lib.load().fthmc_ladder_init(host, K, M, _p(r['betas']), _p(r['beta_b']), _p(r['rung']), _p(r['chain_of']),
                                            _stream(r['betas'])), 'fthmc_ladder_init')
    return r


def replica_swap(betas, C, u, beta_b, rung, chain_of, parity: int, out: Optional[dict] = None):
    """One round of replica exchange over the M = B / K ladders of K = len(betas) consecutive chains (C ABI fthmc_replica_swap):
    for every pair of neighbouring rungs k = parity (mod 2), accept iff u[m, k] < exp((beta_k - beta_{k+1}) (C_c - C_a)), C = sum
    cos P per chain (row 1 of the beta-free state).  beta_b, rung and chain_of are updated IN PLACE; fields never move.
    -> dict(swap_acc [M, K - 1] (1, 0, or -1: not attempted in this round), d [M, K - 1]); `out` may carry both."""
    betas = _dev(betas, 'betas').view(-1); K = betas.numel()
    if isinstance(beta_b, torch.Tensor) and not beta_b.is_contiguous():
        raise FthmcError('beta_b: expected a contiguous tensor (it is updated in place)')
    beta_b = _dev(beta_b, 'beta_b').view(-1); B = beta_b.numel()
    if K < 2 or B % K != 0 or B == 0:
        raise FthmcError(f'replica_swap: {B} chains do not form whole ladders of {K} rungs')
    M = B // K
    C = _dev(C, 'C').reshape(-1); u = _dev(u, 'u').reshape(-1)
    if C.numel() != B or u.numel() != M * (K - 1):
        raise FthmcError(f'replica_swap: expected C [{B}] and u [{M}, {K - 1}]')
    _expect(rung, B, 'rung', torch.int32); _expect(chain_of, B, 'chain_of', torch.int32)
    if int(parity) not in (0, 1):
        raise ValueError(f'parity: 0 or 1, got {parity!r}')
    if out is None:
        out = {}
    for k in ('swap_acc', 'd'):
        out[k] = _out(out.get(k), (M, K - 1), f'out[{k!r}]', beta_b.device)
    with torch.cuda.device(beta_b.device):
        check(_lib.load().fthmc_replica_swap(_p(betas), K, M, int(parity), _p(C), _p(u), _p(beta_b), _p(rung), _p(chain_of),
                                             _p(out['swap_acc']), _p(out['d']), _stream(beta_b)), 'fthmc_replica_swap')
    return out


# ---------------------------------------------------------------- coupling layer
def _w1(w, x, arch=None):
    """-> (one layer's weights, flat and tagged; the call's fthmc_arch_t*; the shape)"""
    a = arch_of(w, arch)
    npl = arch_params(a)
    w = _tag(_dev(w, 'w').reshape(-1), w, a)
    if w.numel() != npl:
        raise FthmcError(f'w: expected {npl} doubles for one layer of net shape {a}, got {w.numel()}')
    return w, _arch(a), a


def flow_layer_fwd(x, w, mu: int, off: int, act='silu', arch=None, inplace=False):
    """-> (y, logJ); inplace: y IS x (a contiguous float64 device tensor, updated where the layer changes it)."""
    x = _field(x); w, ap, a = _w1(w, x, arch); B, _, L, _ = x.shape
    y = x if inplace else torch.empty_like(x); logJ = torch.empty(B, dtype=x.dtype, device=x.device)
    ws, nb = _ws(x, B, L, 1, arch=a)
    check(_lib.load().fthmc_flow_layer_fwd(_p(x), _p(w), ap, B, L, int(mu), int(off), act_code(act), _p(y), _p(logJ),
                                           ws, nb, _stream(x)), 'fthmc_flow_layer_fwd')
    return y, logJ


def flow_layer_bwd(x, w, gy, glogJ, mu: int, off: int, act='silu', need_gw=False, arch=None):
    x = _field(x); w, ap, a = _w1(w, x, arch); gy = _field(gy, 'gy'); glogJ = _dev(glogJ, 'glogJ').reshape(-1)
    B, _, L, _ = x.shape
    gx = torch.empty_like(x)
    gw = _tag(torch.empty(w.numel(), dtype=x.dtype, device=x.device), w) if need_gw else None
    ws, nb = _ws(x, B, L, 1, train=need_gw, arch=a)
    check(_lib.load().fthmc_flow_layer_bwd(_p(x), _p(w), ap, _p(gy), _p(glogJ), B, L, int(mu), int(off), act_code(act),
                                           _p(gx), _p(gw), ws, nb, _stream(x)), 'fthmc_flow_layer_bwd')
    return gx, gw


def flow_layer_fwd_stash(x, w, mu: int, off: int, act='silu', arch=None, inplace=False, stash=None):
    """-> (y, logJ, stash): the layer forward that keeps its activations for `flow_layer_bwd_stash` (stash is None where
    the kernels have none -- the VALU variant: use flow_layer_bwd then); inplace: as in `flow_layer_fwd`; stash: a float64
    device tensor of fthmc_layer_stash_bytes / 8 entries to write into (the kernel leaves the entries no backward reads as
    they are)."""
    x = _field(x); w, ap, a = _w1(w, x, arch); B, _, L, _ = x.shape
    nbytes = int(_lib.load().fthmc_layer_stash_bytes(ap, B, L))
    if nbytes == 0:
        return (*flow_layer_fwd(x, w, mu, off, act, arch=a, inplace=inplace), None)
    y = x if inplace else torch.empty_like(x); logJ = torch.empty(B, dtype=x.dtype, device=x.device)
    stash = _out(stash, (nbytes // 8,), 'stash', x.device)
    ws, nb = _ws(x, B, L, 1, arch=a)
    check(_lib.load().fthmc_flow_layer_fwd_stash(_p(x), _p(w), ap, B, L, int(mu), int(off), act_code(act), _p(y), _p(logJ),
                                                 _p(stash), ws, nb, _stream(x)), 'fthmc_flow_layer_fwd_stash')
    return y, logJ, stash


def flow_layer_bwd_stash(stash, shape, w, gy, glogJ, mu: int, off: int, act='silu', need_gw=False, arch=None):
    """VJP of the layer from the stash of `flow_layer_fwd_stash` (`shape` = that call's x.shape): nothing recomputed."""
    w_, ap, a = _w1(w, gy, arch); gy = _field(gy, 'gy'); glogJ = _dev(glogJ, 'glogJ').reshape(-1)
    B, _, L, _ = shape
    gx = torch.empty_like(gy)
    gw = _tag(torch.empty(w_.numel(), dtype=gy.dtype, device=gy.device), w_) if need_gw else None
    ws, nb = _ws(gy, B, L, 1, train=need_gw, arch=a)
    check(_lib.load().fthmc_flow_layer_bwd_stash(_p(stash), _p(w_), ap, _p(gy), _p(glogJ), B, L, int(mu), int(off), act_code(act),
                                                 _p(gx), _p(gw), ws, nb, _stream(gy)), 'fthmc_flow_layer_bwd_stash')
    return gx, gw


def flow_layer_rev(y, w, mu: int, off: int, act='silu', tol: float = 1e-12, arch=None):
    y = _field(y, 'y'); w, ap, a = _w1(w, y, arch); B, _, L, _ = y.shape
    x = torch.empty_like(y); logJ = torch.empty(B, dtype=y.dtype, device=y.device)
    ws, nb = _ws(y, B, L, 1, arch=a)
    check(_lib.load().fthmc_flow_layer_rev(_p(y), _p(w), ap, B, L, int(mu), int(off), act_code(act), float(tol),
                                           _p(x), _p(logJ), ws, nb, _stream(y)), 'fthmc_flow_layer_rev')
    return x, logJ


def _plaq_field(P, name='P'):
    P = _dev(P, name)
    if P.dim() != 3 or P.shape[1] != P.shape[2] or P.shape[1] % 4 != 0:
        raise FthmcError(f'{name}: expected a plaquette field [B, L, L] with L % 4 == 0, got {tuple(P.shape)}')
    return P


def plaq_coupling_fwd(P, w, mu: int, off: int, act='silu', arch=None):
    """NCPPlaqCouplingLayer.forward on a plaquette field [B, L, L] -> (fP, logJ[B])."""
    P = _plaq_field(P); B, L, _ = P.shape
    w, ap, a = _w1(w, P, arch)
    fP = torch.empty_like(P); logJ = torch.empty(B, dtype=P.dtype, device=P.device)
    ws, nb = _ws(P, B, L, 1, arch=a)
    check(_lib.load().fthmc_plaq_coupling_fwd(_p(P), _p(w), ap, B, L, int(mu), int(off), act_code(act), _p(fP), _p(logJ),
                                              ws, nb, _stream(P)), 'fthmc_plaq_coupling_fwd')
    return fP, logJ


def plaq_coupling_bwd(P, w, gfP, glogJ, mu: int, off: int, act='silu', need_gw=False, arch=None):
    """VJP of plaq_coupling_fwd: -> (gP, gw or None) for the upstream gradients gfP [B, L, L] and glogJ [B]."""
    P = _plaq_field(P); gfP = _plaq_field(gfP, 'gfP'); B, L, _ = P.shape
    glogJ = _dev(glogJ, 'glogJ').reshape(-1)
    if gfP.shape != P.shape or glogJ.numel() != B:
        raise FthmcError('plaq_coupling_bwd: gfP must be shaped like P, glogJ [B]')
    w, ap, a = _w1(w, P, arch)
    gP = torch.empty_like(P)
    gw = _tag(torch.empty(w.numel(), dtype=P.dtype, device=P.device), w) if need_gw else None
    ws, nb = _ws(P, B, L, 1, train=need_gw, arch=a)
    check(_lib.load().fthmc_plaq_coupling_bwd(_p(P), _p(w), ap, _p(gfP), _p(glogJ), B, L, int(mu), int(off), act_code(act),
                                              _p(gP), _p(gw), ws, nb, _stream(P)), 'fthmc_plaq_coupling_bwd')
    return gP, gw


def plaq_coupling_rev(fP, w, mu: int, off: int, act='silu', tol: float = 1e-12, arch=None):
    """NCPPlaqCouplingLayer.reverse on a plaquette field [B, L, L] -> (P, logJ[B])."""
    fP = _plaq_field(fP, 'fP'); B, L, _ = fP.shape
    w, ap, a = _w1(w, fP, arch)
    P = torch.empty_like(fP); logJ = torch.empty(B, dtype=fP.dtype, device=fP.device)
    ws, nb = _ws(fP, B, L, 1, arch=a)
    check(_lib.load().fthmc_plaq_coupling_rev(_p(fP), _p(w), ap, B, L, int(mu), int(off), act_code(act), float(tol),
                                              _p(P), _p(logJ), ws, nb, _stream(fP)), 'fthmc_plaq_coupling_rev')
    return P, logJ


# ---------------------------------------------------------------- whole flow
def _wall(w, n_layers, arch=None):
    """-> (all layers' weights, flat and tagged; the call's fthmc_arch_t*; the shape); (None, NULL, default) without layers"""
    if not n_layers:
        return None, None, DEFAULT_ARCH
    a = arch_of(w, arch)
    npl = arch_params(a)
    w = _tag(_dev(w, 'w').reshape(-1), w, a)
    if w.numel() != n_layers * npl:
        raise FthmcError(f'w: expected {n_layers}*{npl} doubles for net shape {a}, got {w.numel()}')
    return w, _arch(a), a


def flow_forward(x, w, n_layers: int, act='silu', arch=None, wkey=None):
    x = _field(x); B, _, L, _ = x.shape
    w, ap, a = _wall(w, n_layers, arch)
    y = torch.empty_like(x); ld = torch.empty(B, dtype=x.dtype, device=x.device)
    ws, nb = _ws(x, B, L, n_layers, arch=a)
    check(_lib.load().fthmc_flow_forward_v(_p(x), _p(w), ap, n_layers, B, L, act_code(act), _p(y), _p(ld), ws, nb,
                                         _stream(x), weights_version(wkey)), 'fthmc_flow_forward')
    return y, ld


def flow_reverse(y, w, n_layers: int, act='silu', tol: float = 1e-12, arch=None, wkey=None):
    y = _field(y, 'y'); B, _, L, _ = y.shape
    w, ap, a = _wall(w, n_layers, arch)
    x = torch.empty_like(y); ld = torch.empty(B, dtype=y.dtype, device=y.device)
    ws, nb = _ws(y, B, L, n_layers, arch=a)
    check(_lib.load().fthmc_flow_reverse_v(_p(y), _p(w), ap, n_layers, B, L, act_code(act), float(tol), _p(x), _p(ld),
                                         ws, nb, _stream(y), weights_version(wkey)), 'fthmc_flow_reverse')
    return x, ld


def ft_action(x, w, n_layers: int, beta: float, act='silu', arch=None, wkey=None):
    """-> (S_eff, logdet, plaq, Q) each [B]."""
    x = _field(x); B, _, L, _ = x.shape
    w, ap, a = _wall(w, n_layers, arch)
    S, ld, plaq, Q = (torch.empty(B, dtype=x.dtype, device=x.device) for _ in range(4))
    ws, nb = _ws(x, B, L, n_layers, arch=a)
    check(_lib.load().fthmc_ft_action_v(_p(x), _p(w), ap, n_layers, B, L, act_code(act), float(beta), _p(S), _p(ld),
                                      _p(plaq), _p(Q), ws, nb, _stream(x), weights_version(wkey)), 'fthmc_ft_action')
    return S, ld, plaq, Q


def ft_force(x, w, n_layers: int, beta: float, act='silu', arch=None, wkey=None):
    x = _field(x); B, _, L, _ = x.shape
    w, ap, a = _wall(w, n_layers, arch)
    F = torch.empty_like(x)
    ws, nb = _ws(x, B, L, n_layers, arch=a)
    check(_lib.load().fthmc_ft_force_v(_p(x), _p(w), ap, n_layers, B, L, act_code(act), float(beta), _p(F), ws, nb,
                                     _stream(x), weights_version(wkey)), 'fthmc_ft_force')
    return F


def _chains(t, B: int, name: str):
    t = _dev(t, name).reshape(-1)
    if t.numel() != B:
        raise FthmcError(f'{name}: expected {B} per-chain entries, got {t.numel()}')
    return t


def ft_action_vjp(x, w, n_layers: int, beta: float, gS, glogdet=None, act='silu', arch=None, need_gx=True, need_gw=True):
    """-> (gx, gw): d/dx and d/dw of sum_b [gS[b] S_eff[b] + glogdet[b] logdet[b]] (C ABI fthmc_ft_action_vjp: the backward of
    ft_action, autograd of qed_helpers.py:212-223).  gx [B, 2, L, L]; gw flat [n_layers * params] like `w` (empty without
    layers); either is None when not asked for.  Plain kernels for every net shape, deterministic."""
    x = _field(x); B, _, L, _ = x.shape
    w, ap, a = _wall(w, n_layers, arch)
    gS = _chains(gS, B, 'gS')
    glogdet = None if glogdet is None else _chains(glogdet, B, 'glogdet')
    gx = torch.empty_like(x) if need_gx else None
    gw = _tag(torch.zeros(n_layers * arch_params(a), dtype=x.dtype, device=x.device), w, a) if need_gw else None
    if gx is None and not n_layers:
        return gx, gw
    ws, nb = _ws(x, B, L, n_layers, arch=a, vjp=True)
    check(_lib.load().fthmc_ft_action_vjp(_p(x), _p(w), ap, n_layers, B, L, act_code(act), float(beta), _p(gS), _p(glogdet),
                                          _p(gx), _p(gw) if n_layers else None, ws, nb, _stream(x)), 'fthmc_ft_action_vjp')
    return gx, gw


def ft_force_vjp(x, w, n_layers: int, beta: float, g, act='silu', arch=None, need_gx=True, need_gw=True):
    """-> (gx, gw) for the force F = d(sum_b S_eff)/dx (ft_force) and a cotangent g shaped like x: gx = (dF/dx)^T g = H g (the
    Hessian of sum_b S_eff applied to g), gw = d/dw <g, F> flat like `w` (C ABI fthmc_ft_force_vjp: autograd of
    qed_helpers.py:226-242 with create_graph=True).  Dual-number instances of the plain kernels, deterministic."""
    x = _field(x); B, _, L, _ = x.shape
    g = _field(g, 'g')
    if g.shape != x.shape:
        raise FthmcError(f'g: expected {tuple(x.shape)}, got {tuple(g.shape)}')
    w, ap, a = _wall(w, n_layers, arch)
    gx = torch.empty_like(x) if need_gx else None
    gw = _tag(torch.zeros(n_layers * arch_params(a), dtype=x.dtype, device=x.device), w, a) if need_gw else None
    if gx is None and not n_layers:
        return gx, gw
    ws, nb = _ws(x, B, L, n_layers, arch=a, vjp=True)
    check(_lib.load().fthmc_ft_force_vjp(_p(x), _p(w), ap, n_layers, B, L, act_code(act), float(beta), _p(g), _p(gx),
                                         _p(gw) if n_layers else None, ws, nb, _stream(x)), 'fthmc_ft_force_vjp')
    return gx, gw


def ft_leapfrog(x, v, w, n_layers: int, beta: float, dt: float, nstep: int, act='silu', arch=None, wkey=None,
                integrator='leapfrog'):
    """the MD in the latent field -> (x', v'); integrator: 'leapfrog' | 'omelyan' | 'force_gradient' (csrc/integrator.h)"""
    ic = integrator_code(integrator)
    x = _field(x); v = _field(v, 'v'); B, _, L, _ = x.shape
    w, ap, a = _wall(w, n_layers, arch)
    xo, vo = torch.empty_like(x), torch.empty_like(v)
    ws, nb = _ws(x, B, L, n_layers, arch=a)
    lib, wv = _lib.load(), weights_version(wkey)
    args = (_p(x), _p(v), _p(w), ap, n_layers, B, L, act_code(act), float(beta), float(dt), int(nstep), _p(xo), _p(vo), ws, nb, _stream(x))
    if ic:                                        # 'leapfrog' keeps its own entry point (another instance of the one-launch kernel)
        check(lib.fthmc_ft_md_v(*args, ic, wv), 'fthmc_ft_md')
    else:
        check(lib.fthmc_ft_leapfrog_v(*args, wv), 'fthmc_ft_leapfrog')
    return xo, vo


_SIDE_STREAMS: dict = {}


def default_groups(B: int, L: int) -> int:
    """Two chain groups once a launch is large enough to amortise the extra launches (measured: +10 % at
    B=128, L=64; -50 % at B=32, L=16 where the sequence is launch-bound)."""
    if L <= 16 and get_small_path() and get_variant() == 1:
        return 1              # small lattices: a sweep is ONE launch with a workgroup per chain, there is no tail to fill
    return 2 if B >= 16 and B * L * L >= (1 << 17) else 1


def default_train_groups(B: int, L: int) -> int:
    """Chain groups of a training gradient.  On the shapes the fused training backward serves (csrc/flow_bwd_train.hip: L a power
    of two >= 32) ONE: that kernel holds a CU by itself (141 KB of LDS, 241 VGPRs), a second stream finds no room beside it and
    only halves the walks (measured at the config-5 shard: 7.11 ms on one stream, 7.20-7.25 on two; level since the layers'
    partials are reduced in one go); elsewhere as the sampler."""
    if L >= 32 and (L & (L - 1)) == 0 and get_variant() == 1:
        return 1
    return default_groups(B, L)


def _side_streams(device, n: int):
    key = device.index
    pool = _SIDE_STREAMS.setdefault(key, [])
    while len(pool) < n:
        pool.append(torch.cuda.Stream(device=device))
    return pool[:n]


def _chain_groups(device, edges, side_streams=None):
    """The fork and join of a call that runs the chain groups lo .. hi - 1 of `edges` (_group_edges) on concurrent streams.  A
    generator: the side streams (the caller's `side_streams`, else this device's pool) wait for the current stream before
    anything of the call is on it; then (lo, hi, stream) of the groups 1 .. G - 1 on the side streams and of group 0, last, on
    the current stream -- the caller enqueues a group's work under torch.cuda.stream(stream) --; behind the last group the current
    stream waits for the side streams."""
    G = len(edges) - 1
    main = torch.cuda.current_stream(device)
    sides = [] if G == 1 else list(side_streams)[:G - 1] if side_streams is not None else _side_streams(device, G - 1)
    if len(sides) != G - 1:
        raise FthmcError(f'side_streams: {G - 1} streams needed for {G} chain groups')
    for st in sides:
        st.wait_stream(main)
    for gi in list(range(1, G)) + [0]:
        yield edges[gi], edges[gi + 1], main if gi == 0 else sides[gi - 1]
    for st in sides:
        main.wait_stream(st)


def _meta_group_rows(table, B: int, edges):
    """the table rows of the chain groups of `edges` -> [(row_lo, row_hi) or None (the whole table)]: with one row every group reads
    it; otherwise a group must be whole rows (every edge a multiple of B / G), and is handed its own"""
    G = 1 if table.dim() == 1 else table.shape[0]
    if G == 1:
        return [None] * (len(edges) - 1)
    if G < 1 or B % G:
        raise ValueError(f'meta table: {G} rows do not divide the {B} chains')
    cpr = B // G
    if any(e % cpr for e in edges):
        raise ValueError(f'groups: the edges {tuple(edges)} split a table row ({cpr} chains per row): every chain group must be whole rows')
    return [(edges[k] // cpr, edges[k + 1] // cpr) for k in range(len(edges) - 1)]


def _ft_trajectory(x, v, u, w, n_layers, beta, dt, nstep, act, mode, out, state_in, groups, arch, wkey, side_streams, integrator,
                   bias=None, defect=None):
    """The body of ft_trajectory and, with bias = (table, qmax, wall), of ft_meta_trajectory, with defect = (g_b, (i0, j0, Ld)) of
    ft_defect_trajectory: the checks, the result tensors (the state has nrow = 3 rows, 4 with a bias or a defect), the chain-group
    fork (a group is handed its own table rows, its own slice of g_b) and the C call, chosen by (bias, defect, per-chain beta,
    integrator)."""
    ic = integrator_code(integrator)
    if ic and mode not in ('md',):
        raise ValueError(f'mode {mode!r} discards the MD: it goes with integrator=\'leapfrog\' only, got {integrator!r}')
    x = _field(x); v = _field(v, 'v'); u = _dev(u, 'u').reshape(-1); B, _, L, _ = x.shape
    if u.numel() != B:
        raise FthmcError(f'u: expected {B} uniforms, got {u.numel()}')
    bb = _beta_b(beta, B)
    if bb is not None and mode != 'md':
        raise ValueError(f'a per-chain beta goes with mode \'md\' only, got {mode!r}')
    nrow, keys, tab = 3, ('dH', 'acc', 'H0', 'H1', 'plaq', 'Q'), None
    if bias is not None:
        if int(nstep) < 1:
            raise ValueError(f'ft_meta_trajectory: nstep >= 1 expected, got {nstep}')
        nrow, keys, tab = 4, keys + ('qm', 'vbias'), _meta_table(bias[0], B, *bias[1:])
    if defect is not None:
        if int(nstep) < 1:
            raise ValueError(f'ft_defect_trajectory: nstep >= 1 expected, got {nstep}')
        if bb is not None:
            raise ValueError('ft_defect_trajectory: ONE beta per call (a number); the couplings of the chains are g_b')
        nrow, keys, dfa = 4, keys + ('dsum',), _defect_args(beta, defect[0], defect[1], B, L)
    edges = _group_edges(groups, B)                                     # an int, or explicit group sizes (chains per group)
    rows = _meta_group_rows(bias[0], B, edges) if bias is not None else None      # raises before anything is launched
    w, ap, a = _wall(w, n_layers, arch)
    out = {} if out is None else out
    if 'x_new' not in out:
        out['x_new'] = torch.empty_like(x)
    for k in keys:
        if k not in out:
            out[k] = torch.empty(B, dtype=x.dtype, device=x.device)
    if 'state' not in out:
        out['state'] = torch.empty(nrow, B, dtype=x.dtype, device=x.device)
    if state_in is not None:
        state_in = _dev(state_in, 'state_in')
        if state_in.numel() != nrow * B:
            raise FthmcError(f'state_in: expected [{nrow}, {B}]')
        state_in = state_in.reshape(nrow, B)
    if len(edges) > 2:
        parts = []
        for lo, hi, st in _chain_groups(x.device, edges, side_streams):
            r = rows[edges.index(lo)] if rows else None
            with torch.cuda.stream(st):
                og = {k: t[lo:hi] for k, t in out.items() if k != 'state'}
                sg = state_in[:, lo:hi].contiguous() if state_in is not None else None
                bg = bias if r is None else (bias[0][r[0]:r[1]],) + tuple(bias[1:])
                dg = None if defect is None else (defect[0].view(-1)[lo:hi], defect[1])
                _ft_trajectory(x[lo:hi], v[lo:hi], u[lo:hi], w, n_layers, beta if bb is None else bb[lo:hi], dt, nstep, act, mode, og,
                               sg, 1, a, wkey, None, integrator, bg, dg)  # one group: no side streams
                out['state'][:, lo:hi].copy_(og['state'])
                parts.append(og)                                        # keep the group's temporaries alive until the join
        return out
    m = {'md': MODE_MD, 'literal': MODE_LITERAL, 'reference_literal': MODE_LITERAL}[mode]
    ws, nb = _ws(x, B, L, n_layers, arch=a, meta=bias is not None, defect=defect is not None)
    lib, wv = _lib.load(), weights_version(wkey)
    head = (_p(x), _p(v), _p(u), _p(w), ap, n_layers, B, L, act_code(act))
    res = tuple(_p(out[k]) for k in ('x_new',) + keys)
    tail = (_p(state_in), _p(out['state']), ws, nb, _stream(x))
    # the entry point decides which kernel instance runs: a table -> _meta, a tensor beta -> _pb, 'leapfrog' with a number -> the
    # old one, else _int
    if bias is not None:
        check(lib.fthmc_ft_meta_trajectory_v(*head, float(beta), float(dt), int(nstep), ic, *tab, *res, *tail, wv), 'fthmc_ft_meta_trajectory')
    elif defect is not None:
        check(lib.fthmc_ft_defect_trajectory_v(*head, *dfa, float(dt), int(nstep), ic, *res, *tail, wv), 'fthmc_ft_defect_trajectory')
    elif bb is not None:
        check(lib.fthmc_ft_trajectory_pb_v(*head, _p(bb), float(dt), int(nstep), m, *res, *tail, ic, wv), 'fthmc_ft_trajectory_pb')
    elif ic:
        check(lib.fthmc_ft_trajectory_int_v(*head, float(beta), float(dt), int(nstep), m, *res, *tail, ic, wv), 'fthmc_ft_trajectory_int')
    else:
        check(lib.fthmc_ft_trajectory_v(*head, float(beta), float(dt), int(nstep), m, *res, *tail, wv), 'fthmc_ft_trajectory')
    return out


def ft_trajectory(x, v, u, w, n_layers: int, beta, dt: float, nstep: int, act='silu', mode='md',
                  out: Optional[dict] = None, state_in: Optional[torch.Tensor] = None, groups: int = 1, arch=None, wkey=None,
                  side_streams=None, integrator='leapfrog'):
    """One ftHMC trajectory per chain -> dict(x_new, dH, acc, H0, H1, plaq, Q, state).

    `out` may carry preallocated output tensors (same keys) so that a caller can replay the call
    inside a captured graph.  `state` is [3, B] = (S_eff, plaq, Q) of x_new; fed back as `state_in`
    of the next trajectory of the same chains (x = x_new) it saves that call's H0 flow sweep.

    groups > 1 splits the chains into that many contiguous groups (a list gives the group sizes) whose trajectories
    run on concurrent streams (forked from and joined back into the current stream, each with its own workspace):
    chains are independent, and one group's kernels fill the CUs that the other's leave idle in every kernel
    tail and dispatch gap.  Results do not depend on `groups`.

    integrator: 'leapfrog' | 'omelyan' | 'force_gradient' -- the MD between the two energies (csrc/integrator.h; nstep steps cost
    integrator_forces(integrator, nstep) force evaluations); mode 'literal' discards the MD and takes 'leapfrog' only.

    beta: a number, or a device tensor of B doubles -- per-chain beta (C ABI fthmc_ft_trajectory_pb_v; mode 'md' only), read in
    place.  `state` is then the BETA-FREE triple [3, B] = (log det J, sum cos P, Q) of x_new, valid as `state_in` under any beta."""
    return _ft_trajectory(x, v, u, w, n_layers, beta, dt, nstep, act, mode, out, state_in, groups, arch, wkey, side_streams, integrator)


# ---------------------------------------------------------------- metadynamics through the flow
def ft_meta_trajectory(x, v, u, w, n_layers: int, beta: float, dt: float, nstep: int, table, qmax: float, wall: float = 0.0, act='silu',
                       integrator='leapfrog', out: Optional[dict] = None, state_in: Optional[torch.Tensor] = None, groups: int = 1,
                       arch=None, wkey=None, side_streams=None):
    """One ftHMC trajectory per chain under the bias V(Q_m) of the PHYSICAL field F(x) (C ABI fthmc_ft_meta_trajectory_v; mode 'md')
    -> dict(x_new, dH, acc, H0, H1, plaq, Q, qm, vbias, state): ft_trajectory's keys, qm / vbias = Q_m and V(Q_m) of F(x_new) under
    the table the call ran on, and state [4, B] = (S_eff without the bias, plaq, Q, Q_m) of x_new.  The state is table-free: fed back
    as `state_in` it stays valid across meta_deposit calls.  table, qmax, wall: as meta_trajectory.  groups, out, wkey, side_streams:
    as ft_trajectory; with more than one table row every chain group must be whole rows.  Results do not depend on `groups`."""
    return _ft_trajectory(x, v, u, w, n_layers, beta, dt, nstep, act, 'md', out, state_in, groups, arch, wkey, side_streams, integrator,
                          bias=(table, qmax, wall))


def ft_meta_force(x, w, n_layers: int, beta: float, table, qmax: float, wall: float = 0.0, act='silu', arch=None, wkey=None):
    """F = dS_b / dx of S_b(x) = -beta sum cos P(F(x)) - log det J(x) + V(Q_m(F(x))) (C ABI fthmc_ft_meta_force_v), ft_force's sign"""
    x = _field(x); B, _, L, _ = x.shape
    tab = _meta_table(table, B, qmax, wall)
    w, ap, a = _wall(w, n_layers, arch)
    F = torch.empty_like(x)
    ws, nb = _ws(x, B, L, n_layers, arch=a, meta=True)
    check(_lib.load().fthmc_ft_meta_force_v(_p(x), _p(w), ap, n_layers, B, L, act_code(act), float(beta), *tab, _p(F), ws, nb, _stream(x),
                                            weights_version(wkey)), 'fthmc_ft_meta_force')
    return F


def ft_meta_action(x, w, n_layers: int, beta: float, table, qmax: float, wall: float = 0.0, act='silu', arch=None, wkey=None):
    """-> (S_b, logdet, Q_m, V(Q_m)) per chain, Q_m of the physical field F(x) (C ABI fthmc_ft_meta_action_v)"""
    x = _field(x); B, _, L, _ = x.shape
    tab = _meta_table(table, B, qmax, wall)
    w, ap, a = _wall(w, n_layers, arch)
    S, ld, qm, vb = (torch.empty(B, dtype=x.dtype, device=x.device) for _ in range(4))
    ws, nb = _ws(x, B, L, n_layers, arch=a, meta=True)
    check(_lib.load().fthmc_ft_meta_action_v(_p(x), _p(w), ap, n_layers, B, L, act_code(act), float(beta), *tab, _p(S), _p(ld), _p(qm),
                                             _p(vb), ws, nb, _stream(x), weights_version(wkey)), 'fthmc_ft_meta_action')
    return S, ld, qm, vb


# ---------------------------------------------------------------- boundary-condition tempering through the flow
def ft_defect_trajectory(x, v, u, w, n_layers: int, beta: float, g_b, defect, dt: float, nstep: int, act='silu', integrator='leapfrog',
                         out: Optional[dict] = None, state_in: Optional[torch.Tensor] = None, groups: int = 1, arch=None, wkey=None,
                         side_streams=None):
    """One ftHMC trajectory per chain whose PHYSICAL field F(x) carries the defect of defect_trajectory (C ABI
    fthmc_ft_defect_trajectory_v; mode 'md'): S(x) = -beta C + (beta - g_b) Dsum - log det J(x), C and Dsum the cosine sums of F(x)
    -> dict(x_new, dH, acc, H0, H1, plaq, Q, dsum, state): ft_trajectory's keys, dsum = Dsum of F(x_new), and state [4, B] = (S_eff of
    the periodic action, plaq, Q, Dsum) of x_new.  The state is g-free: fed back as `state_in` it stays valid when a replica exchange
    has changed g_b in between.  g_b: a float64 device tensor [B] read in place; defect = (i0, j0, Ld).  groups, out, wkey,
    side_streams: as ft_trajectory; every chain group is handed its slice of g_b.  Results do not depend on `groups`."""
    return _ft_trajectory(x, v, u, w, n_layers, beta, dt, nstep, act, 'md', out, state_in, groups, arch, wkey, side_streams, integrator,
                          defect=(g_b, defect))


def ft_defect_force(x, w, n_layers: int, beta: float, g_b, defect, act='silu', arch=None, wkey=None):
    """F = dS / dx of S(x) = -beta C + (beta - g_b) Dsum - log det J(x) on the physical field F(x) (C ABI fthmc_ft_defect_force_v),
    ft_force's sign"""
    x = _field(x); B, _, L, _ = x.shape
    df = _defect_args(beta, g_b, defect, B, L)
    w, ap, a = _wall(w, n_layers, arch)
    F = torch.empty_like(x)
    ws, nb = _ws(x, B, L, n_layers, arch=a, defect=True)
    check(_lib.load().fthmc_ft_defect_force_v(_p(x), _p(w), ap, n_layers, B, L, act_code(act), *df, _p(F), ws, nb, _stream(x),
                                              weights_version(wkey)), 'fthmc_ft_defect_force')
    return F


def ft_defect_action(x, w, n_layers: int, beta: float, g_b, defect, act='silu', arch=None, wkey=None):
    """-> (S, logdet, csum, dsum, Q) per chain, the sums and the integer charge of the physical field F(x) (C ABI
    fthmc_ft_defect_action_v)"""
    x = _field(x); B, _, L, _ = x.shape
    df = _defect_args(beta, g_b, defect, B, L)
    w, ap, a = _wall(w, n_layers, arch)
    S, ld, cs, ds, Q = (torch.empty(B, dtype=x.dtype, device=x.device) for _ in range(5))
    ws, nb = _ws(x, B, L, n_layers, arch=a, defect=True)
    check(_lib.load().fthmc_ft_defect_action_v(_p(x), _p(w), ap, n_layers, B, L, act_code(act), *df, _p(S), _p(ld), _p(cs), _p(ds), _p(Q),
                                               ws, nb, _stream(x), weights_version(wkey)), 'fthmc_ft_defect_action')
    return S, ld, cs, ds, Q


def train_grad(xi, w, n_layers: int, beta: float, act='silu', need_gw=True, groups: int = 1, _out=None, out_gw=None, arch=None):
    """-> dict(x, logq, logp, gw): pieces of train.train_step for a fixed prior draw; gw = gradient of
    mean_b (logq - logp) wrt the packed weights (written into `out_gw` when given: a contiguous float64 device tensor
    of w.numel() entries, e.g. the flat gradient buffer the conv parameters' .grad are views of).

    groups > 1: the chains are split into contiguous groups (a list gives the group sizes) that run on concurrent streams (as in
    ft_trajectory); the groups' weight gradients are combined with weights B_g / B."""
    xi = _field(xi, 'xi'); B, _, L, _ = xi.shape
    w, ap, arch_ = _wall(w, n_layers, arch)
    if out_gw is not None:
        _expect(out_gw, w.numel(), 'train_grad: out_gw')
    if _out is None:
        x = torch.empty_like(xi)
        logq, logp = (torch.empty(B, dtype=xi.dtype, device=xi.device) for _ in range(2))
    else:
        x, logq, logp = _out
    edges = _group_edges(groups, B)
    if len(edges) > 2:
        gws = torch.empty(len(edges) - 1, w.numel(), dtype=xi.dtype, device=xi.device) if need_gw else None
        for lo, hi, st in _chain_groups(xi.device, edges):
            with torch.cuda.stream(st):
                r = train_grad(xi[lo:hi], w, n_layers, beta, act, need_gw, 1, (x[lo:hi], logq[lo:hi], logp[lo:hi]), arch=arch_)
                if need_gw:
                    torch.mul(r['gw'], (hi - lo) / B, out=gws[edges.index(lo)])    # row g for group g: the sum below adds in group order
        if need_gw and out_gw is not None:
            torch.sum(gws, 0, out=out_gw)
        return {'x': x, 'logq': logq, 'logp': logp,
                'gw': _tag(out_gw if out_gw is not None else gws.sum(0), w) if need_gw else None}
    gw = _tag(out_gw.reshape(-1) if out_gw is not None else torch.empty(w.numel(), dtype=xi.dtype, device=xi.device), w) \
        if need_gw else None
    ws, nb = _ws(xi, B, L, n_layers, train=True, arch=arch_)
    check(_lib.load().fthmc_train_grad(_p(xi), _p(w), ap, n_layers, B, L, act_code(act), float(beta), _p(x), _p(logq),
                                       _p(logp), _p(gw), ws, nb, _stream(xi)), 'fthmc_train_grad')
    return {'x': x, 'logq': logq, 'logp': logp, 'gw': gw}


def train_force_grad(xi, w, n_layers: int, beta: float, act='silu', need_gw=True, out_gw=None, arch=None):
    """-> dict(F, force_sq, gw): the force-norm training step's pieces at a fixed field `xi` (C ABI fthmc_train_force_grad,
    ipynb/ft_hmc.py:253-299): F = d(sum_b S_eff)/dxi [B, 2, L, L] (what ft_force returns), force_sq[b] = sum F_b^2, and
    gw = d(sum_b force_sq[b])/dw flat like `w` (written into `out_gw` when given, with train_grad's contract: a contiguous
    float64 device tensor of w.numel() entries, e.g. the flat gradient buffer); gw is None with need_gw=False or no layers."""
    xi = _field(xi, 'xi'); B, _, L, _ = xi.shape
    w, ap, a = _wall(w, n_layers, arch)
    need_gw = bool(need_gw and n_layers)
    if out_gw is not None and need_gw:
        _expect(out_gw, w.numel(), 'train_force_grad: out_gw')
    F = torch.empty_like(xi)
    fsq = torch.empty(B, dtype=xi.dtype, device=xi.device)
    gw = None
    if need_gw:
        gw = _tag(out_gw.reshape(-1) if out_gw is not None else torch.empty(w.numel(), dtype=xi.dtype, device=xi.device), w, a)
    ws, nb = _ws(xi, B, L, n_layers, arch=a, force=True)
    check(_lib.load().fthmc_train_force_grad(_p(xi), _p(w), ap, n_layers, B, L, act_code(act), float(beta), _p(F), _p(fsq),
                                             _p(gw), ws, nb, _stream(xi)), 'fthmc_train_force_grad')
    return {'F': F, 'force_sq': fsq, 'gw': gw}


def time_kernel(kind: str, x, w=None, mu=0, off=0, act='silu', beta=1.0, reps=20) -> float:
    """Average milliseconds per launch of one kernel ('flow_fwd', 'flow_bwd', 'leap_step', 'hmc_trajectory'),
    measured with HIP events on the current stream (synchronises)."""
    import ctypes
    x = _field(x); B, _, L, _ = x.shape
    k = {'flow_fwd': 0, 'flow_bwd': 1, 'leap_step': 2, 'hmc_trajectory': 3}[kind]
    wp = _p(_w1(w, x)[0]) if k < 2 else None
    ms = ctypes.c_double(0.0)
    ws, nb = _ws(x, B, L, 1)
    check(_lib.load().fthmc_time_kernel(k, _p(x), wp, None, B, L, int(mu), int(off), act_code(act), float(beta),
                                        int(reps), ctypes.byref(ms), ws, nb, _stream(x)), 'fthmc_time_kernel')
    return ms.value


def profile_stages(kind: str, x, w, mu=0, off=0, act='silu', beta=1.0):
    """Mean cycles per stage of one MFMA coupling-layer kernel launch ('flow_fwd' | 'flow_bwd' | 'flow_bwd_train' | 'flow_wgrad')."""
    import ctypes
    x = _field(x); B, _, L, _ = x.shape
    k = {'flow_fwd': 0, 'flow_bwd': 1, 'flow_bwd_train': 2, 'flow_wgrad': 3}[kind]
    buf = (ctypes.c_double * 16)()
    ws, nb = _ws(x, B, L, 1, train=(k >= 2))
    check(_lib.load().fthmc_profile_stages(k, _p(x), _p(_w1(w, x)[0]), None, B, L, int(mu), int(off), act_code(act),
                                           float(beta), buf, ws, nb, _stream(x)), 'fthmc_profile_stages')
    return list(buf)


def small_profile(x, v, u, w, n_layers: int, beta: float, dt: float, nstep: int, act='silu'):
    """Mean cycles per stage (32 slots, include/fthmc_hip.h) of one trajectory on the small-lattice fused path."""
    import ctypes
    x = _field(x); v = _field(v, 'v'); u = _dev(u, 'u').reshape(-1); B, _, L, _ = x.shape
    buf = (ctypes.c_double * 32)()
    ws, nb = _ws(x, B, L, n_layers)
    check(_lib.load().fthmc_small_profile(_p(x), _p(v), _p(u), _p(_wall(w, n_layers)[0]), None, n_layers, B, L, act_code(act), float(beta),
                                          float(dt), int(nstep), buf, ws, nb, _stream(x)), 'fthmc_small_profile')
    return list(buf)


def time_small(x, v, u, w, n_layers: int, beta: float, dt: float, nstep: int, act='silu', reps=20) -> float:
    """Average milliseconds per launch of the small-lattice fused trajectory kernel (HIP events on the current stream)."""
    import ctypes
    x = _field(x); v = _field(v, 'v'); u = _dev(u, 'u').reshape(-1); B, _, L, _ = x.shape
    ms = ctypes.c_double(0.0)
    ws, nb = _ws(x, B, L, n_layers)
    check(_lib.load().fthmc_time_small(_p(x), _p(v), _p(u), _p(_wall(w, n_layers)[0]), None, n_layers, B, L, act_code(act), float(beta),
                                       float(dt), int(nstep), int(reps), ctypes.byref(ms), ws, nb, _stream(x)), 'fthmc_time_small')
    return ms.value
