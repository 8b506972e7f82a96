"""GPU: the weight gradients of the default net where a workgroup WALKS several (chain, tile) items, against the oracle's autograd.

k_flow_wgrad (csrc/flow_wgrad.hip: the two-kernel form) and k_flow_bwd_train (csrc/flow_bwd_train.hip: the fused training backward)
keep their accumulators in registers across the items of a walk, prefetch item i + 1 under item i, reuse LDS planes behind
barriers and write one partial row per workgroup; the host sizes the rows from formulas of its own (csrc/kernels.h).  A walk
starts at 1024 items a launch (two-kernel form) and the fused kernel first reuses a double buffer at a walk of three: the shapes
here are the smallest that get there (tests/walk_model.py LAYER_SHAPES, TRAIN_SHAPES; tests/test_walk_maps.py checks on the CPU
that they walk as listed, and every case asserts it again before it runs).  Every chain and tile carries data of its own (random
links, random upstream gradients, random d/dlogJ per chain), so an item dropped, taken twice or read from the wrong place moves
the result; the whole batch is compared, nothing is sampled.

Bounds (none of them taken from the kernels): weight gradients max|gpu - oracle| / max(1, max|oracle|) <= 1e-10 per parameter
tensor -- the atol factor of tests/test_layer_calls_gpu.py and test_training_gpu.py; the oracle's own noise under a permutation of the
chains is 5.4e-15 of that scale at most on these shapes.  gx: rtol 1e-9, atol 1e-10 max|gx|.  logq, logp: rtol 1e-11.  The
summation order is fixed: a second call returns the same bits.

Observed on an MI355X, as a fraction of the bound (pytest -s prints them):
  one layer (ops.flow_layer_bwd), gw / gx                       training sweep (ops.train_grad), gw / logq / logp
  L=32 B=257 (0, 0)  3.3e-04 / 4.0e-06                          small      L=8  B=130 nl=8   4.9e-05 / 1.2e-05 / 4.9e-02
  L=32 B=257 (1, 0)  1.9e-04 / 3.4e-06                          small      L=16 B=512 nl=8   2.7e-04 / 1.2e-05 / 1.9e-02
  L=32 B=257 (0, 1)  3.3e-04 / 3.8e-06                          small      L=12 B=500 nl=9   1.7e-04 / 2.2e-05 / 2.2e-01
  L=32 B=257 (1, 1)  3.8e-04 / 3.2e-06                          two-kernel L=24 B=260 nl=3   2.3e-04 / 2.1e-05 / 2.9e-03
  L=32 B=257 (0, 2)  4.5e-04 / 3.3e-06                          fused      L=32 B=129 nl=2   1.8e-04 / 1.2e-05 / 3.4e-02
  L=32 B=257 (1, 2)  1.9e-04 / 3.6e-06                          fused      L=32 B=193 nl=2   2.2e-04 / 0       / 6.6e-03
  L=32 B=257 (0, 3)  2.7e-04 / 3.9e-06                          L=16 B=512 nl=8, walks of 8 against one item per workgroup (small
  L=32 B=257 (1, 3)  1.8e-04 / 3.4e-06                          path off): gw 4.3e-06; that path against the oracle 2.7e-04
  L=32 B=385 (0, 1)  3.2e-04 / 3.2e-06
  L=20 B=257 (1, 3)  2.4e-04 / 2.5e-06
  L=40 B=114 (0, 2)  1.6e-04 / 3.2e-06
  L=16 B=1030 (0, 3) 2.1e-04 / 3.0e-06
  L=8 B=2050 (1, 0)  1.7e-04 / 3.0e-06
The largest weight-gradient entry of a case lies between 8.5 and 616; the errors are 5e-15 .. 4.5e-14 of that scale.  With
both walks cut one item short (nwalk - 1 where nwalk > 1, a build made once for this purpose) the nineteen oracle cases miss the
bound by factors of 1.3e9 .. 2.7e10.

The stash case found that fthmc_flow_layer_bwd(need_gw) and the two-call route disagreed in the last bit on the exact tiles
(L a power of two >= 16: 14 % of gx, most of gw, at 1e-15 relative) -- not the walk: the call ran the generic instance of the
forward kernel, the two-call route the training-sweep instance, and the two round their stash differently.  csrc/api.hip
layer_bwd_impl now launches the forward as fthmc_flow_layer_fwd_stash does.
"""
import functools
import math

import numpy as np
import pytest
import torch

import walk_model as M
from gpu_support import R, module_defaults, ops, switches

pytestmark = pytest.mark.gpu
_defaults = module_defaults()

GW_BOUND = 1e-10


def field(B, L, gen):
    return (torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi


def gw_metric(got, ref):
    """max|got - ref| / max(1, max|ref|) over the six parameter tensors of every layer: the largest"""
    worst = 0.0
    for row_g, row_r in zip(got, ref):
        assert len(row_g) == len(row_r) == 6
        for g, r in zip(row_g, row_r):
            g = g.detach().cpu()
            assert g.shape == r.shape and bool(torch.isfinite(g).all())
            worst = max(worst, float((g - r).abs().max()) / max(1.0, float(r.abs().max())))
    return worst


def bound_fraction(got, ref, rtol, atol):
    """max |got - ref| / (atol + rtol |ref|) over every element (np.testing.assert_allclose passes where this is <= 1)"""
    got, ref = got.detach().cpu().numpy(), ref.detach().cpu().numpy()
    assert got.shape == ref.shape and np.isfinite(got).all()
    return float((np.abs(got - ref) / (atol + rtol * np.abs(ref))).max())


# ---------------------------------------------------------------- a) one layer: launch_flow_bwd_gather + k_flow_wgrad
@functools.lru_cache(maxsize=2)
def layer_inputs(L, B):
    """one layer's weights, links, upstream link gradient and d/dlogJ; shared by the (mu, off) cases of a shape, never written"""
    gen = torch.Generator().manual_seed(9100 + 7 * L + B)
    wt = R.default_flow(1, gen)[0]
    x = field(B, L, gen)
    c = torch.randn(B, 2, L, L, generator=gen, dtype=torch.float64)
    dlog = torch.randn(B, generator=gen, dtype=torch.float64)
    return wt, x, c, dlog


def assert_layer_walks(L, B):
    stripes, items, tpw, rows, hist = M.LAYER_SHAPES[(L, B)]
    assert M.wgrad_launch(B, L, 1)[:2] == (items, tpw) and M.wgrad_launch(B, L, 1)[3] == rows
    assert M.wgrad_histogram(B, L, 1) == hist and max(hist) == tpw > 1
    assert ops.get_variant() == 1


LAYER_CASES = [(L, B, mu, off) for (L, B), v in M.LAYER_SHAPES.items() for mu, off in v[0]]


@pytest.mark.parametrize('L,B,mu,off', LAYER_CASES)
def test_walked_layer_weight_gradient_vs_oracle(L, B, mu, off):
    """ops.flow_layer_bwd(need_gw=True) at >= 1024 items = autograd of (y c).sum() + (logJ dlog).sum() through the oracle's layer"""
    assert_layer_walks(L, B)
    wt, x, c, dlog = layer_inputs(L, B)
    xr = x.clone().requires_grad_(True)
    wr = [t.clone().requires_grad_(True) for t in wt]
    yc, ljc = R.layer_forward(xr, wr, mu, off)
    ((yc * c).sum() + (ljc * dlog).sum()).backward()
    wl = ops.pack_weights([wt], device='cuda')
    xd, cd, dd = x.cuda(), c.cuda(), dlog.cuda()
    gx, gw = ops.flow_layer_bwd(xd, wl, cd, dd, mu, off, need_gw=True)
    gx2, gw2 = ops.flow_layer_bwd(xd, wl, cd, dd, mu, off, need_gw=True)
    assert torch.equal(gw, gw2) and torch.equal(gx, gx2)
    ew = gw_metric(ops.unpack_weight_grads(gw, 1), [[t.grad for t in wr]])
    gmax = float(xr.grad.abs().max())
    ex = bound_fraction(gx, xr.grad, 1e-9, 1e-10 * gmax)
    print(f'\nwalked layer L={L} B={B} (mu, off)=({mu}, {off}): gw {ew:.2e} = {ew / GW_BOUND:.1e} of the bound '
          f'(largest entry {max(float(t.grad.abs().max()) for t in wr):.3g}); gx {ex:.1e} of the bound')
    assert ew <= GW_BOUND, ew
    assert ex <= 1.0, ex


def test_walked_layer_from_a_callers_stash_is_bit_equal():
    """fthmc_flow_layer_fwd_stash + fthmc_flow_layer_bwd_stash(need_gw): the same forward launch and the same two backward
    kernels on the caller's stash as fthmc_flow_layer_bwd(need_gw) runs on the workspace's -- the same bits (csrc/api.hip
    layer_bwd_impl; tests/test_layer_calls_gpu.py has the ragged L = 24, this is an exact-tile shape at a walk of two)"""
    L, B, mu, off = 32, 257, 1, 2
    assert_layer_walks(L, B)
    wt, x, c, dlog = layer_inputs(L, B)
    wl = ops.pack_weights([wt], device='cuda')
    xd, cd, dd = x.cuda(), c.cuda(), dlog.cuda()
    gx, gw = ops.flow_layer_bwd(xd, wl, cd, dd, mu, off, need_gw=True)
    y, lj, stash = ops.flow_layer_fwd_stash(xd, wl, mu, off)
    assert stash is not None
    gxs, gws = ops.flow_layer_bwd_stash(stash, tuple(x.shape), wl, cd, dd, mu, off, need_gw=True)
    assert torch.equal(gxs, gx) and torch.equal(gws, gw)


# ---------------------------------------------------------------- b) training sweeps: ops.train_grad on the whole batch
def run_train_case(L, B, nl):
    beta, path, tpw, ns, rows, hist = M.TRAIN_SHAPES[(L, B, nl)]
    got, (items, tpw_, ns_, rows_) = M.train_launch(B, L, nl)
    assert (got, tpw_, ns_, rows_) == (path, tpw, ns, rows) and M.histogram(items, tpw, ns) == hist and max(hist) == tpw > 1
    assert ops.get_variant() == 1 and ops.get_small_path()
    gen = torch.Generator().manual_seed(9300 + 11 * L + B + nl)
    flow = R.default_flow(nl, gen)
    xi = field(B, L, gen)
    w = ops.pack_weights(flow, device='cuda')
    xd = xi.cuda()
    r = ops.train_grad(xd, w, nl, beta)
    r2 = ops.train_grad(xd, w, nl, beta)
    assert torch.equal(r['gw'], r2['gw']) and torch.equal(r['logq'], r2['logq']) and torch.equal(r['logp'], r2['logp'])
    out, grads = R.train_grads(xi, flow, beta)
    eq = bound_fraction(r['logq'], out['logq'].detach(), 1e-11, 0.0)
    ep = bound_fraction(r['logp'], out['logp'].detach(), 1e-11, 0.0)
    ew = gw_metric(ops.unpack_weight_grads(r['gw'], nl), grads)
    print(f'\nwalked training sweep ({path}) L={L} B={B} layers={nl}: gw {ew:.2e} = {ew / GW_BOUND:.1e} of the bound '
          f'(largest entry {max(float(g.abs().max()) for lg in grads for g in lg):.3g}); logq {eq:.1e}, logp {ep:.1e} of the bound')
    assert ew <= GW_BOUND, ew
    assert eq <= 1.0 and ep <= 1.0, (eq, ep)
    return r, xd, w, beta, grads


@pytest.mark.parametrize('L,B,nl', [k for k in M.TRAIN_SHAPES if k != (16, 512, 8)])
def test_walked_training_gradient_vs_oracle(L, B, nl):
    """fthmc_train_grad = loss_dkl.backward() of the oracle on the WHOLE batch: the small path's one launch over every layer, the
    two-kernel form inside the sweep, the fused kernel at walks of 2, 3 and 4"""
    run_train_case(L, B, nl)


def test_walked_training_gradient_at_config_2_vs_oracle_and_vs_the_unwalked_path():
    """512 chains of L = 16, 8 layers: walks of 8 on the small path; switched off, the same call goes layer by layer with 512
    items a launch, one per workgroup -- the unwalked twin"""
    L, B, nl = 16, 512, 8
    r, xd, w, beta, grads = run_train_case(L, B, nl)
    assert M.wgrad_histogram(B, L, 1) == {1: B}
    with switches(small=False):
        plain = ops.train_grad(xd, w, nl, beta)
    ref = [[g.cpu() for g in row] for row in ops.unpack_weight_grads(plain['gw'], nl)]
    ew = gw_metric(ops.unpack_weight_grads(r['gw'], nl), ref)
    eo = gw_metric(ref, grads)
    print(f'\nL={L} B={B} layers={nl}: walks of 8 vs one item per workgroup {ew:.2e} = {ew / GW_BOUND:.1e} of the bound; '
          f'one item per workgroup vs oracle {eo / GW_BOUND:.1e} of the bound')
    assert ew <= GW_BOUND and eo <= GW_BOUND, (ew, eo)
