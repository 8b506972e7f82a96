"""Aligned tile origins of the coupling-layer forward (flow_fwd.hip, the EXACT instances: L a power of two, tiles divide
the lattice): across the stripe lines tile t starts at (16 t + off + 3) mod L, so a tile can straddle the lattice edge and
every global line of an own site is wrapped.

(a) each of the 8 (mu, off) layers at L = 16, 32, 64, 128, forward and reverse, against oracle/ref_cpu.py at the
    tolerances test_hip_parity.py::test_layers_golden uses for the same quantities;
(b) ft_force, ft_action, train_grad at L = 32 and 64, 8 layers, against the oracle's autograd at the tolerances of
    test_ft_vs_oracle_random / test_train_grad_vs_oracle_random;
(c) translation: the field rolled by 4, 8, 12 and L/2 - 4 lines across and along gives the rolled outputs at the tolerances
    of (a) -- this finds a missed wrap at the lattice edge -- and rolled by 16, a whole tile, bit for bit: y is compared with
    torch.equal.  log J is a sum of per-tile partial sums taken in tile order, and a roll by a tile permutes the tiles: its
    terms are bit-identical, the order of the additions is not, so log J is held to the tolerance of (a) there;
(d) the same layers and sweeps at L = 16 (one tile that wraps onto itself) with the small-lattice path switched off.
"""
import math

import numpy as np
import pytest
import torch

from gpu_support import H, R, close, module_defaults, ops, switches

pytestmark = pytest.mark.gpu
_defaults = module_defaults()

LAYERS = [(mu, off) for off in range(4) for mu in range(2)]


@pytest.fixture
def tiled():
    """small-lattice path off: L = 16 takes the tiled kernels"""
    with switches(small=False):
        yield


def angle_err(a, b):
    d = (H(a) - H(b) + np.pi) % (2 * np.pi) - np.pi
    return float(np.max(np.abs(d)))


def field(B, L, seed):
    gen = torch.Generator().manual_seed(seed)
    flow = R.default_flow(8, gen)
    x = (torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi
    return flow, x


def check_layers(L, B=2):
    flow, x = field(B, L, 4100 + L)
    for li, (mu, off) in enumerate(LAYERS):
        w = flow[li]
        wl = ops.pack_weights([w], device='cuda')
        y, lj = R.layer_forward(x, w, mu, off)
        yg, ljg = ops.flow_layer_fwd(x.cuda(), wl, mu, off, 'silu')
        print(f'L={L} mu={mu} off={off}: fwd |dy| {float((yg.cpu() - y).abs().max()):.2e} |dlogJ| {float((ljg.cpu() - lj).abs().max()):.2e}')
        close(yg, y, atol=1e-12); close(ljg, lj, atol=1e-12)
        xr, ljr = ops.flow_layer_rev(y.cuda(), wl, mu, off, 'silu', tol=1e-13)
        e = angle_err(xr, x)
        print(f'                     rev |dx| {e:.2e} |dlogJ| {float((ljr.cpu() + lj).abs().max()):.2e}')
        assert e < 1e-9, e                                   # exact inverse, not the reference's 1e-6 bisection
        close(ljr, -lj, atol=1e-8)
        xo, ljo = R.layer_reverse(y, w, mu, off)             # the oracle's own reverse (bisection to 1e-6)
        assert angle_err(xr, xo) < 5e-6
        close(ljr, ljo, atol=5e-5)


def check_sweeps(L, B=3, beta=4.0):
    flow, x = field(B, L, 5200 + L)
    w = ops.pack_weights(flow, device='cuda')
    Se = R.ft_action(x, flow, beta)
    Seg = ops.ft_action(x.cuda(), w, 8, beta)[0]
    close(Seg, Se, rtol=1e-11)
    F = R.ft_force(x, flow, beta)
    Fg = ops.ft_force(x.cuda(), w, 8, beta)
    print(f'L={L}: action rel {float(((Seg.cpu() - Se) / Se).abs().max()):.2e} force abs {float((Fg.cpu() - F).abs().max()):.2e}')
    close(Fg, F, rtol=1e-8, atol=1e-9)
    out, grads = R.train_grads(x, flow, beta)
    r = ops.train_grad(x.cuda(), w, 8, beta)
    close(r['logq'], out['logq'], rtol=1e-11); close(r['logp'], out['logp'], rtol=1e-11)
    assert angle_err(r['x'], out['x']) < 1e-10
    gws = ops.unpack_weight_grads(r['gw'], 8)
    for li in range(8):
        for pi in range(6):
            close(gws[li][pi], grads[li][pi], rtol=1e-8, atol=1e-11)


# ---------------------------------------------------------------- (a)
@pytest.mark.parametrize('L', [16, 32, 64, 128])
def test_layers_vs_oracle(L):
    check_layers(L)


# ---------------------------------------------------------------- (b)
@pytest.mark.parametrize('L', [32, 64])
def test_sweeps_vs_oracle(L):
    check_sweeps(L)


# ---------------------------------------------------------------- (c)
@pytest.mark.parametrize('L', [32, 64])
def test_translation(L):
    flow, x = field(2, L, 6300 + L)
    xg = x.cuda()
    for li, (mu, off) in enumerate(LAYERS):
        wl = ops.pack_weights([flow[li]], device='cuda')
        y, lj = ops.flow_layer_fwd(xg, wl, mu, off, 'silu')
        for dim in (2, 3):                                   # rows / columns: across or along the stripe lines, by mu
            for s in (4, 8, 12, L // 2 - 4, 16):
                ys, ljs = ops.flow_layer_fwd(torch.roll(xg, s, dims=dim).contiguous(), wl, mu, off, 'silu')
                yr = torch.roll(y, s, dims=dim)
                if s == 16:
                    assert torch.equal(ys, yr), (mu, off, dim, s, float((ys - yr).abs().max()))
                else:
                    close(ys, yr, atol=1e-12)
                close(ljs, lj, atol=1e-12)
                xr, ljr = ops.flow_layer_rev(yr.contiguous(), wl, mu, off, 'silu', tol=1e-13)
                e = angle_err(xr, torch.roll(xg, s, dims=dim))
                assert e < 1e-9, (mu, off, dim, s, e)
                close(ljr, -lj, atol=1e-8)


# ---------------------------------------------------------------- (d)
def test_L16_tiled_layers(tiled):
    check_layers(16)


def test_L16_tiled_sweeps(tiled):
    check_sweeps(16)
