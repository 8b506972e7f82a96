"""In-place forward layers (flow_fwd.hip INPL; api.hip sweep_forward): on the exact tiles a sweep maps the caller's field into one
work buffer with layer 0 and updates that buffer in place with layers 1 .. nl - 1, each loading and storing only the 64 links per
tile it changes.

(a) one layer with y == x against the same layer with a separate y, all eight (mu, off), at L = 16 (B = 2: one tile that wraps
    onto itself, every active link next to the tile's own edge) and L = 32 (B = 3: 2 x 2 tiles whose origins are shifted across
    the lattice edge for every off): link field, log J and stash bit-equal.  Both entry points: flow_layer_fwd (the action-sweep
    instance) and flow_layer_fwd_stash (the training-sweep instance).  The in-place buffer is a copy of x, so a link the layer
    does not own must come out as it went in: compared against x itself, not only against the other run.
(b) 8-layer sweeps at L = 32, B = 3: ft_action and ft_force against oracle/ref_cpu.py at the tolerances of
    test_hip_parity.py::test_ft_vs_oracle_random; a second call on another field through the same workspace (whose work buffer
    then holds the first field's result: a link left stale would show) bit-equal to that field's first answer; ft_trajectory with
    carried state against the stateless one (test_hip_parity.py: torch.equal); the caller's x unchanged by ft_force, the
    leapfrog's input x and v unchanged by ft_leapfrog, both compared with clones.
(c) ragged L = 20 (non-EXACT instances, tile origin 0, checkpoint chain): against the oracle, same tolerances.
(d) steep weights (tests/golden/steep_inverse.npz, s0 = 2, 5, 10, 20): the forward map of the link-level cases, out of place and
    in place, within the bounds test_steep_inverse_gpu.py derives (8 delta_ref + 4 ulp(pi) per link, 1e-12 sum |local log J|).
(e) train_grad at L = 32, 8 layers (the training-sweep instances in place) against the oracle's autograd at the tolerances of
    test_hip_parity.py::test_train_grad_golden (train_L8 / train_L16).
"""
import math

import numpy as np
import pytest
import torch

import steep_fixture as SF
from steep_fixture import ULP_PI

from gpu_support import H, R, close, module_defaults, ops

pytestmark = pytest.mark.gpu
_defaults = module_defaults(small=False)          # L = 16 on the tiled kernels

LAYERS = [(mu, off) for off in range(4) for mu in range(2)]


def draw(B, L, seed, nl=8):
    gen = torch.Generator().manual_seed(seed)
    flow = R.default_flow(nl, gen)
    x = (torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi
    return flow, x


_sweep = {}


def sweep_case(L, B=3, beta=4.0):
    """field, weights and the oracle's answers of the sweep tests, computed once"""
    if L not in _sweep:
        flow, x = draw(B, L, 8800 + L)
        _sweep[L] = dict(flow=flow, x=x, beta=beta, w=ops.pack_weights(flow, device='cuda'),
                         Se=R.ft_action(x, flow, beta), F=R.ft_force(x, flow, beta))
    return _sweep[L]


# ---------------------------------------------------------------- (a)
@pytest.mark.parametrize('L,B', [(16, 2), (32, 3)])
def test_layer_in_place_bit_equal(L, B):
    flow, x = draw(B, L, 7700 + L)
    xg = x.cuda()
    for li, (mu, off) in enumerate(LAYERS):
        wl = ops.pack_weights([flow[li]], device='cuda')
        act = torch.from_numpy(SF.active_mask(L, mu, off)).cuda()
        same = torch.ones_like(xg, dtype=torch.bool)
        same[:, mu] = ~act
        # action-sweep instance
        y, lj = ops.flow_layer_fwd(xg, wl, mu, off)
        buf = xg.clone()
        yi, lji = ops.flow_layer_fwd(buf, wl, mu, off, inplace=True)
        assert yi.data_ptr() == buf.data_ptr()
        assert torch.equal(yi, y) and torch.equal(lji, lj), (mu, off, float((yi - y).abs().max()))
        assert torch.equal(yi[same], xg[same]), (mu, off)
        assert not torch.equal(yi[:, mu][:, act], xg[:, mu][:, act])          # ... and the active links did move
        # training-sweep instance (stash with h1, h2)
        # (the stash has entries no kernel writes -- dead stripe lines, reserved planes: both runs start from the same fill)
        from fthmc_amd import _lib
        nst = int(_lib.load().fthmc_layer_stash_bytes(None, B, L)) // 8
        ys, ljs, st = ops.flow_layer_fwd_stash(xg, wl, mu, off, stash=torch.full((nst,), 1234.5, dtype=torch.float64, device='cuda'))
        buf = xg.clone()
        ysi, ljsi, sti = ops.flow_layer_fwd_stash(buf, wl, mu, off, inplace=True,
                                                  stash=torch.full((nst,), 1234.5, dtype=torch.float64, device='cuda'))
        assert ysi.data_ptr() == buf.data_ptr()
        assert torch.equal(ysi, ys) and torch.equal(ljsi, ljs), (mu, off)
        assert torch.equal(sti, st) and float((st != 1234.5).double().mean()) > 0.4, (mu, off)
        assert torch.equal(ysi[same], xg[same]), (mu, off)
        # a second layer on top of the first, in place twice against out of place twice
        mu2, off2 = LAYERS[(li + 3) % 8]
        w2 = ops.pack_weights([flow[(li + 3) % 8]], device='cuda')
        y2, lj2 = ops.flow_layer_fwd(y, w2, mu2, off2)
        y2i, lj2i = ops.flow_layer_fwd(yi, w2, mu2, off2, inplace=True)
        assert torch.equal(y2i, y2) and torch.equal(lj2i, lj2), (mu, off, mu2, off2)


# ---------------------------------------------------------------- (b)
def test_sweeps_vs_oracle_L32():
    c = sweep_case(32)
    xg = c['x'].cuda()
    keep = xg.clone()
    Seg = ops.ft_action(xg, c['w'], 8, c['beta'])[0]
    Fg = ops.ft_force(xg, c['w'], 8, c['beta'])
    print(f"L=32: action rel {float(((Seg.cpu() - c['Se']) / c['Se']).abs().max()):.2e} force abs {float((Fg.cpu() - c['F']).abs().max()):.2e}")
    close(Seg, c['Se'], rtol=1e-11)
    close(Fg, c['F'], rtol=1e-8, atol=1e-9)
    assert torch.equal(xg, keep)                                               # the caller's field
    # the same workspace again on another field, then on the first: the work buffer holds the other field's result each time
    _, x2 = draw(3, 32, 9911)
    x2g = x2.cuda()
    S2 = ops.ft_action(x2g, c['w'], 8, c['beta'])
    F2 = ops.ft_force(x2g, c['w'], 8, c['beta'])
    assert float((S2[0] - Seg).abs().min()) > 1e-3                             # another field indeed
    Sb = ops.ft_action(xg, c['w'], 8, c['beta'])[0]
    Fb = ops.ft_force(xg, c['w'], 8, c['beta'])
    assert torch.equal(Sb, Seg) and torch.equal(Fb, Fg)
    S2b = ops.ft_action(x2g, c['w'], 8, c['beta'])
    assert all(torch.equal(a, b) for a, b in zip(S2b, S2)) and torch.equal(ops.ft_force(x2g, c['w'], 8, c['beta']), F2)
    # flow_forward hands the flowed field out: against the oracle, and the layers one by one out of place
    y, ld = R.flow_forward(c['x'], c['flow'])
    yg, ldg = ops.flow_forward(xg, c['w'], 8)
    close(yg, y, atol=1e-11); close(ldg, ld, rtol=1e-11, atol=1e-11)
    z, lsum = xg, torch.zeros(3, dtype=torch.float64, device='cuda')
    for li, (mu, off) in enumerate(LAYERS):
        z, lj = ops.flow_layer_fwd(z, ops.pack_weights([c['flow'][li]], device='cuda'), mu, off)
        lsum = lsum + lj
    assert torch.equal(yg, z)
    close(ldg, lsum, rtol=1e-13, atol=1e-13)                                   # same terms, another order of the sum
    assert torch.equal(xg, keep)


def test_trajectory_state_and_inputs_L32():
    c = sweep_case(32)
    gen = torch.Generator().manual_seed(4242)
    B, L, dt, nstep = 3, 32, 0.05, 3
    xa, xb, state = c['x'].cuda(), c['x'].cuda(), None
    for t in range(2):
        v = torch.randn(B, 2, L, L, generator=gen, dtype=torch.float64).cuda()
        u = torch.rand(B, generator=gen, dtype=torch.float64).cuda()
        keep_x, keep_v = xa.clone(), v.clone()
        ra = ops.ft_trajectory(xa, v, u, c['w'], 8, c['beta'], dt, nstep)
        rb = ops.ft_trajectory(xb, v, u, c['w'], 8, c['beta'], dt, nstep, state_in=state)
        for k in ('x_new', 'dH', 'acc', 'H0', 'H1', 'plaq', 'Q', 'state'):
            assert torch.equal(ra[k], rb[k]), k
        assert torch.equal(xa, keep_x) and torch.equal(v, keep_v)
        Se = ops.ft_action(ra['x_new'], c['w'], 8, c['beta'])[0]
        close(ra['state'][0], Se, rtol=1e-13)
        xa, xb, state = ra['x_new'].clone(), rb['x_new'].clone(), rb['state'].clone()
    # the leapfrog state: ft_leapfrog's x, v in; its result against the kicks v' = v - dt F and drifts written out with ft_force
    v = torch.randn(B, 2, L, L, generator=gen, dtype=torch.float64).cuda()
    x0 = c['x'].cuda()
    keep_x, keep_v = x0.clone(), v.clone()
    xo, vo = ops.ft_leapfrog(x0, v, c['w'], 8, c['beta'], dt, 2)
    assert torch.equal(x0, keep_x) and torch.equal(v, keep_v)
    xs = x0 + 0.5 * dt * v
    vs = v - dt * ops.ft_force(xs, c['w'], 8, c['beta'])
    xs = xs + dt * vs
    vs = vs - dt * ops.ft_force(xs, c['w'], 8, c['beta'])
    xs = xs + 0.5 * dt * vs
    close(xo, xs, rtol=0, atol=1e-12); close(vo, vs, rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------- (c)
def test_ragged_L20_unchanged():
    flow, x = draw(2, 20, 8820)
    w = ops.pack_weights(flow, device='cuda')
    beta = 3.0
    xg = x.cuda()
    keep = xg.clone()
    y, ld = R.flow_forward(x, flow)
    yg, ldg = ops.flow_forward(xg, w, 8)
    close(yg, y, atol=1e-11); close(ldg, ld, rtol=1e-11, atol=1e-11)
    close(ops.ft_action(xg, w, 8, beta)[0], R.ft_action(x, flow, beta), rtol=1e-11)
    close(ops.ft_force(xg, w, 8, beta), R.ft_force(x, flow, beta), rtol=1e-8, atol=1e-9)
    assert torch.equal(xg, keep)
    # y == x on a ragged lattice: the full copy onto itself
    for li, (mu, off) in enumerate(LAYERS[:4]):
        wl = ops.pack_weights([flow[li]], device='cuda')
        y1, lj1 = ops.flow_layer_fwd(xg, wl, mu, off)
        yi, lji = ops.flow_layer_fwd(xg.clone(), wl, mu, off, inplace=True)
        assert torch.equal(yi, y1) and torch.equal(lji, lj1)


# ---------------------------------------------------------------- (d)
def test_steep_forward_bounds():
    g = SF.load()
    worst = {}
    for ci in range(len(g['case_s0'])):
        _, L, mu, off = (int(v) for v in g[f'link{ci}_meta'])
        delta = g['delta_ref'][SF.si_of(g, ci)]
        w = ops.pack_weights([tuple(torch.from_numpy(np.asarray(a)) for a in SF.case_weights(g, ci))], device='cuda')
        act = SF.active_mask(L, mu, off)
        x = g[f'link{ci}_x']
        xg = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()
        same = np.ones(x.shape, bool)
        same[:, mu][:, act] = False
        for inplace in (False, True):
            yg, ljg = ops.flow_layer_fwd(xg.clone(), w, mu, off, inplace=inplace)
            yg, ljg = H(yg), H(ljg)
            ey = np.abs(SF.wrapdiff(yg[:, mu][:, act], g[f'link{ci}_yl'])) / (8 * delta + 4 * ULP_PI)
            el = np.abs(ljg - g[f'link{ci}_logJ']) / (1e-12 * g[f'link{ci}_labs'])
            key = (float(g['case_s0'][ci]), inplace)
            worst[key] = max(worst.get(key, 0.0), float(ey.max()), float(el.max()))
            assert np.all(np.isfinite(yg)) and ey.max() <= 1.0 and el.max() <= 1.0, (ci, L, mu, off, inplace, ey.max(), el.max())
            assert np.array_equal(yg[same], x[same]), (ci, inplace)
    print('steep forward, error / bound by (s0, in place): ' + ', '.join(f'{k} {v:.3f}' for k, v in sorted(worst.items())))
    assert {k[0] for k in worst} == set(SF.S0)


# ---------------------------------------------------------------- (e)
def test_train_grad_L32():
    c = sweep_case(32)
    out, grads = R.train_grads(c['x'], c['flow'], c['beta'])
    xg = c['x'].cuda()
    keep = xg.clone()
    r = ops.train_grad(xg, c['w'], 8, c['beta'])
    gws = ops.unpack_weight_grads(r['gw'], 8)
    err = max(float((gws[li][pi].cpu() - grads[li][pi]).abs().max()) for li in range(8) for pi in range(6))
    print(f'train_grad L=32: max abs gradient error {err:.2e}')
    close(r['logq'], out['logq'], rtol=1e-11); close(r['logp'], out['logp'], rtol=1e-11)
    d = (H(r['x']) - H(out['x']) + np.pi) % (2 * np.pi) - np.pi
    assert float(np.abs(d).max()) < 1e-10
    for li in range(8):
        for pi in range(6):
            close(gws[li][pi], grads[li][pi], rtol=1e-8, atol=1e-12)
    assert torch.equal(xg, keep)
