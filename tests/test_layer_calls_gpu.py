"""GPU tests of single layer and kernel entry points: aliased (in-place) layer calls and inverse sweep, the row-strip kernels
against the tile kernels, any s/t net shape against the oracle, the backward from the forward's stash, the final tanh, the
plaquette-level backward, the net shape as an argument of each call, outputs written in place, the device-side run statistics, and
the forward instances that store their stash past the caches."""
import math

import numpy as np
import pytest
import torch

from gpu_support import H, R, angle_close, close, module_defaults, ops, switches

pytestmark = pytest.mark.gpu
_defaults = module_defaults()


# ---------------------------------------------------------------- inverse sweep runs out of place
def test_flow_reverse_in_place_and_out_of_place_agree():
    gen = torch.Generator().manual_seed(12)
    B, L, nl = 5, 48, 8                                   # 9 tiles per chain: halos cross tile borders
    flow = R.default_flow(nl, gen)
    w = ops.pack_weights(flow, device='cuda')
    y = ((torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi).cuda()
    x1, ld1 = ops.flow_reverse(y, w, nl)
    # same call with the output aliasing the input (C ABI allows x == y)
    from fthmc_amd import _lib
    y2 = y.clone(); ld2 = torch.empty_like(ld1)
    wsb = torch.empty(ops.ws_bytes(B, L, nl) // 8 + 1, dtype=torch.float64, device='cuda')
    rc = _lib.load().fthmc_flow_reverse(y2.data_ptr(), w.data_ptr(), None, nl, B, L, 0, 1e-12, y2.data_ptr(), ld2.data_ptr(),
                                        wsb.data_ptr(), wsb.numel() * 8, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(y2, x1) and torch.equal(ld2, ld1)
    yb, _ = ops.flow_forward(x1, w, nl)
    angle_close(yb, y, atol=1e-9)


# ---------------------------------------------------------------- aliased layer calls
@pytest.mark.parametrize('variant', [1, 0])
def test_layer_calls_with_output_aliasing_input(variant):
    """include/fthmc_hip.h: y may alias x in fthmc_flow_layer_fwd / _rev and in fthmc_flow_reverse -- lattices of several
    tiles per chain (halos cross tile borders), both kernel variants, all (mu, off), against the out-of-place call."""
    from fthmc_amd import _lib
    lib = _lib.load()
    with switches(variant=variant):
        gen = torch.Generator().manual_seed(33)
        B, L = 3, 48
        flow = R.default_flow(8, gen)
        w = ops.pack_weights(flow, device='cuda')
        x = ((torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi).cuda()
        wsb = torch.empty(ops.ws_bytes(B, L, 8) // 8 + 1, dtype=torch.float64, device='cuda')
        st = torch.cuda.current_stream().cuda_stream
        for li in range(8):
            mu, off = li % 2, (li // 2) % 4
            wl = w[li * 955:(li + 1) * 955].contiguous()
            y, lj = ops.flow_layer_fwd(x, wl, mu, off)
            xa = x.clone(); lja = torch.empty_like(lj)
            assert lib.fthmc_flow_layer_fwd(xa.data_ptr(), wl.data_ptr(), None, B, L, mu, off, 0, xa.data_ptr(), lja.data_ptr(),
                                            wsb.data_ptr(), wsb.numel() * 8, st) == 0
            torch.cuda.synchronize()
            assert torch.equal(xa, y) and torch.equal(lja, lj), (mu, off)
            xr, ljr = ops.flow_layer_rev(y, wl, mu, off)
            ya = y.clone(); ljb = torch.empty_like(lj)
            assert lib.fthmc_flow_layer_rev(ya.data_ptr(), wl.data_ptr(), None, B, L, mu, off, 0, 1e-12, ya.data_ptr(), ljb.data_ptr(),
                                            wsb.data_ptr(), wsb.numel() * 8, st) == 0
            torch.cuda.synchronize()
            assert torch.equal(ya, xr) and torch.equal(ljb, ljr), (mu, off)
            angle_close(xr, x, atol=1e-9)
        # the sweep (last layer out of place, the rest in place) == explicit out-of-place layer calls
        yfull, _ = ops.flow_forward(x, w, 8)
        xs, lds = ops.flow_reverse(yfull, w, 8)
        cur, tot = yfull, torch.zeros(B, dtype=torch.float64, device='cuda')
        for li in reversed(range(8)):
            cur, lj = ops.flow_layer_rev(cur, w[li * 955:(li + 1) * 955].contiguous(), li % 2, (li // 2) % 4)
            tot = tot + lj
        assert torch.equal(xs, cur)
        close(lds, tot, rtol=1e-13, atol=1e-12)


# ---------------------------------------------------------------- row-strip leapfrog kernel (L % 64 == 0)
@pytest.mark.parametrize('B,L', [(3, 64), (2, 128), (1, 192)])
def test_row_strip_leapfrog_kernel(B, L):
    """k_leap_rows (16-byte accesses, two sites per thread; serves L % 64 == 0) == the 16 x 16-tile kernel bit for bit
    (same arithmetic per site), == the oracle's leapfrog to round-off, and reversible."""
    gen = torch.Generator().manual_seed(64 + L)
    beta, dt, nstep = 3.0, 0.1, 5
    x = ((torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi)
    p = torch.randn(B, 2, L, L, generator=gen, dtype=torch.float64)
    xa, pa = ops.leapfrog(x.cuda(), p.cuda(), beta, dt, nstep)
    with switches(leap_rows=False):
        xb, pb = ops.leapfrog(x.cuda(), p.cuda(), beta, dt, nstep)
    assert torch.equal(xa, xb) and torch.equal(pa, pb)
    xr, pr = R.leapfrog(x, p, lambda y: R.wilson_force_analytic(y, beta), dt, nstep)
    close(xa, xr, rtol=1e-11, atol=1e-11); close(pa, pr, rtol=1e-11, atol=1e-11)
    x2, p2 = ops.leapfrog(xa, -pa, beta, dt, nstep)
    close(x2, x, rtol=1e-10, atol=1e-10); close(-p2, p, rtol=1e-10, atol=1e-10)


# ---------------------------------------------------------------- any s/t net shape (csrc/flow_generic.hip)
@pytest.mark.parametrize('hidden,k,n_mix,L,nl,act', [((8, 8), 3, 3, 8, 4, 'silu'), ((4, 6, 5), 5, 1, 12, 3, 'silu'), ((16,), 3, 2, 16, 2, 'relu'),
                                                     ((), 3, 2, 8, 8, 'silu'), ((8, 8), 1, 2, 8, 2, 'leaky_relu'), ((12, 12), 3, 4, 20, 2, 'silu')])
def test_generic_net_shapes_against_the_oracle(hidden, k, n_mix, L, nl, act):
    """hidden_sizes / kernel_size / n_mixture_comps other than the reference default (fthmc/utils/layers.py:138-167, 399-429
    accept any): every flowed entry point against the oracle -- layer forward / VJP / weight gradient / reverse, the sweeps,
    S_eff, ft_force, an MD trajectory, the training gradient -- and the default shape still takes the tuned kernels."""
    gen = torch.Generator().manual_seed(500 + L + k + n_mix + len(hidden))
    B, beta = 3, 2.5
    flow = R.default_flow(nl, gen, hidden=hidden, n_mix=n_mix, k=k)
    w = ops.pack_weights(flow, device='cuda')
    assert ops.arch_of(w) == (tuple(hidden), k, n_mix) and w.numel() == nl * ops.arch_params(ops.arch_of(w))
    x = (torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi
    xd = x.cuda()
    # one layer: forward, VJP, weight gradient, reverse -- all (mu, off) of the first layers
    for li in range(min(nl, 3)):
        mu, off = li % 2, (li // 2) % 4
        wl = ops.pack_weights([flow[li]], device='cuda')
        y, lj = ops.flow_layer_fwd(xd, wl, mu, off, act)
        xr_ = x.clone().requires_grad_(True)
        wr_ = [t.clone().requires_grad_(True) for t in flow[li]]
        yc, ljc = R.layer_forward(xr_, wr_, mu, off, act)
        angle_close(y, yc.detach(), atol=1e-11); close(lj, ljc.detach(), rtol=1e-11, atol=1e-11)
        c = torch.randn(B, 2, L, L, generator=gen, dtype=torch.float64); dlog = torch.randn(B, generator=gen, dtype=torch.float64)
        ((yc * c).sum() + (ljc * dlog).sum()).backward()
        gx, gw = ops.flow_layer_bwd(xd, wl, c.cuda(), dlog.cuda(), mu, off, act, need_gw=True)
        close(gx, xr_.grad, rtol=1e-9, atol=1e-10 * float(xr_.grad.abs().max()))
        for g_, t_ in zip(ops.unpack_weight_grads(gw, 1)[0], wr_):
            close(g_, t_.grad, rtol=1e-9, atol=1e-10 * max(1.0, float(t_.grad.abs().max())))
        xb_, ljb = ops.flow_layer_rev(y, wl, mu, off, act)
        angle_close(xb_, xd, atol=1e-9); close(ljb, -lj, atol=1e-8)
    # the flow
    y, ld = ops.flow_forward(xd, w, nl, act)
    yc, ldc = R.flow_forward(x, flow, act)
    angle_close(y, yc, atol=1e-10); close(ld, ldc, rtol=1e-10, atol=1e-10)
    xb_, ldb = ops.flow_reverse(y, w, nl, act)
    angle_close(xb_, xd, atol=1e-8); close(ldb, -ld, atol=1e-7)
    S, ld2, plq, Q = ops.ft_action(xd, w, nl, beta, act)
    close(S, R.ft_action(x, flow, beta, act), rtol=1e-11, atol=1e-10); close(plq, R.plaq_mean(yc, beta), rtol=1e-10); close(Q, R.charge(yc), atol=1e-9)
    F = ops.ft_force(xd, w, nl, beta, act)
    Fc = R.ft_force(x, flow, beta, act)
    close(F, Fc, rtol=1e-9, atol=1e-10 * float(Fc.abs().max()))
    assert torch.equal(F, ops.ft_force(xd, w, nl, beta, act))
    v = torch.randn(B, 2, L, L, generator=gen, dtype=torch.float64); u = torch.rand(B, generator=gen, dtype=torch.float64)
    xs = 0.3 * x
    r = ops.ft_trajectory(xs.cuda(), v.cuda(), u.cuda(), w, nl, beta, 0.05, 4, act)
    dH, _, acc, newx, h0, h1 = R.ft_hmc(xs, v, u, flow, beta, 0.05, 4, act=act, mode='md')
    close(r['H0'], h0, rtol=1e-11); close(r['H1'], h1, rtol=1e-9); close(r['dH'], dH, rtol=1e-6, atol=1e-7)
    assert np.array_equal(H(r['acc']) > 0.5, H(acc))
    angle_close(r['x_new'], newx, atol=1e-8)
    outc, gc = R.train_grads(x, flow, beta, act)
    tr = ops.train_grad(xd, w, nl, beta, act)
    close(tr['logq'], outc['logq'], rtol=1e-10); close(tr['logp'], outc['logp'], rtol=1e-10)
    for li, row in enumerate(ops.unpack_weight_grads(tr['gw'], nl)):
        for g_, t_ in zip(row, gc[li]):
            close(g_, t_, rtol=1e-8, atol=1e-10 * max(1.0, float(t_.abs().max())))
    # plaquette-level map
    P = (torch.rand(B, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi
    fP, lj = ops.plaq_coupling_fwd(P.cuda(), ops.pack_weights([flow[0]], device='cuda'), 0, 0, act)
    fPc, ljc = R.plaq_coupling_forward(P, flow[0], 0, 0, act)
    angle_close(fP, fPc, atol=1e-11); close(lj, ljc, rtol=1e-11, atol=1e-11)
    Pb, _ = ops.plaq_coupling_rev(fP, ops.pack_weights([flow[0]], device='cuda'), 0, 0, act)
    angle_close(Pb, P, atol=1e-9)
    # a default-shaped flow right behind it: the shape is an argument of each call, the library remembers nothing
    fd = R.default_flow(2, gen)
    wd = ops.pack_weights(fd, device='cuda')
    xq = (torch.rand(2, 2, 8, 8, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi
    close(ops.ft_force(xq.cuda(), wd, 2, beta), R.ft_force(xq, fd, beta), rtol=1e-10, atol=1e-10)
    # the shape given explicitly to a PLAIN tensor (a clone drops pack_weights' tag) == the tagged call
    wp = w.clone()
    assert ops.arch_of(wp) == ops.DEFAULT_ARCH
    assert torch.equal(ops.ft_force(x.cuda(), wp, nl, beta, act, arch=(hidden, k, n_mix)), ops.ft_force(x.cuda(), w, nl, beta, act))


# ---------------------------------------------------------------- autograd route: the backward reads the forward's stash
@pytest.mark.parametrize('hidden,k,n_mix', [((8, 8), 3, 2), ((6,), 3, 3)])
def test_layer_backward_from_the_forwards_stash(hidden, k, n_mix):
    """fthmc_flow_layer_fwd_stash + fthmc_flow_layer_bwd_stash (what the autograd bridge of GaugeEquivCouplingLayer uses:
    the layer is not run a second time inside its backward) == fthmc_flow_layer_bwd bit for bit; the VALU variant, which
    has no stash, falls back to it."""
    gen = torch.Generator().manual_seed(91)
    B, L = 3, 24
    flow = R.default_flow(4, gen, hidden=hidden, n_mix=n_mix, k=k)
    x = ((torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi).cuda()
    gy = torch.randn(B, 2, L, L, generator=gen, dtype=torch.float64).cuda()
    gl = torch.randn(B, generator=gen, dtype=torch.float64).cuda()
    for li in range(4):
        mu, off = li % 2, (li // 2) % 4
        w = ops.pack_weights([flow[li]], device='cuda')
        y0, lj0 = ops.flow_layer_fwd(x, w, mu, off)
        y, lj, stash = ops.flow_layer_fwd_stash(x, w, mu, off)
        assert stash is not None and torch.equal(y, y0) and torch.equal(lj, lj0)
        for need_gw in (False, True):
            gx0, gw0 = ops.flow_layer_bwd(x, w, gy, gl, mu, off, need_gw=need_gw)
            gx, gw = ops.flow_layer_bwd_stash(stash, x.shape, w, gy, gl, mu, off, need_gw=need_gw)
            assert torch.equal(gx, gx0) and (not need_gw or torch.equal(gw, gw0))
    if tuple(hidden) == (8, 8):
        with switches(variant=0):
            w = ops.pack_weights([flow[0]], device='cuda')
            assert ops.flow_layer_fwd_stash(x, w, 0, 0)[2] is None
    # through autograd: a two-layer composition, gradients wrt x and wrt the weights against the oracle
    from fthmc_amd.utils import layers as Lyr
    nets = Lyr.make_u1_equiv_layers(n_layers=2, n_mixture_comps=n_mix, lattice_shape=(L, L), hidden_sizes=list(hidden),
                                    kernel_size=k, activation_fn='silu')
    names = [f'net.{2 * i}.{n}' for i in range(len(hidden) + 1) for n in ('weight', 'bias')]
    nets.load_state_dict({f'{li}.plaq_coupling.{n}': flow[li][pi].cuda() for li in range(2) for pi, n in enumerate(names)})
    xr = x.clone().requires_grad_(True)
    y1, l1 = nets[0](xr); y2, l2 = nets[1](y1)
    loss = (y2 * gy).sum() + ((l1 + l2) * gl).sum()
    loss.backward()
    xc = x.cpu().clone().requires_grad_(True)
    wc = [[t.clone().requires_grad_(True) for t in flow[li]] for li in range(2)]
    a1, b1 = R.layer_forward(xc, wc[0], 0, 0); a2, b2 = R.layer_forward(a1, wc[1], 1, 0)
    ((a2 * gy.cpu()).sum() + ((b1 + b2) * gl.cpu()).sum()).backward()
    close(xr.grad, xc.grad, rtol=1e-9, atol=1e-10 * float(xc.grad.abs().max()))
    for li in range(2):
        for p, t in zip(nets[li].parameters(), wc[li]):
            close(p.grad, t.grad, rtol=1e-8, atol=1e-10 * max(1.0, float(t.grad.abs().max())))


def test_device_side_run_statistics():
    """RunStats.add_device (one launch of fthmc_stats_accumulate) == RunStats.add (the stacked torch reduction), and qold moves on."""
    from fthmc_amd import parallel as P
    gen = torch.Generator().manual_seed(17)
    B = 37
    a, b = P.RunStats.zeros('cuda'), P.RunStats.zeros('cuda')
    qold = torch.randint(-3, 4, (B,), generator=gen).double().cuda()
    qa = qold.clone()
    for _ in range(3):
        acc = (torch.rand(B, generator=gen) < 0.5).double().cuda()
        plaq = torch.rand(B, generator=gen, dtype=torch.float64).cuda()
        q = torch.randint(-3, 4, (B,), generator=gen).double().cuda()
        dh = torch.randn(B, generator=gen, dtype=torch.float64).cuda()
        a.add(acc, plaq, q, q - qa, dh); qa = q.clone()
        b.add_device(acc, plaq, q, qold, dh)
        assert torch.equal(qold, q)
    close(b.vec, a.vec, rtol=1e-13, atol=1e-12)
    assert float(b.vec[0]) == 3 * B


# ---------------------------------------------------------------- the net shape is an argument of the call
def test_two_net_shapes_on_two_threads_and_streams():
    """Two flows of different s/t net shapes driven from two Python threads on two streams at the same time (ctypes drops
    the GIL inside the C entry points): the shape travels with each call (fthmc_arch_t), the library keeps none, so neither
    thread can see the other's -- every result of every repetition equals the oracle's."""
    import threading
    gen = torch.Generator().manual_seed(77)
    B, L, nl, beta = 4, 16, 3, 2.0
    jobs = []
    for hidden, k, n_mix in (((8, 8), 3, 2), ((4, 6, 5), 5, 1)):
        flow = R.default_flow(nl, gen, hidden=hidden, n_mix=n_mix, k=k)
        x = (torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi
        jobs.append(dict(w=ops.pack_weights(flow, device='cuda'), x=x.cuda(), F=R.ft_force(x, flow, beta),
                         S=R.ft_action(x, flow, beta).detach(), stream=torch.cuda.Stream(), out=[], err=[]))
    torch.cuda.synchronize()
    gate = threading.Barrier(2)

    def run(j):
        try:
            with torch.cuda.stream(j['stream']):
                gate.wait()
                for _ in range(25):
                    j['out'].append((ops.ft_force(j['x'], j['w'], nl, beta), ops.ft_action(j['x'], j['w'], nl, beta)[0]))
                j['stream'].synchronize()
        except Exception as e:                                   # surfaces in the main thread below
            j['err'].append(e)
    threads = [threading.Thread(target=run, args=(j,)) for j in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for j in jobs:
        assert not j['err'], j['err']
        assert len(j['out']) == 25
        for F, S in j['out']:
            close(F, j['F'], rtol=1e-9, atol=1e-10); close(S, j['S'], rtol=1e-11, atol=1e-10)


@pytest.mark.parametrize('hidden,k,n_mix,L,nl', [((8, 8), 3, 2, 8, 3), ((6,), 3, 3, 12, 2)])
def test_final_tanh_option(hidden, k, n_mix, L, nl):
    """make_conv_net(use_final_tanh=True) (layers.py:144,163-164; never built by the reference, :419): the tanh behind the last
    conv through the C ABI (`fthmc_arch_t.final_tanh`, plain kernels) against the oracle -- forward, log det, reverse, force,
    training gradient -- and through the reference-shaped layer with autograd."""
    gen = torch.Generator().manual_seed(300 + L)
    B, beta = 3, 2.0
    flow = R.default_flow(nl, gen, hidden=hidden, n_mix=n_mix, k=k)
    flow = [tuple(t * 2.0 for t in lw) for lw in flow]                       # large enough for the tanh to bend
    w = ops.pack_weights(flow, device='cuda', final_tanh=True)
    assert ops.arch_of(w) == (tuple(hidden), k, n_mix, True)
    x = (torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi
    y, ld = ops.flow_forward(x.cuda(), w, nl)
    yc, ldc = R.flow_forward(x, flow, 'silu+tanh')
    d = (H(y) - H(yc) + np.pi) % (2 * np.pi) - np.pi
    assert np.abs(d).max() < 1e-11
    close(ld, ldc, rtol=1e-11, atol=1e-11)
    y0, _ = ops.flow_forward(x.cuda(), ops.pack_weights(flow, device='cuda'), nl)
    assert float((y - y0).abs().max()) > 1e-3                                # it is a different map
    xb, ldb = ops.flow_reverse(y, w, nl)
    d = (H(xb) - H(x) + np.pi) % (2 * np.pi) - np.pi
    assert np.abs(d).max() < 1e-9 and float((ldb + ld).abs().max()) < 1e-8
    close(ops.ft_force(x.cuda(), w, nl, beta), R.ft_force(x, flow, beta, 'silu+tanh'), rtol=1e-9, atol=1e-10)
    out, grads = R.train_grads(x, flow, beta, 'silu+tanh')
    r = ops.train_grad(x.cuda(), w, nl, beta)
    close(r['logq'], out['logq'], rtol=1e-11); close(r['logp'], out['logp'], rtol=1e-11)
    gws = ops.unpack_weight_grads(r['gw'], nl)
    gmax = max(float(g.abs().max()) for lg in grads for g in lg)
    for li in range(nl):
        for pi in range(len(flow[0])):
            close(gws[li][pi], grads[li][pi], rtol=1e-8, atol=1e-11 * max(gmax, 1.0))
    # the reference-shaped modules: a coupling layer built on a net with the tanh, forward and autograd
    from fthmc_amd.utils import layers as LY
    net = LY.make_conv_net(hidden_sizes=list(hidden), kernel_size=k, in_channels=2, out_channels=n_mix + 1, use_final_tanh=True)
    assert isinstance(net[-1], torch.nn.Tanh) and net.final_tanh
    with torch.no_grad():
        for p_, t_ in zip(LY.net_weights(net), flow[0]):
            p_.copy_(t_.cuda())
    layer = LY.GaugeEquivCouplingLayer(lattice_shape=(L, L), mask_mu=0, mask_off=0,
                                       plaq_coupling=LY.NCPPlaqCouplingLayer(net, mask_shape=(L, L), mask_mu=0, mask_off=0))
    xg = x.cuda().requires_grad_(True)
    yl, lj = layer(xg)
    xr_ = x.clone().requires_grad_(True)
    wr_ = [t.clone().requires_grad_(True) for t in flow[0]]
    ylc, ljc = R.layer_forward(xr_, wr_, 0, 0, 'silu+tanh')
    close(lj, ljc.detach(), rtol=1e-11, atol=1e-11)
    c = torch.randn(B, 2, L, L, generator=gen, dtype=torch.float64)
    ((yl * c.cuda()).sum() + lj.sum()).backward()
    ((ylc * c).sum() + ljc.sum()).backward()
    close(xg.grad, xr_.grad, rtol=1e-9, atol=1e-10 * float(xr_.grad.abs().max()))
    for p_, t_ in zip(LY.net_weights(net), wr_):
        close(p_.grad, t_.grad, rtol=1e-8, atol=1e-10 * max(1.0, float(t_.grad.abs().max())))
    xi_, _ = layer.reverse(yl.detach())
    d = (H(xi_) - H(x) + np.pi) % (2 * np.pi) - np.pi
    assert np.abs(d).max() < 1e-9


@pytest.mark.parametrize('hidden,k,n_mix,L,B', [((8, 8), 3, 2, 8, 3), ((8, 8), 3, 2, 40, 2), ((4, 6), 5, 3, 12, 2)])
def test_plaquette_level_autograd(hidden, k, n_mix, L, B):
    """NCPPlaqCouplingLayer.forward on a plaquette field under autograd (layers.py:348-371): fthmc_plaq_coupling_bwd -- the
    link-level backward kernels with the upstream gradient dressed as a link gradient -- against the oracle's autograd, wrt the
    plaquette field and wrt every conv weight, all (mu, off) classes, tuned and plain kernels, through `ops` and the module."""
    from fthmc_amd.utils import layers as LY
    gen = torch.Generator().manual_seed(77 + L + k)
    flow = R.default_flow(1, gen, hidden=hidden, n_mix=n_mix, k=k)[0]
    w = ops.pack_weights([flow], device='cuda')
    for mu, off in ((0, 0), (1, 2), (0, 3), (1, 1)):
        P = (torch.rand(B, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi
        c = torch.randn(B, L, L, generator=gen, dtype=torch.float64); dl = torch.randn(B, generator=gen, dtype=torch.float64)
        Pr = P.clone().requires_grad_(True)
        wr = [t.clone().requires_grad_(True) for t in flow]
        fPc, ljc = R.plaq_coupling_forward(Pr, wr, mu, off)
        ((fPc * c).sum() + (ljc * dl).sum()).backward()
        gP, gw = ops.plaq_coupling_bwd(P.cuda(), w, c.cuda(), dl.cuda(), mu, off, need_gw=True)
        close(gP, Pr.grad, rtol=1e-9, atol=1e-10 * max(1.0, float(Pr.grad.abs().max())))
        for g_, t_ in zip(ops.unpack_weight_grads(gw, 1)[0], wr):
            close(g_, t_.grad, rtol=1e-8, atol=1e-10 * max(1.0, float(t_.grad.abs().max())))
        assert torch.equal(ops.plaq_coupling_bwd(P.cuda(), w, c.cuda(), dl.cuda(), mu, off)[0], gP)
    # the module: P.requires_grad no longer raises
    net = LY.make_conv_net(hidden_sizes=list(hidden), kernel_size=k, in_channels=2, out_channels=n_mix + 1)
    with torch.no_grad():
        for p_, t_ in zip(LY.net_weights(net), flow):
            p_.copy_(t_.cuda())
    layer = LY.NCPPlaqCouplingLayer(net, mask_shape=(L, L), mask_mu=mu, mask_off=off)
    Pg = P.cuda().requires_grad_(True)
    fP, lj = layer(Pg)
    ((fP * c.cuda()).sum() + (lj * dl.cuda()).sum()).backward()
    close(Pg.grad, Pr.grad, rtol=1e-9, atol=1e-10 * max(1.0, float(Pr.grad.abs().max())))
    for p_, t_ in zip(LY.net_weights(net), wr):
        close(p_.grad, t_.grad, rtol=1e-8, atol=1e-10 * max(1.0, float(t_.grad.abs().max())))
    with torch.no_grad():
        fP2, _ = layer(P.cuda())
    assert torch.equal(fP2, fP.detach())


def test_kernel_wider_than_the_lattice_is_refused():
    """A circular pad wider than the lattice (kernel_size // 2 > L) is refused before any launch, as torch's circular Conv2d
    refuses it (the plain kernels fold an index once)."""
    from fthmc_amd._lib import FthmcError
    gen = torch.Generator().manual_seed(4)
    flow = R.default_flow(1, gen, hidden=(4,), n_mix=2, k=11)
    w = ops.pack_weights(flow, device='cuda')
    x = torch.zeros(2, 2, 4, 4, dtype=torch.float64, device='cuda')
    for call in (lambda: ops.flow_forward(x, w, 1), lambda: ops.ft_force(x, w, 1, 1.0), lambda: ops.flow_layer_fwd(x, w, 0, 0)):
        with pytest.raises(FthmcError, match='unsupported'):
            call()
    ok = ops.pack_weights(R.default_flow(1, gen, hidden=(4,), n_mix=2, k=9), device='cuda')      # 9 // 2 = 4 <= L
    assert torch.isfinite(ops.flow_forward(x, ok, 1)[0]).all()


# ---------------------------------------------------------------- row-strip stencil kernels of the flowed step
@pytest.mark.parametrize('B,L,nl', [(3, 64, 2), (2, 128, 1)])
def test_row_strip_seed_and_kick_kernels(B, L, nl):
    """k_gp_rows / k_kick_rows (16-byte accesses, two sites per thread; serve L % 64 == 0) == k_force<2> / k_kick_from_gp bit
    for bit, through the flowed force and the flowed leapfrog (seed of the backward sweep, kick + drift), and the plain Wilson
    part of the force == the oracle."""
    gen = torch.Generator().manual_seed(640 + L)
    beta, dt, nstep = 5.0, 0.1, 2
    w = ops.pack_weights(R.default_flow(nl, gen), device='cuda')
    x = ((torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi).cuda()
    v = torch.randn(B, 2, L, L, generator=gen, dtype=torch.float64).cuda()

    def run():
        return (ops.ft_force(x, w, nl, beta), *ops.ft_leapfrog(x, v, w, nl, beta, dt, nstep), ops.ft_force(x, None, 0, beta))
    a = run()
    with switches(leap_rows=False):
        b = run()
    for ta, tb in zip(a, b):
        assert torch.equal(ta, tb)
    close(a[3], R.wilson_force_analytic(x.cpu(), beta), rtol=1e-12, atol=1e-12)     # zero layers: seed + stencil adjoint alone


def test_plain_hmc_outputs_in_place():
    """ops.hmc_trajectory / ops.wilson_action_charge write into caller-supplied tensors (`out=`: the bench loop's captured sequence
    carries no copy launches behind them) and return the same numbers as the allocating form; x_new must not alias x."""
    import math
    from fthmc_amd import ops
    from fthmc_amd.ops import FthmcError
    gen = torch.Generator().manual_seed(5)
    B, L = 3, 8
    x = ((torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi).cuda()
    v = torch.randn(B, 2, L, L, generator=gen, dtype=torch.float64).cuda()
    u = torch.rand(B, generator=gen, dtype=torch.float64).cuda()
    ref = ops.hmc_trajectory(x, v, u, 2.0, 0.1, 10)
    out = {'x_new': torch.empty_like(x)}
    for k in ('dH', 'acc', 'H0', 'H1', 'plaq', 'Q'):
        out[k] = torch.full((B,), float('nan'), dtype=torch.float64, device='cuda')
    r = ops.hmc_trajectory(x, v, u, 2.0, 0.1, 10, out=out)
    for k in ('x_new', 'dH', 'acc', 'H0', 'H1'):
        assert r[k].data_ptr() == out[k].data_ptr() and torch.equal(out[k], ref[k]), k
    S, Q, plaq = ops.wilson_action_charge(out['x_new'], 2.0)
    S2, Q2, plaq2 = ops.wilson_action_charge(out['x_new'], 2.0, out=out)
    assert Q2.data_ptr() == out['Q'].data_ptr() and plaq2.data_ptr() == out['plaq'].data_ptr()
    assert torch.equal(S, S2) and torch.equal(Q, out['Q']) and torch.equal(plaq, out['plaq'])
    with pytest.raises(FthmcError):
        ops.hmc_trajectory(x, v, u, 2.0, 0.1, 10, out={'x_new': x})
    with pytest.raises(FthmcError):
        ops.hmc_trajectory(x, v, u, 2.0, 0.1, 10, out={'dH': torch.empty(B + 1, dtype=torch.float64, device='cuda')})


def test_non_temporal_stash_instances_agree_with_the_cached_ones():
    """a layer's stash of 128 MB or more is stored past the caches (csrc/flow_fwd.hip launch_fwd: the SWEEP = 5 / 6 instances of
    the forward) -- the same kernel with another store instruction: a batch big enough to take them gives, chain by chain, what
    the chains give alone (small stash: the cached instances), and the first chain agrees with the oracle"""
    gen = torch.Generator().manual_seed(61)
    L, nl, beta = 256, 2, 3.0
    flow = R.default_flow(nl, gen)
    w = ops.pack_weights(flow, device='cuda')
    # training sweep: 8 chains x 65536 sites x 280 bytes = 147 MB per layer
    B = 8
    xi = ((torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi).cuda()
    r = ops.train_grad(xi, w, nl, beta, groups=1)
    alone = [ops.train_grad(xi[c:c + 1], w, nl, beta, groups=1) for c in range(B)]
    assert torch.equal(r['logq'], torch.cat([a['logq'] for a in alone])) and torch.equal(r['logp'], torch.cat([a['logp'] for a in alone]))
    close(r['gw'], sum(a['gw'] for a in alone) / B, rtol=1e-9, atol=1e-11)
    out, grads = R.train_grads(xi[:1].cpu(), flow, beta)
    close(alone[0]['logq'], out['logq'], rtol=1e-11, atol=0.0)
    gws = ops.unpack_weight_grads(alone[0]['gw'], nl)
    for li in range(nl):
        for pi in range(6):
            scale = float(grads[li][pi].abs().max())
            close(gws[li][pi], grads[li][pi], rtol=1e-8, atol=1e-10 * max(scale, 1.0))
    # force sweep: 16 chains x 65536 sites x 152 bytes = 159 MB per layer
    B = 16
    x = ((torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi).cuda()
    F = ops.ft_force(x, w, nl, beta)
    for c in (0, 7, 15):
        assert torch.equal(F[c:c + 1], ops.ft_force(x[c:c + 1], w, nl, beta))
    # ... and by POSITION in the sweep (csrc/api.hip sweep_forward: FlowLayerArgs::stash_far): a chain group of the headline shape
    # (64 chains of L = 64, 8 layers: 38 MiB of stash per layer) stores the stash of every layer but the last two past the caches
    L, nl, B = 64, 8, 64
    flow = R.default_flow(nl, gen)
    w = ops.pack_weights(flow, device='cuda')
    x = ((torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi).cuda()
    F = ops.ft_force(x, w, nl, 6.0)
    for c in (0, 31, 63):
        assert torch.equal(F[c:c + 1], ops.ft_force(x[c:c + 1], w, nl, 6.0))
    close(F[:1], R.ft_force(x[:1].cpu(), flow, 6.0), rtol=1e-9, atol=1e-9)
