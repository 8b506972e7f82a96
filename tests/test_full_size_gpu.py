"""GPU tests of the BASELINE configs at their own size: the config-5 shard and its full batch, the 1024 chains of configs[3] on one
GPU through size-independent properties, the headline size against the exact plaquette and against the oracle."""
import math

import numpy as np
import pytest
import torch

from gpu_support import H, R, angle_close, close, module_defaults, ops

pytestmark = pytest.mark.gpu
_defaults = module_defaults()


# ---------------------------------------------------------------- BASELINE config 5 shard at its real size
def test_config5_shard_properties_and_oracle():
    """Config 5 per-GPU shard (B=32, L=256, 16 layers, beta=7): size-independent properties at the full shard,
    and the oracle on one of its chains for ft_force and the training gradient."""
    gen = torch.Generator().manual_seed(555)
    B, L, nl, beta = 32, 256, 16, 7.0
    flow = R.default_flow(nl, gen)
    w = ops.pack_weights(flow, device='cuda')
    x = ((torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi).cuda()
    y, ld = ops.flow_forward(x, w, nl)
    Q = ops.wilson_action_charge(y, beta)[1]
    assert float((Q - Q.round()).abs().max()) < 1e-7
    xb, ldb = ops.flow_reverse(y, w, nl, tol=1e-13)
    angle_close(xb, x, atol=1e-8); close(ldb, -ld, atol=1e-5)
    F = ops.ft_force(x, w, nl, beta)
    assert torch.equal(F, ops.ft_force(x, w, nl, beta))          # deterministic
    d = torch.randn(B, 2, L, L, generator=gen, dtype=torch.float64).cuda()
    eps = 1e-5
    fd = (ops.ft_action(x + eps * d, w, nl, beta)[0] - ops.ft_action(x - eps * d, w, nl, beta)[0]) / (2 * eps)
    close((F * d).flatten(1).sum(1), fd, rtol=5e-5, atol=1e-2)
    # a chain's results do not depend on what else is in the batch
    F1 = ops.ft_force(x[5:6].contiguous(), w, nl, beta)
    assert torch.equal(F1[0], F[5])
    # oracle on chain 5: effective action, force, training gradient
    xc = x[5:6].cpu()
    Sg, ldg, pg, qg = ops.ft_action(x[5:6].contiguous(), w, nl, beta)
    yc, ldc = R.flow_forward(xc, flow)
    close(Sg, R.action(yc, beta) - ldc, rtol=1e-10)
    close(ldg, ldc, rtol=1e-9, atol=1e-7); close(pg, R.plaq_mean(yc, beta), rtol=1e-10); close(qg, R.charge(yc), atol=1e-7)
    close(F1, R.ft_force(xc, flow, beta), rtol=1e-7, atol=1e-8)
    outc, gc = R.train_grads(xc, flow, beta)
    r = ops.train_grad(x[5:6].contiguous(), w, nl, beta)
    close(r['logq'], outc['logq'], rtol=1e-10); close(r['logp'], outc['logp'], rtol=1e-10)
    gws = ops.unpack_weight_grads(r['gw'], nl)
    for li in range(nl):
        for pi in range(6):
            scale = float(gc[li][pi].abs().max())
            close(gws[li][pi], gc[li][pi], rtol=1e-7, atol=1e-9 * max(scale, 1.0))
    # a second chain of the shard against the oracle (effective action and force), from the other end of the batch
    xc2 = x[31:32].cpu()
    yc2, ldc2 = R.flow_forward(xc2, flow)
    close(ops.ft_action(x[31:32].contiguous(), w, nl, beta)[0], R.action(yc2, beta) - ldc2, rtol=1e-10)
    close(F[31:32], R.ft_force(xc2, flow, beta), rtol=1e-7, atol=1e-8)
    # full-shard training gradient = mean of per-chain gradients (chains 0..3 checked against their own calls)
    rb = ops.train_grad(x[:4].contiguous(), w, nl, beta)
    acc = sum(ops.train_grad(x[i:i + 1].contiguous(), w, nl, beta)['gw'] for i in range(4)) / 4
    close(rb['gw'], acc, rtol=1e-9, atol=1e-9)


# ---------------------------------------------------------------- BASELINE configs[3]: 1024 chains
def test_config4_1024_chains_on_one_gpu():
    """configs[3] = 1024 chains of L=64, beta=6, 8 layers (128 per GPU on 8 GPUs).  All of them fit one MI355X
    (workspace 6.3 GB): size-independent properties on the full batch, and any chain of the 1024 equals the same
    chain run alone and run inside its 128-chain shard, bit for bit (what sharding over ranks relies on)."""
    gen = torch.Generator().manual_seed(1024)
    B, L, nl, beta, dt, nstep = 1024, 64, 8, 6.0, 0.1, 10
    flow = R.default_flow(nl, gen)
    w = ops.pack_weights(flow, device='cuda')
    x = ((torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi).cuda()
    y, ld = ops.flow_forward(x, w, nl)
    S, Q, plaq = ops.wilson_action_charge(y, beta)
    assert float((Q - Q.round()).abs().max()) < 1e-8                       # integer topological charge
    xb, ldb = ops.flow_reverse(y, w, nl, tol=1e-13)
    angle_close(xb, x, atol=1e-9); close(ldb, -ld, atol=1e-6)             # forward o reverse = id
    F = ops.ft_force(x, w, nl, beta)
    assert torch.equal(F, ops.ft_force(x, w, nl, beta))                    # deterministic
    d = torch.randn(B, 2, L, L, generator=gen, dtype=torch.float64).cuda()
    eps = 1e-5
    fd = (ops.ft_action(x + eps * d, w, nl, beta)[0] - ops.ft_action(x - eps * d, w, nl, beta)[0]) / (2 * eps)
    close((F * d).flatten(1).sum(1), fd, rtol=2e-5, atol=5e-3)             # force = gradient of S_eff
    # gauge invariance of the effective action: x_mu(n) -> x_mu(n) + a(n) - a(n + mu)
    a = (torch.rand(B, L, L, generator=gen, dtype=torch.float64) * 2 * math.pi).cuda()
    xg = torch.stack([x[:, 0] + a - torch.roll(a, -1, 1), x[:, 1] + a - torch.roll(a, -1, 2)], 1).contiguous()
    close(ops.ft_action(xg, w, nl, beta)[0], ops.ft_action(x, w, nl, beta)[0], rtol=1e-10, atol=1e-7)
    # whole trajectories: chain k of the 1024 == chain k alone == chain k inside its 128-chain shard (rank k // 128)
    v = torch.randn(B, 2, L, L, generator=gen, dtype=torch.float64).cuda()
    u = torch.rand(B, generator=gen, dtype=torch.float64).cuda()
    x_cold = (0.2 * x).contiguous()
    r = ops.ft_trajectory(x_cold, v, u, w, nl, beta, dt, nstep, groups=2)
    assert float(r['dH'].abs().max()) < 1e3 and bool(torch.isfinite(r['x_new']).all())
    for k in (0, 517, 1023):
        r1 = ops.ft_trajectory(x_cold[k:k + 1].contiguous(), v[k:k + 1].contiguous(), u[k:k + 1].contiguous(), w, nl, beta, dt, nstep)
        for key in ('x_new', 'dH', 'acc', 'H0', 'H1', 'plaq', 'Q'):
            assert torch.equal(r1[key][0], r[key][k]), (k, key)
    lo = 512
    rs = ops.ft_trajectory(x_cold[lo:lo + 128].contiguous(), v[lo:lo + 128].contiguous(), u[lo:lo + 128].contiguous(),
                           w, nl, beta, dt, nstep, groups=2)
    for key in ('x_new', 'dH', 'acc', 'H0', 'H1', 'plaq', 'Q'):
        assert torch.equal(rs[key], r[key][lo:lo + 128]), key
    # leapfrog reversibility on the full batch
    xo, vo = ops.ft_leapfrog(x_cold, v, w, nl, beta, dt, nstep)
    xr, vr = ops.ft_leapfrog(xo, -vo, w, nl, beta, dt, nstep)
    angle_close(xr, x_cold, atol=1e-8); close(-vr, v, rtol=1e-8, atol=1e-8)
    ops.release_workspaces()


# ---------------------------------------------------------------- BASELINE configs[4]: the FULL batch on one GPU
def test_config5_full_batch_on_one_gpu():
    """configs[4] = 256 chains of L=256, beta=7, 16 layers (32 per GPU on 8 GPUs).  All 256 fit one MI355X (force workspace
    ~50 GB, training ~90 GB of the 288): size-independent properties on the full batch -- integer Q, forward o reverse = id,
    force = finite-difference gradient of S_eff, training gradient = finite-difference derivative of the loss -- and chains
    0 / 131 / 255 bit-equal to the same chain inside its 32-chain shard.  Workspaces are released afterwards."""
    gen = torch.Generator().manual_seed(256)
    B, L, nl, beta = 256, 256, 16, 7.0
    flow = R.default_flow(nl, gen)
    w = ops.pack_weights(flow, device='cuda')
    try:
        x = ops.random_uniform(torch.arange(B, dtype=torch.int64, device='cuda') + 77, (B, 2, L, L), -math.pi, math.pi)
        y, ld = ops.flow_forward(x, w, nl)
        Q = ops.wilson_action_charge(y, beta)[1]
        assert float((Q - Q.round()).abs().max()) < 1e-6
        xb, ldb = ops.flow_reverse(y, w, nl, tol=1e-13)
        d = (xb - x + math.pi) % (2 * math.pi) - math.pi
        assert float(d.abs().max()) < 1e-8 and float((ldb + ld).abs().max()) < 1e-5
        del xb, ldb, d
        F = ops.ft_force(x, w, nl, beta)
        dirn = ops.random_momenta(torch.arange(B, dtype=torch.int64, device='cuda') + 5, (B, 2, L, L), need_u=False)[0]
        eps = 1e-5
        fd = (ops.ft_action(x + eps * dirn, w, nl, beta)[0] - ops.ft_action(x - eps * dirn, w, nl, beta)[0]) / (2 * eps)
        close((F * dirn).flatten(1).sum(1), fd, rtol=5e-5, atol=2e-3)
        # shards: chains 0, 131, 255 inside their 32-chain blocks
        for c in (0, 131, 255):
            lo = c // 32 * 32
            Fs = ops.ft_force(x[lo:lo + 32].contiguous(), w, nl, beta)
            assert torch.equal(Fs[c - lo], F[c])
            ys = ops.flow_forward(x[lo:lo + 32].contiguous(), w, nl)[0]
            assert torch.equal(ys[c - lo], y[c])
        del F, dirn, fd, y
        # training gradient on the full batch: directional finite difference of the loss in weight space
        r = ops.train_grad(x, w, nl, beta, groups=1)
        loss = lambda ww: float((lambda t: (t['logq'] - t['logp']).mean())(ops.train_grad(x, ww, nl, beta, need_gw=False)))
        dw = torch.randn(w.numel(), generator=gen, dtype=torch.float64).cuda()
        dw = dw / dw.norm()
        epsw = 1e-6
        fdw = (loss(w + epsw * dw) - loss(w - epsw * dw)) / (2 * epsw)
        an = float((r['gw'] * dw).sum())
        assert abs(an - fdw) < 1e-4 * max(1.0, abs(an)), (an, fdw)
        rs = ops.train_grad(x[128:160].contiguous(), w, nl, beta, groups=1, need_gw=False)
        assert torch.equal(rs['logq'][3], r['logq'][131]) and torch.equal(rs['logp'][3], r['logp'][131])
    finally:
        ops.release_workspaces()
        torch.cuda.empty_cache()


def test_headline_size_sampler_reproduces_the_exact_plaquette():
    """L = 64 (the tiled MFMA kernels, two chain groups), beta = 6: plain HMC and ftHMC with an untrained 2-layer flow from the
    near-cold start; <cos P> of the (flowed) field against I1/I0 and <exp(-dH)> against 1, errors over independent chains
    (tools/operating_point.py is the long version: profiles/r04_headline_size_plaquette.json).  Seeds are fixed: deterministic."""
    import math
    from fthmc_amd import ops, parallel, train as T
    from fthmc_amd.config import PLAQ_EXACT, TrainConfig
    from fthmc_amd.utils.layers import net_weights
    L, beta, B, nl, therm, ntraj, nstep = 64, 6.0, 128, 2, 250, 250, 20
    dev = torch.device('cuda', 0)
    torch.manual_seed(3)
    model = T.get_model(TrainConfig(L=L, beta=beta, n_layers=nl, batch_size=B, print_freq=0))
    w = ops.pack_weights([net_weights(l.plaq_coupling.net) for l in model.layers], device=dev)
    for flowed in (False, True):
        g0, _ = ops.random_momenta(parallel.chain_seeds(77, 0, B, 0).to(dev), (B, 2, L, L), need_u=False)
        x = (0.1 * torch.erf(g0 / math.sqrt(2.0))).contiguous()
        plaq_s = torch.zeros(B, dtype=torch.float64, device=dev); emdh_s = torch.zeros_like(plaq_s); acc_s = torch.zeros_like(plaq_s)
        for it in range(therm + ntraj):
            v, u = ops.random_momenta(parallel.chain_seeds(78, 0, B, it).to(dev), (B, 2, L, L))
            if flowed:
                r = ops.ft_trajectory(x, v, u, w, nl, beta, 1.0 / nstep, nstep, mode='md', groups=2)
                plaq = r['plaq']
            else:
                r = ops.hmc_trajectory(x, v, u, beta, 1.0 / nstep, nstep)
                plaq = ops.wilson_action_charge(r['x_new'], beta)[2]
            x = r['x_new']
            if it >= therm:
                plaq_s += plaq; emdh_s += torch.exp(-r['dH']); acc_s += r['acc']
        p = (plaq_s / ntraj).cpu().numpy(); e = (emdh_s / ntraj).cpu().numpy()
        perr, eerr = p.std(ddof=1) / math.sqrt(B), e.std(ddof=1) / math.sqrt(B)
        assert float(acc_s.mean()) / ntraj > 0.6
        assert perr < 5e-5 and abs(p.mean() - PLAQ_EXACT[beta]) < 4 * perr, (flowed, p.mean(), perr)
        assert abs(e.mean() - 1.0) < 4 * eerr, (flowed, e.mean(), eerr)


# ---------------------------------------------------------------- more of the headline size against the oracle
def test_headline_size_two_chain_groups_against_the_oracle():
    """BASELINE configs[2] at its own lattice size and depth (L = 64, beta = 6, 8 layers), 24 chains = two chain groups on two
    streams: S_eff, log det J, plaquette, Q, the force and ONE WHOLE 10-step trajectory (H0, H1, dH, accepts, end field) against
    the oracle on all 24 chains (the round-4 suite compared 3 chains at this size; bench.py compares 128 in every run)."""
    B, L, nl, beta, dt, nstep = 24, 64, 8, 6.0, 0.1, 10
    gen = torch.Generator().manual_seed(4242)
    flow = R.default_flow(nl, gen)
    w = ops.pack_weights(flow, device='cuda')
    x = 0.35 * (torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1)        # near-cold, as the bench's chains
    v = torch.randn(B, 2, L, L, generator=gen, dtype=torch.float64)
    u = torch.rand(B, generator=gen, dtype=torch.float64)
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    y, ld = R.flow_forward(x, flow)
    Sg, ldg, pg, qg = ops.ft_action(x.cuda(), w, nl, beta)
    np.testing.assert_allclose(H(ldg), H(ld), rtol=1e-11, atol=1e-10)
    np.testing.assert_allclose(H(Sg), H(R.ft_action(x, flow, beta)), rtol=1e-12)
    np.testing.assert_allclose(H(pg), H(R.plaq_mean(y, beta)), rtol=1e-12)
    np.testing.assert_allclose(H(qg), H(R.charge(y)), atol=1e-8)
    F = R.ft_force(x, flow, beta)
    np.testing.assert_allclose(H(ops.ft_force(x.cuda(), w, nl, beta)), H(F), rtol=1e-8, atol=1e-9 * float(F.abs().max()))
    dH, _, acc, newx, h0, h1 = R.ft_hmc(x, v, u, flow, beta, dt, nstep, mode='md')
    r = ops.ft_trajectory(x.cuda(), v.cuda(), u.cuda(), w, nl, beta, dt, nstep, mode='md', groups=2)
    np.testing.assert_allclose(H(r['H0']), H(h0), rtol=1e-12)
    np.testing.assert_allclose(H(r['H1']), H(h1), rtol=1e-9)                     # ten MD steps amplify rounding
    np.testing.assert_allclose(H(r['dH']), H(dH), rtol=0, atol=1e-6 * float(h1.abs().max()))
    border = (u - torch.exp(-dH)).abs() < 1e-9
    assert bool((((r['acc'].cpu() > 0.5) == acc) | border).all())
    d = (r['x_new'].cpu() - newx + math.pi) % (2 * math.pi) - math.pi
    assert float(d.abs().max()) < 1e-6
