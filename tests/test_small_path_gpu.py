"""GPU tests of the small-lattice fused path (csrc/flow_small.hip: L = 8, 12, 16 as one launch per trajectory / force / action)
against the tiled path, the oracle and in a captured graph, and of the wave-split action sums of few chains on a large lattice."""
import math

import numpy as np
import pytest
import torch

from gpu_support import H, R, angle_close, capture, close, module_defaults, ops, switches

pytestmark = pytest.mark.gpu
_defaults = module_defaults()


# ---------------------------------------------------------------- small-lattice fused path (csrc/flow_small.hip)
def _both_paths(fn):
    with switches(small=True):
        a = fn()
    with switches(small=False):
        b = fn()
    return a, b


@pytest.mark.parametrize('L,nl,B,beta,act', [(16, 4, 32, 4.0, 'silu'), (8, 2, 3, 2.0, 'silu'), (12, 8, 5, 3.0, 'silu'),
                                             (16, 16, 2, 4.0, 'relu'), (8, 8, 1, 2.0, 'leaky_relu'), (12, 1, 7, 4.0, 'silu')])
def test_small_lattice_path_equals_tiled_path(L, nl, B, beta, act):
    """L = 8, 12, 16 run by default as ONE launch per trajectory / force / action (one workgroup per chain, periodic planes
    in LDS).  Same results as the tiled kernels (one launch per layer) on the same inputs: every entry point that takes
    the path, to fp64 round-off (1e-11; trajectories 1e-9 after 6 MD steps)."""
    import bench
    gen = torch.Generator().manual_seed(100 + L + nl)
    flow = bench.make_flow(gen, nl)
    w = ops.pack_weights(flow, device='cuda')
    x = ((torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi).cuda()
    v = torch.randn(B, 2, L, L, generator=gen, dtype=torch.float64).cuda()
    u = torch.rand(B, generator=gen, dtype=torch.float64).cuda()
    (ya, lda), (yb, ldb) = _both_paths(lambda: ops.flow_forward(x, w, nl, act))
    angle_close(ya, yb, atol=1e-11); close(lda, ldb, rtol=1e-12, atol=1e-10)
    (Sa, la, pa, qa), (Sb, lb, pb, qb) = _both_paths(lambda: ops.ft_action(x, w, nl, beta, act))
    close(Sa, Sb, rtol=1e-12, atol=1e-10); close(la, lb, rtol=1e-12, atol=1e-10); close(pa, pb, rtol=1e-12); close(qa, qb, atol=1e-10)
    Fa, Fb = _both_paths(lambda: ops.ft_force(x, w, nl, beta, act))
    close(Fa, Fb, rtol=1e-10, atol=1e-11 * float(Fb.abs().max()))
    assert torch.equal(Fa, ops.ft_force(x, w, nl, beta, act))                       # deterministic
    xs = (0.3 * x).contiguous()
    (xa, va), (xb_, vb) = _both_paths(lambda: ops.ft_leapfrog(xs, v, w, nl, beta, 0.05, 4, act))
    angle_close(xa, xb_, atol=1e-10); close(va, vb, rtol=1e-9, atol=1e-9)
    ra, rb = _both_paths(lambda: ops.ft_trajectory(xs, v, u, w, nl, beta, 0.05, 6, act))
    close(ra['H0'], rb['H0'], rtol=1e-12); close(ra['H1'], rb['H1'], rtol=1e-10); close(ra['dH'], rb['dH'], atol=1e-8)
    assert torch.equal(ra['acc'], rb['acc'])
    angle_close(ra['x_new'], rb['x_new'], atol=1e-9); close(ra['state'], rb['state'], rtol=1e-10, atol=1e-9)
    close(ra['plaq'], rb['plaq'], rtol=1e-10); close(ra['Q'], rb['Q'], atol=1e-9)
    # chained (state_in from the previous launch) == stateless, bit for bit; a chain alone == the chain in its batch
    rc = ops.ft_trajectory(ra['x_new'].clone(), v, u, w, nl, beta, 0.05, 6, act, state_in=ra['state'].clone())
    rd = ops.ft_trajectory(ra['x_new'].clone(), v, u, w, nl, beta, 0.05, 6, act)
    for k in ('x_new', 'dH', 'H0', 'H1', 'acc', 'state', 'plaq', 'Q'):
        assert torch.equal(rc[k], rd[k]), k
    k = B - 1
    r1 = ops.ft_trajectory(xs[k:k + 1].contiguous(), v[k:k + 1].contiguous(), u[k:k + 1].contiguous(), w, nl, beta, 0.05, 6, act)
    for key in ('x_new', 'dH', 'H0', 'H1', 'acc'):
        assert torch.equal(r1[key][0], ra[key][k]), key


def test_small_lattice_path_against_the_oracle_and_in_a_graph():
    """Config-2 shape against the oracle (not only against the other kernels), and the one-launch trajectory captured
    into a hipGraph and replayed."""
    gen = torch.Generator().manual_seed(2)
    B, L, nl, beta, dt, nstep = 6, 16, 4, 4.0, 0.1, 10
    flow = R.default_flow(nl, gen)
    w = ops.pack_weights(flow, device='cuda')
    x = ((torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * 0.4).contiguous()
    v = torch.randn(B, 2, L, L, generator=gen, dtype=torch.float64)
    u = torch.rand(B, generator=gen, dtype=torch.float64)
    assert ops.get_small_path()
    r = ops.ft_trajectory(x.cuda(), v.cuda(), u.cuda(), w, nl, beta, dt, nstep)
    dH, _, acc, newx, h0, h1 = R.ft_hmc(x, v, u, flow, beta, dt, nstep, mode='md')
    close(r['H0'], h0, rtol=1e-11); close(r['H1'], h1, rtol=1e-8); close(r['dH'], dH, rtol=1e-6, atol=1e-7)
    assert np.array_equal(H(r['acc']) > 0.5, H(acc))
    angle_close(r['x_new'], newx, atol=1e-7)
    close(ops.ft_force(x.cuda(), w, nl, beta), R.ft_force(x, flow, beta), rtol=1e-9, atol=1e-9)
    # graph capture: workspace warmed by the eager call above
    xd, vd, ud = x.cuda(), v.cuda(), u.cuda()
    out = {k: torch.empty_like(t) for k, t in r.items()}
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ops.ft_trajectory(xd, vd, ud, w, nl, beta, dt, nstep, out=out)
        st.synchronize()
        g = torch.cuda.CUDAGraph()
        with capture(g, st):
            ops.ft_trajectory(xd, vd, ud, w, nl, beta, dt, nstep, out=out)
        for t in out.values():
            t.zero_()
        g.replay()
        st.synchronize()
    for k in ('x_new', 'dH', 'H0', 'H1', 'acc', 'plaq', 'Q'):
        assert torch.equal(out[k], r[k]), k


@pytest.mark.parametrize('B,L', [(5, 128), (32, 256), (127, 128)])
def test_wave_split_action_sums_are_bit_identical(B, L):
    """few chains of a large lattice (B < 128, L >= 128) with a workspace at hand: the action / charge sums run one WAVE per
    workgroup (csrc/wilson.hip k_action_charge_waves) -- the same threads' sums added in the same order as the one-workgroup-
    per-chain kernel, which fthmc_wilson_action_charge (no workspace) still launches: every output bit-equal; the sum over a
    sweep's log J partials with one wave per layer (k_sum_parts) against the layers' own log J, added in order"""
    gen = torch.Generator().manual_seed(7 + B)
    x = ((torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi).cuda()
    beta = 3.0
    S0, Q0, p0 = ops.wilson_action_charge(x, beta)
    S1, ld, p1, Q1 = ops.ft_action(x, torch.zeros(0, dtype=torch.float64, device='cuda'), 0, beta)
    assert torch.equal(S0, S1) and torch.equal(Q0, Q1) and torch.equal(p0, p1) and float(ld.abs().max()) == 0.0
    if B <= 32:
        nl = 3
        flow = R.default_flow(nl, gen)
        w = ops.pack_weights(flow, device='cuda')
        S, ld, _, _ = ops.ft_action(x, w, nl, beta)
        y, tot = x, torch.zeros(B, dtype=torch.float64, device='cuda')
        for l in range(nl):
            y, lj = ops.flow_layer_fwd(y, w[l * 955:(l + 1) * 955], l % 2, (l // 2) % 4)
            tot = tot + lj
        assert torch.equal(ld, tot)
