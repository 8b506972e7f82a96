"""The kernels at the edges of the shapes their entry points accept (include/fthmc_hip.h), checked by periodicity.

Every site of a lattice sees only its neighbourhood, and the flow's stripe masks have period 4: a field tiled from a small one
gives, site for site, the small field's outputs, bit for bit, and its sums scale with the number of tiles.  Identical chains
give identical per-chain results.  So the largest accepted shapes are checked against small ones that the oracle tests pin.
tests/test_index_limits.py shows on the CPU that the 32-bit offsets of the accepted shapes fit; these tests run them.  The
large-lattice cases need tens of GB of device memory and skip, with the amount, where it is not free.
"""
import math
import os
import re

import pytest
import torch

from conftest import ROOT
from gpu_support import module_defaults

pytestmark = pytest.mark.gpu
_defaults = module_defaults()

HDR = open(os.path.join(ROOT, 'include', 'fthmc_hip.h')).read()
MAX_B = int(re.search(r'#define FTHMC_MAX_B (\d+)', HDR).group(1))
MAX_L = int(re.search(r'#define FTHMC_MAX_L (\d+)', HDR).group(1))


def need_memory(nbytes, what):
    free = torch.cuda.mem_get_info()[0]
    if free < 1.1 * nbytes:
        pytest.skip(f'{what}: needs {nbytes / 2**30:.1f} GiB of device memory, {free / 2**30:.1f} GiB free')


def field(B, L, seed):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(B, 2, L, L, generator=g, dtype=torch.float64) * 2 - 1) * math.pi).cuda()


def close(big, small, scale, rel=1e-12):
    return float((big - small * scale).abs().max()) <= rel * max(1.0, float((small * scale).abs().max()))


@pytest.fixture
def release():
    yield
    from fthmc_amd import ops
    ops.release_workspaces()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------- plain lattice, B
@pytest.mark.parametrize('B', [65537, MAX_B])
def test_plain_lattice_at_large_chain_counts(B, release):
    """B identical chains of L = 4 give the B = 1 results in every chain: the chain index runs through blockIdx.x / y / z of
    every plain-lattice kernel past 65536 and up to FTHMC_MAX_B"""
    from fthmc_amd import ops
    L, beta = 4, 2.0
    need_memory(B * 2 * L * L * 8 * 12, f'B = {B}')
    x1 = field(1, L, 11)
    v1 = torch.randn(1, 2, L, L, generator=torch.Generator().manual_seed(12), dtype=torch.float64).cuda()
    u1 = torch.full((1,), 0.5, dtype=torch.float64, device='cuda')
    xB, vB, uB = x1.expand(B, -1, -1, -1).contiguous(), v1.expand(B, -1, -1, -1).contiguous(), u1.expand(B).contiguous()

    def same(big, small, what):
        assert torch.equal(big, small.expand_as(big)), what

    same(ops.plaquettes(xB), ops.plaquettes(x1), 'plaquettes')
    for a, b, k in zip(ops.wilson_action_charge(xB, beta), ops.wilson_action_charge(x1, beta), ('S', 'Q', 'plaq')):
        same(a, b, k)
    same(ops.wilson_force(xB, beta), ops.wilson_force(x1, beta), 'force')
    same(ops.kinetic(vB), ops.kinetic(v1), 'kinetic')
    for a, b, k in zip(ops.leapfrog(xB, vB, beta, 0.1, 3), ops.leapfrog(x1, v1, beta, 0.1, 3), ('x', 'p')):
        same(a, b, 'leapfrog ' + k)
    rB, r1 = ops.hmc_trajectory(xB, vB, uB, beta, 0.1, 3), ops.hmc_trajectory(x1, v1, u1, beta, 0.1, 3)
    for k in ('x_new', 'dH', 'acc', 'H0', 'H1'):
        same(rB[k], r1[k], 'hmc ' + k)
    seeds = torch.full((B,), 1234, dtype=torch.int64, device='cuda')
    vr, ur = ops.random_momenta(seeds, (B, 2, L, L))
    v1r, u1r = ops.random_momenta(seeds[:1], (1, 2, L, L))
    same(vr, v1r, 'random momenta')
    same(ur, u1r, 'random uniforms')
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------- plain lattice, L
def test_plain_lattice_at_the_largest_lattice(release):
    """L = FTHMC_MAX_L (17 GB per field): plaquettes, Wilson force and action of a field tiled from an L = 4 one"""
    from fthmc_amd import ops
    L, beta, t = MAX_L, 2.0, MAX_L // 4
    need_memory(2 * L * L * 8 * 3 + L * L * 8, f'L = {L}')
    x1 = field(1, 4, 13)
    x = x1.repeat(1, 1, t, t)
    P = ops.plaquettes(x)
    assert torch.equal(P, ops.plaquettes(x1).repeat(1, t, t))
    del P
    F = ops.wilson_force(x, beta)
    assert torch.equal(F, ops.wilson_force(x1, beta).repeat(1, 1, t, t))
    del F
    S, Q, plaq = ops.wilson_action_charge(x, beta)
    S1, Q1, plaq1 = ops.wilson_action_charge(x1, beta)
    assert close(S, S1, t * t, rel=1e-10) and close(plaq, plaq1, 1.0, rel=1e-10) and close(Q, Q1, t * t, rel=1e-9)


# ---------------------------------------------------------------------------------------------------------- flow
def _flow(nl=2):
    from fthmc_amd import ops
    from oracle import ref_cpu as R
    flow = R.default_flow(nl, torch.Generator().manual_seed(21))
    return ops.pack_weights(flow, device='cuda'), nl


def _same_in_every_chain(big, small, what):
    assert torch.equal(big, small.expand_as(big)), what


def test_generic_flow_kernels_at_large_chain_counts(release):
    """B = 65537 identical chains of L = 4 through csrc/flow_generic.hip (hidden = (2,), k = 3, two components, two layers): its
    launches carry the chain index in gridDim.y / gridDim.z (k_gen_transform: gridDim.x), past 65535 here.  Every chain of
    flow_forward, ft_action, ft_force and of ft_force_vjp's H g is the B = 1 result; train_grad returns the gradient of the MEAN
    over the chains, the chain sum (B times the single gradient) over B: the single one, to `close`"""
    from fthmc_amd import _lib, ops
    from oracle import ref_cpu as R
    B, L, nl, beta, arch = 65537, 4, 2, 2.0, ((2,), 3, 2)
    flow = R.default_flow(nl, torch.Generator().manual_seed(25), hidden=arch[0], k=arch[1], n_mix=arch[2])
    w = ops.pack_weights(flow, device='cuda')
    assert ops.arch_of(w) == arch != ops.DEFAULT_ARCH and B > 65535
    need_memory(int(_lib.load().fthmc_train_ws_bytes(ops._arch(arch), B, L, nl)) + ops.vjp_ws_bytes(B, L, nl, arch)
                + 8 * B * 2 * L * L * 8, f'generic net, B = {B}')
    x1 = field(1, L, 27)
    g1 = torch.randn(1, 2, L, L, generator=torch.Generator().manual_seed(28), dtype=torch.float64).cuda()
    xB, gB = x1.expand(B, -1, -1, -1).contiguous(), g1.expand(B, -1, -1, -1).contiguous()
    for a, b, k in zip(ops.flow_forward(xB, w, nl), ops.flow_forward(x1, w, nl), ('y', 'logdet')):
        _same_in_every_chain(a, b, 'flow_forward ' + k)
    for a, b, k in zip(ops.ft_action(xB, w, nl, beta), ops.ft_action(x1, w, nl, beta), ('S_eff', 'logdet', 'plaq', 'Q')):
        _same_in_every_chain(a, b, 'ft_action ' + k)
    _same_in_every_chain(ops.ft_force(xB, w, nl, beta), ops.ft_force(x1, w, nl, beta), 'ft_force')
    _same_in_every_chain(ops.ft_force_vjp(xB, w, nl, beta, gB, need_gw=False)[0], ops.ft_force_vjp(x1, w, nl, beta, g1, need_gw=False)[0],
                         'ft_force_vjp Hg')
    rB, r1 = ops.train_grad(xB, w, nl, beta), ops.train_grad(x1, w, nl, beta)
    for k in ('x', 'logq', 'logp'):
        _same_in_every_chain(rB[k], r1[k], 'train_grad ' + k)
    print('train_grad gw, B = %d against B = 1: %.1e' % (B, float((rB['gw'] - r1['gw']).abs().max() / r1['gw'].abs().max())))
    assert close(rB['gw'], r1['gw'], 1.0)
    torch.cuda.synchronize()


def test_tuned_flow_kernels_at_the_largest_chain_count(release):
    """B = 2^20 identical chains of L = 4, the largest B flow_shape_ok accepts (the tuned launches carry (B + 7) / 8 = 131072 in
    gridDim.z): every chain of flow_forward, ft_action and ft_force is the B = 1 result.  tests/test_index_limits.py has the first
    refused B."""
    from fthmc_amd import ops
    w, nl = _flow()
    B, L, beta = 1 << 20, 4, 2.0
    assert ops.arch_of(w) == ops.DEFAULT_ARCH and ops.get_variant() == 1
    need_memory(ops.ws_bytes(B, L, nl) + 4 * B * 2 * L * L * 8, f'default net, B = {B}')
    x1 = field(1, L, 29)
    xB = x1.expand(B, -1, -1, -1).contiguous()
    for a, b, k in zip(ops.flow_forward(xB, w, nl), ops.flow_forward(x1, w, nl), ('y', 'logdet')):
        _same_in_every_chain(a, b, 'flow_forward ' + k)
    for a, b, k in zip(ops.ft_action(xB, w, nl, beta), ops.ft_action(x1, w, nl, beta), ('S_eff', 'logdet', 'plaq', 'Q')):
        _same_in_every_chain(a, b, 'ft_action ' + k)
    _same_in_every_chain(ops.ft_force(xB, w, nl, beta), ops.ft_force(x1, w, nl, beta), 'ft_force')
    torch.cuda.synchronize()


def test_flow_refuses_the_first_lattice_past_its_limit(release):
    """L = 8196: the tuned kernels' launchers refuse with FTHMC_ERR_ARG (flow_shape_ok: the stash planes' byte offsets)"""
    from fthmc_amd import ops
    from fthmc_amd._lib import FthmcError
    w, nl = _flow()
    L = 8196
    need_memory(ops.ws_bytes(1, L, nl) + 2 * 2 * L * L * 8, f'L = {L}')
    x = torch.zeros(1, 2, L, L, dtype=torch.float64, device='cuda')
    with pytest.raises(FthmcError, match=r'code -1\b'):
        ops.ft_force(x, w, nl, 2.0)
    torch.cuda.synchronize()


def test_training_refuses_a_stash_past_32_bits(release):
    """35 B L^2 >= 2^32 (L = 1024, B = 118): one call of the training sweep refuses with FTHMC_ERR_UNSUPPORTED; 117 chains
    would fit (the callers split larger batches into chain groups)"""
    from fthmc_amd import _lib, ops
    from fthmc_amd._lib import FthmcError
    w, nl = _flow()
    L, B = 1024, 118
    assert 35 * (B - 1) * L * L < 2 ** 32 <= 35 * B * L * L
    need_memory(int(_lib.load().fthmc_train_ws_bytes(None, B, L, nl)) + 2 * B * 2 * L * L * 8, f'training B = {B}, L = {L}')
    x = torch.zeros(B, 2, L, L, dtype=torch.float64, device='cuda')
    with pytest.raises(FthmcError, match=r'code -2\b'):
        ops.train_grad(x, w, nl, 2.0)
    torch.cuda.synchronize()


def test_flow_at_the_largest_lattice_is_the_tiled_small_one(release):
    """L = 8192, B = 1 (the largest shape of the tuned kernels) from an L = 64 field tiled 128 x 128 (tiles aligned at 16, stripe
    period 4): the flowed field and the force site for site bit-identical, log J, S_eff and Q 16384 times the small ones"""
    from fthmc_amd import ops
    w, nl = _flow()
    L, t, beta = 8192, 128, 2.0
    need_memory(ops.ws_bytes(1, L, nl) + 3 * 2 * L * L * 8, f'L = {L}')
    xs = field(1, 64, 17)
    x = xs.repeat(1, 1, t, t)
    y, ld = ops.flow_forward(x, w, nl)
    ys, lds = ops.flow_forward(xs, w, nl)
    assert torch.equal(y, ys.repeat(1, 1, t, t)) and close(ld, lds, t * t, rel=1e-10)
    del y
    F = ops.ft_force(x, w, nl, beta)
    assert torch.equal(F, ops.ft_force(xs, w, nl, beta).repeat(1, 1, t, t))
    del F
    S, ldA, plaq, Q = ops.ft_action(x, w, nl, beta)
    Ss, ldAs, plaqs, Qs = ops.ft_action(xs, w, nl, beta)
    # sums of 6.7e7 site terms in another order than 16384 times the sum of 4096: 1e-10 relative (log J and Q mix signs)
    assert close(S, Ss, t * t, rel=1e-10) and close(ldA, ldAs, t * t, rel=1e-10) and close(plaq, plaqs, 1.0, rel=1e-10)
    assert close(Q, Qs, t * t, rel=1e-9)
    torch.cuda.synchronize()


def test_training_at_the_largest_lattice_is_the_tiled_small_one(release):
    """fthmc_train_grad at L = 8192, B = 1 (35 L^2 < 2^32: one call): the flowed field bit-identical to the tiles of the
    L = 64 one, log q / log p and the weight gradient 16384 times the small ones"""
    from fthmc_amd import _lib, ops
    w, nl = _flow()
    L, t, beta = 8192, 128, 2.0
    need_memory(int(_lib.load().fthmc_train_ws_bytes(None, 1, L, nl)) + 3 * 2 * L * L * 8, f'training L = {L}')
    xs = field(1, 64, 19)
    x = xs.repeat(1, 1, t, t)
    r = ops.train_grad(x, w, nl, beta)
    rs = ops.train_grad(xs, w, nl, beta)
    assert torch.equal(r['x'], rs['x'].repeat(1, 1, t, t))
    assert close(r['logq'], rs['logq'], t * t, rel=1e-10) and close(r['logp'], rs['logp'], t * t, rel=1e-10)
    assert close(r['gw'], rs['gw'], t * t, rel=1e-10)
    torch.cuda.synchronize()
