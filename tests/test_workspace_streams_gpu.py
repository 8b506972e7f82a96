"""GPU tests of the host plumbing of fthmc_amd/ops.py (the CPU half: tests/test_scratch_cache.py): a captured graph keeps
replaying into the scratch of the families beside the flow workspace ('loops', 'instanton', 'train_force') after a larger call
replaced it -- tests/test_capture_gpu.py::test_workspace_survives_growth_after_capture holds the flow family to the same --, and
train_grad over explicit chain-group sizes."""
import math

import numpy as np
import pytest
import torch

from gpu_support import R, capture, module_defaults, ops

pytestmark = pytest.mark.gpu
_defaults = module_defaults()

BETA = 2.0


def links(B, L, gen):
    return ((torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi).cuda()


def loops_call(B, L, Rmax, gen):
    x, out = links(B, L, gen), torch.empty(B, Rmax, Rmax, dtype=torch.float64, device='cuda')
    return ops.wilson_loops_ws_bytes(B, L, Rmax, Rmax), lambda: (ops.wilson_loops(x, Rmax, out=out),)


def instanton_call(B, L, gen):
    x, seeds = links(B, L, gen), ops.chain_seeds(4242, 0, B, device='cuda')
    out = {'x': torch.empty_like(x), 'k': torch.empty(B, dtype=torch.int32, device='cuda'),
           'nacc': torch.empty(B, dtype=torch.int32, device='cuda')}
    return ops.instanton_ws_bytes(B, L, 2), lambda: ops.instanton_hit(x, BETA, seeds, n_hit=4, path=2, out=out)


def train_force_call(B, L, gen, w):
    x, gw = links(B, L, gen), torch.empty_like(w)

    def call():
        r = ops.train_force_grad(x, w, 2, BETA, out_gw=gw)
        assert r['gw'].data_ptr() == gw.data_ptr()
        return r['F'], r['force_sq'], r['gw']
    return ops.train_force_ws_bytes(B, L, 2), call


def family_calls(family, gen):
    """-> ((bytes, call) at the small shape, (bytes, call) at the large one); call() -> the tuple of result tensors"""
    if family == 'loops':
        return loops_call(2, 8, 2, gen), loops_call(4, 16, 8, gen)
    if family == 'instanton':
        # fthmc_instanton_ws_bytes(B, L, 2) is 256 at (1, 8) and still 256 at (3, 16) -- the size is rounded up to 256 bytes --;
        # (4, 16), the large shape of the other two families, is the first B at L = 16 that asks for more: 512
        return instanton_call(1, 8, gen), instanton_call(4, 16, gen)
    w = ops.pack_weights(R.default_flow(2, gen), device='cuda')
    return train_force_call(2, 8, gen, w), train_force_call(4, 16, gen, w)


def same(a, b):
    return len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))


@pytest.mark.parametrize('family', ('loops', 'instanton', 'train_force'))
def test_family_scratch_survives_growth_after_capture(family):
    from fthmc_amd._lib import FthmcError
    (n_small, small), (n_large, large) = family_calls(family, torch.Generator().manual_seed(31))
    assert 0 < n_small < n_large, (n_small, n_large)            # else nothing below grows
    st = torch.cuda.Stream()
    flow_key = (torch.cuda.current_device(), st.cuda_stream)
    key = flow_key + (family,)
    if key in ops._WS:      # the handle comes from a pool and may have served an earlier test: start without a buffer, keep that one alive
        ops._WS_RETIRED.append(ops._WS.pop(key))
    torch.cuda.synchronize()                                    # the inputs were made on the default stream
    with torch.cuda.stream(st):
        want = [t.clone() for t in small()]                      # warm-up: allocates this stream's buffer of the family
        st.synchronize()
        graph = torch.cuda.CUDAGraph()
        with capture(graph, st):
            got = small()
        with pytest.raises(FthmcError, match='graph capture'):
            g2 = torch.cuda.CUDAGraph()
            with capture(g2, st):
                large()                                          # would have to grow the buffer while capturing
        old_ptr = ops._WS[key].data_ptr()
        assert ops._WS[key].numel() * 8 < n_large
        flow_ptr = ops._WS[flow_key].data_ptr() if flow_key in ops._WS else None
        big = [t.clone() for t in large()]                       # eager: the buffer is replaced, the old one retired
        big2 = large()
        st.synchronize()
        assert same(big, big2)
        assert ops._WS[key].data_ptr() != old_ptr and ops._WS[key].numel() * 8 >= n_large
        assert any(b.data_ptr() == old_ptr for b in ops._WS_RETIRED)
        assert (ops._WS[flow_key].data_ptr() if flow_key in ops._WS else None) == flow_ptr
        for t in got:
            t.zero_()
        graph.replay()
        st.synchronize()
        assert same(got, want)


def test_train_grad_takes_explicit_group_sizes():
    """groups=[1, 2] of three chains: x, logq, logp are per chain and keep their bits; gw adds the groups' partial gradients
    (1/3 g_0 + 2/3 g_1) where one group adds the chains, so it agrees to rounding: 1e-12 of max |gw|; and with the oracle within
    what tests/test_layer_calls_gpu.py asks of a training gradient at this size."""
    gen = torch.Generator().manual_seed(77)
    B, L, nl = 3, 8, 2
    flow = R.default_flow(nl, gen)
    w = ops.pack_weights(flow, device='cuda')
    xi = links(B, L, gen)
    one = ops.train_grad(xi, w, nl, BETA, groups=1)
    two = ops.train_grad(xi, w, nl, BETA, groups=[1, 2])
    torch.cuda.synchronize()
    for k in ('x', 'logq', 'logp'):
        assert torch.equal(one[k], two[k]), k
    scale = float(one['gw'].abs().max())
    err = float((one['gw'] - two['gw']).abs().max())
    print(f'train_grad groups=[1, 2] against groups=1: max |dgw| = {err:.3e}, max |gw| = {scale:.3e}')
    assert err <= 1e-12 * scale
    _, grads = R.train_grads(xi.cpu(), flow, BETA)
    for li, row in enumerate(ops.unpack_weight_grads(two['gw'], nl)):
        for g, t in zip(row, grads[li]):
            np.testing.assert_allclose(g.cpu().numpy(), t.detach().numpy(), rtol=1e-8, atol=1e-10 * max(1.0, float(t.abs().max())))
