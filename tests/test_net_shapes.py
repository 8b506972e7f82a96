"""CPU: the cases of tests/net_shape_cases.py are fit to be held to 1e-9 per tensor and per chain, the oracle's conv net is right
where its circular pad is at its own limit, and the host-side shape arithmetic of fthmc_amd.ops and of the library's
make_flow_arch holds at every case's shape and at every limit from both sides.

Admissibility is the condition second_order_cases.py states, asserted for both orders as tests/test_first_order_hard.py and
tests/test_second_order_hard.py do: the oracle at the inputs and at a copy with every link and weight moved by one relative 2^-52
(three sets of signs) differ by at most 1e-12 on every parameter tensor and every chain; pytest -s prints each case's figures.

The second statement of the conv net: a direct NumPy longdouble circular convolution, a sum of np.roll-ed planes over
(ci, ky, kx).  np.roll is right for any number of wraps, where F.pad(mode='circular') refuses pad > L and is at its limit at
pad == L (k9_L4)."""
import ctypes

import numpy as np
import pytest
import torch

import net_shape_cases as N
from oracle import ref_cpu as R


@pytest.mark.parametrize('case', N.CASES, ids=N.IDS)
def test_reference_is_well_conditioned_at_the_case(case):
    inp, ref1, ref2 = N.inputs(case), N.first_order(case), N.second_order(case)
    first, second = N.sensitivities(case, 9000 + 10 * N.CASES.index(case))
    (n1, e1), (n2, e2) = N.worst(first), N.worst(second)
    print(f'{case.name}: sensitivity, first order {e1:.1e} ({n1}), second order {e2:.1e} ({n2})')
    assert all(torch.isfinite(ref1[k]).all() for k in ('F', 'y', 'lf_x', 'lf_v', 'S_eff', 'logdet', 'logq', 'logp'))
    assert all(torch.isfinite(ref2[k]).all() for k in ('F', 'Hg', 'ax', 'force_sq'))
    # every quantity the GPU file compares is among the entries held
    B, nl, npar = case.B, case.nl, 2 * (len(case.arch[0]) + 1)
    assert len(first) == 2 * npar * nl + 9 * B + 2 * nl * B, len(first)
    assert len(second) == 3 * npar * nl + 4 * B, len(second)
    N.hold(first, N.SENS_BOUND, f'{case.name}, first order')
    N.hold(second, N.SENS_BOUND, f'{case.name}, second order')
    # the inputs are the hard ones: links on the cut in chain 0, the weights scaled
    assert float(inp.x[0, 0, 0, 0]) == np.pi - 1e-9 and float(inp.x[0, 1, 0, 0]) == -np.pi + 1e-9
    k = case.arch[1]
    assert 1.0 / np.sqrt(2 * k * k) < float(inp.flow[0][0].abs().max()) <= case.scale / np.sqrt(2 * k * k)


def test_cases_cover_what_they_are_for():
    """every edge the cases are named for, with seeds of their own; inputs and references made once and never modified"""
    by = N.BY_NAME
    assert len(by) == len(N.CASES) == 11 and not set(by) & {c.name for c in N.FC.CASES}
    assert all(c.scale == 2.0 and c.arch is not None and c.L % 4 == 0 and c.arch[1] // 2 <= c.L for c in N.CASES)
    assert [N.seed(c) for c in N.CASES[:2]] == [73480, 73441] and len({N.seed(c) for c in N.CASES}) == 11
    assert by['k9_L4'].arch[1] // 2 == by['k9_L4'].L and by['k9_L4'].nl == 8
    assert by['k5_L4_nohidden'].arch[0] == () and by['k5_L4_nohidden'].arch[1] > by['k5_L4_nohidden'].L
    assert by['k15_L8'].arch[1] == 15 > by['k15_L8'].L and by['k1_L4'].arch == ((8, 8), 1, 2)
    assert by['wide256'].arch[0] == (256, 256) and 256 * 256 * 9 + 256 == 590080
    hidden, _, n_mix = by['mix64'].arch
    assert n_mix == 64 and n_mix + 1 > max(hidden + (2,))                           # the output sets cmax
    assert by['uneven_mix1'].arch == ((3, 17, 2), 3, 1) and by['uneven_mix1'].B % 2 == 1
    assert len(by['deep8'].arch[0]) == 8 and by['tanh_net'].tanh and N.inputs(by['tanh_net']).act == 'leaky_relu+tanh'
    assert N.arch(by['tanh_net']) == ((5,), 5, 3, True) and N.arch(by['deep8']) == by['deep8'].arch
    assert by['L20_k7'].L ** 2 > 256
    c = by['L132_stride']
    assert c.L ** 2 > 64 * 256 and c.B * max(c.arch[0]) * c.L ** 2 > 4096 * 256                 # sgrid and egrid both go round twice
    assert {c.act for c in N.CASES} == {'silu', 'relu', 'leaky_relu'}
    c = by['k1_L4']
    assert N.inputs(c) is N.inputs(c) and N.first_order(c) is N.first_order(c) and N.second_order(c) is N.second_order(c)
    assert N.layers_at_every_stripe(c) is N.layers_at_every_stripe(c) and sorted(set(N.MU_OFF)) == [(m, o) for m in (0, 1) for o in range(4)]
    # a layer beyond the case's own reuses the weights of layer li % layers, at its own (mu, off)
    inp8 = N.eight_layers(N.inputs(c))
    assert len(inp8.flow) == 8 and inp8.flow[5] is N.inputs(c).flow[1] and inp8.x is N.inputs(c).x
    assert torch.equal(N.layers_at_every_stripe(c)['layer_y'][1], N.first_order(c)['layer_y'][1])


# ------------------------------------------------------------------------------------------- the oracle's conv, a second statement
def roll_conv(a, w, b):
    """[B][Cin][L][L] (*) [Cout][Cin][k][k] + [Cout], circular, in longdouble: out[s] = b + sum w[ci, ky, kx] a[ci][s + (ky - r, kx - r)],
    the shifted plane as np.roll by (r - ky, r - kx) -- right for any number of wraps"""
    a, w, b = (np.asarray(t, dtype=np.longdouble) for t in (a, w, b))
    cout, cin, k, _ = w.shape
    r = k // 2
    out = np.zeros((a.shape[0], cout) + a.shape[2:], dtype=np.longdouble) + b[None, :, None, None]
    for ci in range(cin):
        for ky in range(k):
            for kx in range(k):
                plane = np.roll(a[:, ci], (r - ky, r - kx), axis=(1, 2))
                out += w[None, :, ci, ky, kx, None, None] * plane[:, None]
    return out


def roll_net(inp, w, act, final_tanh):
    fn = {'silu': lambda z: z / (1 + np.exp(-z)), 'relu': lambda z: np.maximum(z, 0),
          'leaky_relu': lambda z: np.where(z > 0, z, np.longdouble(0.01) * z)}[act]
    h = np.asarray(inp.numpy(), dtype=np.longdouble)
    n = len(w) // 2
    for li in range(n):
        h = roll_conv(h, w[2 * li].numpy(), w[2 * li + 1].numpy())
        if li != n - 1:
            h = fn(h)
    return np.tanh(h) if final_tanh else h


@pytest.mark.parametrize('final_tanh', [False, True], ids=['plain', 'tanh'])
@pytest.mark.parametrize('name', ['k9_L4', 'k5_L4_nohidden', 'k15_L8', 'k1_L4'])
def test_oracle_conv_net_against_rolled_planes(name, final_tanh):
    """oracle.ref_cpu.conv_net at the net input of the case's layer 0 (cos P, sin P on the frozen stripes of (0, 0), (1, 0)
    elsewhere) against the rolled-plane statement: 1e-14 of the largest output"""
    case = N.BY_NAME[name]
    assert np.finfo(np.longdouble).eps < 2.0 ** -60
    inp = N.inputs(case)
    mF = R.stripe_masks(case.L, 0, 0)[1]
    x2 = mF * R.plaq(inp.x)
    net_in = torch.stack((torch.cos(x2), torch.sin(x2)), dim=1)
    for lw in inp.flow:
        got = R.conv_net(net_in, lw, case.act + ('+tanh' if final_tanh else '')).numpy()
        ref = roll_net(net_in, lw, case.act, final_tanh)
        assert got.shape == ref.shape == (case.B, case.arch[2] + 1, case.L, case.L)
        err = float(np.abs(got - ref).max() / np.abs(ref).max())
        assert err <= 1e-14, (name, err)
    # where k > L the taps alias: the same net is NOT the one whose kernel is cut to the lattice (the statement can tell)
    if case.arch[1] > case.L:
        w0 = inp.flow[0][0].numpy()
        c = (case.arch[1] - case.L + 1) // 2
        cut = np.zeros_like(w0)
        cut[:, :, c:-c, c:-c] = w0[:, :, c:-c, c:-c]
        full = roll_conv(net_in.numpy(), w0, inp.flow[0][1].numpy())
        assert np.abs(full - roll_conv(net_in.numpy(), cut, inp.flow[0][1].numpy())).max() > 1e-3 * np.abs(full).max()


# ------------------------------------------------------------------------------------------- host-side shape arithmetic
def torch_param_shapes(hidden, k, n_mix):
    chans = [2, *hidden, n_mix + 1]
    convs = [torch.nn.Conv2d(ci, co, k) for ci, co in zip(chans[:-1], chans[1:])]
    return [tuple(p.shape) for c in convs for p in (c.weight, c.bias)]


@pytest.mark.parametrize('case', N.CASES, ids=N.IDS)
def test_parameter_counts_are_the_pytorch_ones(case):
    """ops.arch_params, the library's fthmc_arch_params, ops.pack_weights and ops.unpack_weight_grads at the case's shape against
    the parameter shapes of torch.nn.Conv2d"""
    from fthmc_amd import _lib, ops
    hidden, k, n_mix = case.arch
    shapes = torch_param_shapes(hidden, k, n_mix)
    total = sum(int(np.prod(s)) for s in shapes)
    a = N.arch(case)
    assert ops.arch_params(a) == total == int(_lib.load().fthmc_arch_params(ops._arch(a)))
    inp = N.inputs(case)
    assert [tuple(t.shape) for t in inp.flow[0]] == shapes
    w = ops.pack_weights(inp.flow, final_tanh=case.tanh)
    assert ops.arch_of(w) == a and w.numel() == case.nl * total
    rows = ops.unpack_weight_grads(w, case.nl)
    assert len(rows) == case.nl
    for row, lw in zip(rows, inp.flow):
        assert [tuple(t.shape) for t in row] == shapes and all(torch.equal(a_, b_) for a_, b_ in zip(row, lw))
    # second_order_cases.split, which the comparisons use, agrees
    assert all(torch.equal(a_, b_) for ra, rb in zip(N.C.split(w, inp.flow), rows) for a_, b_ in zip(ra, rb))


def test_the_output_sets_the_scratch_width_of_mix64():
    """FlowArch::cmax() (hbuf, gbuf) is the widest of ALL channel counts, the n_mix + 1 outputs included: the workspaces of mix64
    are larger than those of the same net with two components by more than its larger stash alone"""
    from fthmc_amd import _lib, ops
    case = N.BY_NAME['mix64']
    hidden, k, n_mix = case.arch
    B, L, nl = case.B, case.L, case.nl
    small = (hidden, k, 2)
    n = B * L * L
    for fn in (ops.ws_bytes, ops.vjp_ws_bytes):
        assert fn(B, L, nl, case.arch) > fn(B, L, nl, small) > 0
    stash = lambda a: int(_lib.load().fthmc_layer_stash_bytes(ops._arch(a), B, L))
    assert stash(case.arch) - stash(small) == (n_mix - 2) * n * 8
    # beyond the stash of every layer: hbuf and the two halves of gbuf, B cmax L^2 each with cmax = 65 against 3 (doubles in the
    # first-order workspace, dual numbers in the second-order one, which also holds the larger weight gradient)
    scratch = 3 * (n_mix + 1 - 3) * n * 8
    extra = ops.ws_bytes(B, L, nl, case.arch) - ops.ws_bytes(B, L, nl, small) - nl * (n_mix - 2) * n * 8
    assert abs(extra - scratch) < 4096, (extra, scratch)                    # the regions' alignment
    extra = ops.vjp_ws_bytes(B, L, nl, case.arch) - ops.vjp_ws_bytes(B, L, nl, small) - 2 * nl * (n_mix - 2) * n * 8
    gw = 2 * nl * (n_mix - 2) * (hidden[-1] * k * k + 1) * 8
    assert abs(extra - 2 * scratch - gw) < 4096, (extra, scratch, gw)


def _arch_t(hidden, k, n_mix):
    from fthmc_amd import _lib
    a = _lib.ArchT()
    a.n_hidden, a.kernel_size, a.n_mix, a.final_tanh = len(hidden), k, n_mix, 0
    for i, h in enumerate(hidden[:8]):
        a.hidden[i] = h
    return ctypes.pointer(a)


LIMITS = [  # (accepted, first refused), as (hidden, k, n_mix, L)
    ('hidden layers', ((2,) * 8, 3, 2, 8), ((2,) * 9, 3, 2, 8)),
    ('channels', ((256,), 3, 2, 8), ((257,), 3, 2, 8)),
    ('channels, last hidden', ((4, 256), 3, 2, 8), ((4, 257), 3, 2, 8)),
    ('kernel_size', ((4,), 15, 2, 8), ((4,), 17, 2, 8)),
    ('n_mix', ((4,), 3, 64, 8), ((4,), 3, 65, 8)),
    ('n_mix, below', ((4,), 3, 1, 8), ((4,), 3, 0, 8)),
    ('kernel_size // 2 against L', ((4,), 9, 2, 4), ((4,), 11, 2, 4)),
]


@pytest.mark.parametrize('what,ok,bad', LIMITS, ids=[l[0] for l in LIMITS])
def test_every_limit_of_the_net_shape_from_both_sides(what, ok, bad):
    """make_flow_arch (csrc/flow_generic.hip) and the kernel_size // 2 <= L of gen_fwd / gen_bwd, through calls that refuse before
    any launch: the size queries answer for the last accepted shape and return 0 / FTHMC_ERR_UNSUPPORTED for the first refused
    one, and every entry point refuses that one with FTHMC_ERR_UNSUPPORTED (its pointers are never dereferenced)"""
    from fthmc_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(64)
    B, nl, big = 2, 1, 1 << 40
    hidden, k, n_mix, L = ok
    a = _arch_t(hidden, k, n_mix)
    chans = [2, *hidden, n_mix + 1]
    assert lib.fthmc_arch_params(a) == sum(co * ci * k * k + co for ci, co in zip(chans[:-1], chans[1:]))
    assert lib.fthmc_layer_stash_bytes(a, B, L) == B * L * L * (3 + sum(chans[1:])) * 8
    assert lib.fthmc_ws_bytes(a, B, L, nl) > 0 and lib.fthmc_train_ws_bytes(a, B, L, nl) > 0
    assert lib.fthmc_vjp_ws_bytes(a, B, L, nl) > 0 and lib.fthmc_train_force_ws_bytes(a, B, L, nl) > 0
    hidden, k, n_mix, L = bad
    a = _arch_t(hidden, k, n_mix)
    fits_arch = k // 2 > L                                  # the one limit that is the lattice's, not make_flow_arch's
    if fits_arch:
        assert lib.fthmc_arch_params(a) > 0 and lib.fthmc_layer_stash_bytes(a, B, L) > 0
    else:
        assert lib.fthmc_arch_params(a) == -2 and lib.fthmc_layer_stash_bytes(a, B, L) == 0
        assert lib.fthmc_ws_bytes(a, B, L, nl) == 0 and lib.fthmc_train_ws_bytes(a, B, L, nl) == 0
    assert lib.fthmc_vjp_ws_bytes(a, B, L, nl) == 0 and lib.fthmc_train_force_ws_bytes(a, B, L, nl) == 0
    assert lib.fthmc_flow_layer_fwd(p, p, a, B, L, 0, 0, 0, p, p, p, big, None) == -2
    assert lib.fthmc_flow_layer_rev(p, p, a, B, L, 0, 0, 0, 1e-12, p, p, p, big, None) == -2
    assert lib.fthmc_flow_layer_bwd(p, p, a, p, p, B, L, 0, 0, 0, p, p, p, big, None) == -2
    assert lib.fthmc_flow_forward(p, p, a, nl, B, L, 0, p, p, p, big, None) == -2
    assert lib.fthmc_ft_force(p, p, a, nl, B, L, 0, 1.0, p, p, big, None) == -2
    assert lib.fthmc_ft_force_vjp(p, p, a, nl, B, L, 0, 1.0, p, p, p, p, big, None) == -2
    assert lib.fthmc_train_force_grad(p, p, a, nl, B, L, 0, 1.0, p, p, p, p, big, None) == -2


def test_the_python_side_refuses_the_same_shapes():
    """ops.pack_weights at the limits: 8 hidden layers of 256 channels, k = 15 and 64 components pack; one more of each raises"""
    from fthmc_amd import ops
    from fthmc_amd._lib import FthmcError
    z = torch.zeros

    def net(hidden, k, n_mix):
        chans = [2, *hidden, n_mix + 1]
        return [t for ci, co in zip(chans[:-1], chans[1:]) for t in (z(co, ci, k, k), z(co))]
    for hidden, k, n_mix in (((2,) * 8, 3, 2), ((256, 1), 3, 2), ((2,), 15, 2), ((2,), 3, 64)):
        assert ops.arch_of(ops.pack_weights([net(hidden, k, n_mix)])) == (hidden, k, n_mix)
    for hidden, k, n_mix in (((2,) * 9, 3, 2), ((257, 1), 3, 2), ((2,), 17, 2), ((2,), 3, 65)):
        with pytest.raises(FthmcError, match='beyond the limits of the HIP kernels'):
            ops.pack_weights([net(hidden, k, n_mix)])
