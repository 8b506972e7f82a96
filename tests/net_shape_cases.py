"""Net shapes at the edges of what csrc/flow_generic.hip accepts (make_flow_arch: up to 8 hidden layers of up to 256 channels, odd
kernel_size up to 15, 1 .. 64 mixture components, L % 4 == 0 with kernel_size // 2 <= L), on the hard inputs and under the measures
of tests/second_order_cases.py and tests/first_order_cases.py: shared by tests/test_net_shapes.py (CPU: the oracle's own
conditioning at these inputs, the oracle's conv against a second statement, the host-side shape arithmetic) and
tests/test_net_shapes_gpu.py (the kernels).  A plain module.

Cases, measure, bound and the rule that admits a case are imported, not copied: weights oracle.ref_cpu.default_flow(..., hidden, k,
n_mix) times `scale`, links pinned 1e-9 from +-pi, max|got - ref| / max|ref| <= BOUND = 1e-9 per parameter tensor and per chain,
admissible where the oracle itself moves by at most SENS_BOUND = 1e-12 under a move of every input by one relative 2^-52.  A case
that misses the condition gets a smaller scale or fewer layers, never a looser bound (uneven_mix1 did and lost a layer; every case
runs at scale 2.0; the figures are in the docstring of tests/test_net_shapes_gpu.py).  The inputs have a seed of their own,
73000 + 100 L + 10 layers + index; the cases are NOT appended to second_order_cases.CASES or first_order_cases.FIRST_ONLY, whose
indices seed existing inputs and fixtures.

Each case is the smallest shape that reaches its edge."""
import math

import torch

import first_order_cases as FC
import second_order_cases as C
from first_order_cases import compare, layer_vjp                                    # noqa: F401
from oracle import ref_cpu as R
from second_order_cases import (BETA, BOUND, SENS_BOUND, Case, Inputs, hold, nudged, per_chain, per_tensor,  # noqa: F401
                                pin_links, worst)

first_order_results = FC.oracle_results
second_order_results = C.oracle_results

SCALE = 2.0
CASES = [
    # k // 2 == L, the last shape gen_fwd / gen_bwd accept: 9 taps of a kernel row on 4 sites (wrapc wraps once, only just
    # enough); 8 layers = all eight (mu, off) in the sweeps
    Case('k9_L4', 4, 2, 8, SCALE, 'silu', ((4,), 9, 2), False),
    Case('k5_L4_nohidden', 4, 2, 4, SCALE, 'silu', ((), 5, 2), False),              # nh = 0 together with aliasing taps
    Case('k15_L8', 8, 2, 2, SCALE, 'leaky_relu', ((3,), 15, 3), False),             # the largest kernel, k > L
    Case('k1_L4', 4, 2, 2, SCALE, 'relu', ((8, 8), 1, 2), False),                   # k = 1; the default widths, not the default net
    Case('wide256', 4, 2, 1, SCALE, 'silu', ((256, 256), 3, 2), False),             # channel limit; 590 080 weight-gradient workgroups
    Case('mix64', 8, 2, 2, SCALE, 'relu', ((1,), 3, 64), False),                    # component limit; one hidden channel; cmax from the output
    # non-monotone widths, one component, odd B.  Planned with 4 layers: on its seed the second order missed the condition
    # (gw_vjp layer 2 tensor 7 moved by 1.1e-12 > SENS_BOUND), so it runs with 3 layers (2.7e-14), at the scale of the others
    Case('uneven_mix1', 12, 3, 3, SCALE, 'silu', ((3, 17, 2), 3, 1), False),
    Case('deep8', 8, 2, 3, SCALE, 'silu', ((2,) * 8, 3, 2), False),                 # eight hidden layers
    Case('tanh_net', 8, 2, 4, SCALE, 'leaky_relu', ((5,), 5, 3), True),             # the final tanh on another shape
    Case('L20_k7', 20, 2, 2, SCALE, 'silu', ((6,), 7, 2), False),                   # n = 400 > 256 threads: k_gen_transform, k_gen_conv_bwd_w
    # L^2 = 17424 > 16384 = 64 x 256 (sgrid) and B 32 L^2 = 1115136 > 2^20 = 4096 x 256 (egrid): both grid-stride loops go round twice
    Case('L132_stride', 132, 2, 1, SCALE, 'silu', ((32,), 3, 2), False),
]
BY_NAME = {c.name: c for c in CASES}
IDS = [c.name for c in CASES]
MU_OFF = [R.layer_mu_off(li) for li in range(8)]                                   # all eight (mu, off), in the flow's order

_INPUTS, _FIRST, _SECOND, _LAYERS = {}, {}, {}, {}


def arch(case):
    """the case's net shape as fthmc_amd.ops names it: (hidden, k, n_mix), with a fourth entry True for a final tanh"""
    return case.arch + ((True,) if case.tanh else ())


def seed(case):
    return 73000 + 100 * case.L + 10 * case.nl + CASES.index(case)


def inputs(case):
    """the inputs of a case, built like second_order_cases.inputs, made once and never modified"""
    if case.name not in _INPUTS:
        gen = torch.Generator().manual_seed(seed(case))
        hidden, k, n_mix = case.arch
        flow = [tuple(t * case.scale for t in lw) for lw in R.default_flow(case.nl, gen, hidden=hidden, k=k, n_mix=n_mix)]
        x = pin_links((torch.rand(case.B, 2, case.L, case.L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi)
        g = torch.randn(case.B, 2, case.L, case.L, generator=gen, dtype=torch.float64)
        gS = torch.randn(case.B, generator=gen, dtype=torch.float64)
        glogdet = torch.randn(case.B, generator=gen, dtype=torch.float64)
        _INPUTS[case.name] = Inputs(flow, x, g, gS, glogdet, case.act + ('+tanh' if case.tanh else ''))
    return _INPUTS[case.name]


def first_order(case):
    """first_order_cases.oracle_results at the inputs of a case, computed once and never modified"""
    if case.name not in _FIRST:
        _FIRST[case.name] = first_order_results(inputs(case))
    return _FIRST[case.name]


def second_order(case):
    """second_order_cases.oracle_results at the inputs of a case, computed once and never modified"""
    if case.name not in _SECOND:
        _SECOND[case.name] = second_order_results(inputs(case))
    return _SECOND[case.name]


def eight_layers(inp):
    """the inputs with eight layers, layer li carrying the weights of layer li % layers: one layer at every (mu, off)"""
    return inp._replace(flow=[inp.flow[li % len(inp.flow)] for li in range(8)])


def layers_at_every_stripe(case):
    """first_order_cases.layer_vjp of every layer li < 8 at layer_mu_off(li), keyed like first_order_cases.oracle_results
    (layer_y, layer_logJ [B, 8], layer_gx, layer_gw); computed once and never modified"""
    if case.name not in _LAYERS:
        inp8 = eight_layers(inputs(case))
        rows = [layer_vjp(inp8, li) for li in range(8)]
        _LAYERS[case.name] = {'layer_y': [r[0] for r in rows], 'layer_logJ': torch.stack([r[1] for r in rows], 1),
                              'layer_gx': [r[2] for r in rows], 'layer_gw': [r[3] for r in rows]}
    return _LAYERS[case.name]


def sensitivities(case, seed0):
    """(first order, second order): first_order_cases.sensitivity and second_order_cases.sensitivity at the case"""
    inp = inputs(case)
    return FC.sensitivity(inp, first_order(case), seed0), C.sensitivity(inp, second_order(case), seed0 + 5)
