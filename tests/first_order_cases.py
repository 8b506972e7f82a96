"""Hard inputs for the first-order flow sweeps (fthmc_flow_forward, fthmc_ft_action, fthmc_ft_force, fthmc_ft_leapfrog,
fthmc_train_grad, fthmc_flow_layer_bwd) and the measures they are held to: shared by tests/test_first_order_hard.py (CPU: the
oracle's own conditioning at these inputs, the fixture) and tests/test_first_order_hard_gpu.py (the kernels).  A plain module.

Cases, measure, bound and the rule that admits a case are those of tests/second_order_cases.py, imported from there and not
copied: scaled-up weights, links pinned 1e-9 from +-pi, max|got - ref| / max|ref| <= BOUND = 1e-9 for every layer's every parameter
tensor and for every chain on its own, admissible where the oracle itself moves by at most SENS_BOUND = 1e-12 under a move of
every input by one relative 2^-52.  A case that misses the condition gets a smaller scale or fewer layers, never a looser bound.

Every case of second_order_cases.CASES is a case here, with the same inputs (one set of hard inputs serves both orders).  FIRST_ONLY
adds the lattice kinds that the tuned first-order kernels distinguish and the dual kernels do not; they are built like
second_order_cases.inputs, with the seed 61000 + 100 L + 10 layers + index."""
import math

import numpy as np
import torch

import second_order_cases as C
import walk_model as W
from conftest import golden_flow, load_golden
from oracle import ref_cpu as R
from second_order_cases import (BETA, BOUND, NUDGES, SENS_BOUND, Case, Inputs, hold, nudged, per_chain,  # noqa: F401
                                per_tensor, pin_links, split, tensor_spread, worst)

DT = 0.05                       # the one flowed leapfrog step of oracle_results

FIRST_ONLY = [
    Case('L4_silu', 4, 3, 8, 2.0, 'silu', None, False),          # the smallest lattice: every window wraps several times; tiled kernels
    Case('L20_silu', 20, 2, 4, 3.0, 'silu', None, False),        # ragged 16 + 4 tiles, the slow-wrap instance (L < 24)
    Case('L28_leaky', 28, 1, 3, 3.0, 'leaky_relu', None, False),  # ragged 16 + 12, fast wrap
    Case('L36_relu', 36, 1, 2, 3.0, 'relu', None, False),        # two whole tiles and a 4-wide edge
    Case('L40_silu', 40, 1, 3, 3.0, 'silu', None, False),        # two whole tiles and an 8-wide edge
    Case('L64_silu', 64, 1, 2, 3.0, 'silu', None, False),        # 16 tiles per chain on the fused training backward
    Case('L32_relu', 32, 2, 8, 2.0, 'relu', None, False),        # every (mu, off) on the exact-tile instances, run-time activation
]
CASES = list(C.CASES) + FIRST_ONLY
BY_NAME = {c.name: c for c in CASES}
IDS = [c.name for c in CASES]

_INPUTS, _ORACLE = {}, {}


def inputs(case):
    """the inputs of a case, made once and never modified: second_order_cases.inputs for its cases, built alike for the others"""
    if case in C.CASES:
        return C.inputs(case)
    if case.name not in _INPUTS:
        gen = torch.Generator().manual_seed(61000 + 100 * case.L + 10 * case.nl + FIRST_ONLY.index(case))
        assert case.arch is None and not case.tanh
        flow = [tuple(t * case.scale for t in lw) for lw in R.default_flow(case.nl, gen)]
        x = pin_links((torch.rand(case.B, 2, case.L, case.L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi)
        g = torch.randn(case.B, 2, case.L, case.L, generator=gen, dtype=torch.float64)
        gS = torch.randn(case.B, generator=gen, dtype=torch.float64)
        glogdet = torch.randn(case.B, generator=gen, dtype=torch.float64)
        _INPUTS[case.name] = Inputs(flow, x, g, gS, glogdet, case.act)
    return _INPUTS[case.name]


def layer_vjp(inp, li):
    """one layer on its own at the case's links: (y, logJ, gx, gw) with gx, gw the autograd of (y c).sum() + (logJ dlog).sum()
    through oracle.ref_cpu.layer_forward, c = inp.g, dlog = inp.gS"""
    mu, off = R.layer_mu_off(li)
    xg = inp.x.detach().clone().requires_grad_(True)
    wl = tuple(t.detach().clone().requires_grad_(True) for t in inp.flow[li])
    y, logJ = R.layer_forward(xg, wl, mu, off, inp.act)
    g = torch.autograd.grad((y * inp.g).sum() + (logJ * inp.gS).sum(), [xg] + list(wl))
    return y.detach(), logJ.detach(), g[0], tuple(g[1:])


def oracle_results(inp, beta=BETA):
    """The CPU oracle's first-order quantities, detached fp64 (inp.act carries the '+tanh' of a final tanh through to
    oracle.ref_cpu.conv_net, as second_order_cases.oracle_results hands it on):
        y, logdet, S_eff:    flow_forward, ft_action                                  (fthmc_flow_forward, fthmc_ft_action)
        F:                   ft_force                                                 (fthmc_ft_force)
        logq, logp, gw:      train_grads; gw as per-layer tuples                      (fthmc_train_grad)
        layer_y, layer_gx, layer_gw:  per layer li at layer_mu_off(li), see layer_vjp    (fthmc_flow_layer_fwd / _bwd)
        layer_logJ [B, layers]:  the layers' log J side by side, a field per chain: one layer's log J alone is a sum that may
                             cancel (0.005 from terms of order 1 in L8_silu, layer 6), which no relative measure can hold
        lf_x, lf_v:          one flowed leapfrog step from (x, v = inp.g), dt = DT, nstep = 1: x' = x + dt/2 v, v' = v - dt F(x'),
                             x'' = x' + dt/2 v'                                       (fthmc_ft_leapfrog)"""
    with torch.no_grad():
        y, logdet = R.flow_forward(inp.x, inp.flow, inp.act)
        S = R.ft_action(inp.x, inp.flow, beta, inp.act)
    out, grads = R.train_grads(inp.x, inp.flow, beta, inp.act)
    lf_x, lf_v = R.leapfrog(inp.x, inp.g, lambda z: R.ft_force(z, inp.flow, beta, inp.act), DT, 1)
    layers = [layer_vjp(inp, li) for li in range(len(inp.flow))]
    return {'y': y, 'logdet': logdet, 'S_eff': S, 'F': R.ft_force(inp.x, inp.flow, beta, inp.act).detach(),
            'logq': out['logq'].detach(), 'logp': out['logp'].detach(), 'gw': [tuple(g.detach() for g in lg) for lg in grads],
            'layer_y': [l[0] for l in layers], 'layer_logJ': torch.stack([l[1] for l in layers], 1),
            'layer_gx': [l[2] for l in layers], 'layer_gw': [l[3] for l in layers],
            'lf_x': lf_x.detach(), 'lf_v': lf_v.detach()}


def oracle(case):
    """oracle_results at the inputs of a case, computed once and never modified"""
    if case.name not in _ORACLE:
        _ORACLE[case.name] = oracle_results(inputs(case))
    return _ORACLE[case.name]


ANGLES = ('y', 'lf_x', 'layer_y')           # links: compared as an angle difference


def _cpu(t):
    return torch.as_tensor(t).detach().double().cpu()


def per_chain_angle(got, ref, what):
    """per_chain of links that are equal where they differ by a multiple of 2 pi: max|wrap(got - ref)| / max|ref| per chain (the
    wrapped difference is put back onto ref, which rounds it to an ulp of ref: 1e-16 of max|ref|)"""
    got, ref = _cpu(got), _cpu(ref)
    return per_chain(ref + R.wrap(got - ref), ref, what)


def compare(got, ref, flow):
    """every output of `got`, by the measure of second_order_cases: weight gradients (flat or per-layer tuples) per tensor, fields
    and per-chain vectors per chain, links as angle differences; the per-layer lists entry by entry (None: not computed)"""
    errs = {}
    for key, val in got.items():
        if key == 'gw':
            errs.update(per_tensor(val if isinstance(val, list) else split(val, flow), ref[key], key))
        elif key == 'layer_gw':
            rows = [v if isinstance(v, tuple) else split(v, [flow[li]])[0] for li, v in enumerate(val)]
            errs.update(per_tensor(rows, ref[key], key))
        elif key == 'layer_logJ':
            val = torch.stack([_cpu(v) for v in val], 1) if isinstance(val, list) else val
            errs.update(per_chain(val, ref[key], key))
        elif key.startswith('layer_'):
            assert len(val) == len(ref[key])
            for li, (a, b) in enumerate(zip(val, ref[key])):
                errs.update((per_chain_angle if key in ANGLES else per_chain)(a, b, f'{key} {li}'))
        else:
            errs.update((per_chain_angle if key in ANGLES else per_chain)(val, ref[key], key))
    return errs


def sensitivity(inp, ref, seed):
    """the measure of every output between the oracle at `inp` (= ref) and at NUDGES nudged copies: the worst per entry"""
    errs = {}
    for n in range(NUDGES):
        for key, e in compare(oracle_results(nudged(inp, seed + n)), ref, inp.flow).items():
            errs[key] = max(errs.get(key, 0.0), e) if e == e else e
    return errs


def steep_fixture():
    """(fixture, Inputs, reference results keyed like first_order_cases.oracle_results) of tests/golden/first_order_steep_L8.npz"""
    g = load_golden('first_order_steep_L8')
    nl = int(g['n_layers'])
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    x = t(g['x'])
    z = torch.zeros(x.shape[0], dtype=torch.float64)
    inp = Inputs(golden_flow(g), x, torch.zeros_like(x), z, z, str(g['act']))
    ref = {'F': t(g['F']), 'S_eff': t(g['S_eff']), 'logq': t(g['logq']), 'logp': t(g['logp']),
           'gw': [tuple(t(g[f'gw{li}_{pi}']) for pi in range(6)) for li in range(nl)]}
    return g, inp, ref


# ---------------------------------------------------------------- which kernels serve a case under a setting of the switches
SETTINGS = {'mfma': (1, True), 'mfma-tiled': (1, False), 'valu': (0, True)}


def default_net(case):
    return case.arch is None and not case.tanh


def train_path(case, setting):
    """the kernels behind ops.train_grad's weight gradients for a case under a setting"""
    if not default_net(case):
        return 'generic'
    if setting == 'valu':
        return 'valu'
    if setting == 'mfma':
        return W.train_launch(case.B, case.L, case.nl)[0]
    assert W.ft_small_shape(case.L, case.nl) and not W.flow_bwd_train_shape(case.L)
    return 'two-kernel'
