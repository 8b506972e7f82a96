"""Hard inputs for the second-order sweeps (fthmc_ft_force_vjp, fthmc_ft_action_vjp, fthmc_train_force_grad) and the measures
they are held to: shared by tests/test_second_order_hard.py (CPU: the oracle's own conditioning at these inputs, the fixture) and
tests/test_second_order_hard_gpu.py (the kernels).  A plain module: cases, the oracle's double backward, measures.

Inputs of a case: oracle.ref_cpu.default_flow times `scale` (the sigmoids saturate, the transform's slopes get steep), links uniform
in (-pi, pi) with x[0, 0, 0, :] = pi - 1e-9 and x[0, 1, :, 0] = -pi + 1e-9 (plaquettes at the branch cut of the wrap and of
tan(P / 2), as tests/test_hip_parity.py test_activations_and_extremes_vs_oracle pins them), beta = 2, random normal g, gS, glogdet.

Measure: max|got - ref| / max|ref| for every layer's every parameter tensor on its own (weight gradients) and for every chain on
its own (field outputs), bound 1e-9 -- TOL of tests/test_force_training_gpu.py, which that file applies to the concatenation of all
tensors, where the smallest tensor's gradient is 7e-2 .. 1e-5 of the largest and an error of that relative size in it passes.

A case may be held to 1e-9 per tensor only where the reference itself is well-conditioned: the oracle's results at the inputs and
at a copy with every link and weight moved by one relative 2^-52 (seeded random sign) differ by at most SENS_BOUND = 1e-12 per
tensor, three orders below the bound -- room for the device's other summation order over L^2 sites and its few-ulp exp / sigmoid /
atan.  A case that misses the condition gets a smaller scale or fewer layers, never a looser bound (L = 16 with 8 layers at scale 3
is 4.5e-12 .. 2.5e-11 and every 8-layer flow at scale 4 is 1e-9: not usable; L = 8 with 8 layers at scale 3 moved by 2e-13 .. 4.7e-12
from one set of signs to the next and runs at scale 2.5, 3e-14 .. 1.2e-13 -- scale 3 on that shape is the reference fixture
tests/golden/second_order_steep_L8.npz, whose inputs were picked by this condition).  The condition is asserted for NUDGES sets of
signs."""
import collections
import math

import numpy as np
import torch

from conftest import golden_flow, load_golden
from oracle import ref_cpu as R

BOUND = 1e-9
SENS_BOUND = 1e-12
NUDGES = 3
BETA = 2.0

Case = collections.namedtuple('Case', 'name L B nl scale act arch tanh')
# arch: None = the default net (2 -> 8 -> 8 -> 3, k = 3: the tuned and the fused dual kernels), else (hidden, k, n_mix)
CASES = [
    Case('L8_silu', 8, 2, 8, 2.5, 'silu', None, False),               # one tile wrapping onto itself
    Case('L16_silu', 16, 2, 8, 2.0, 'silu', None, False),             # every (mu, off), 8 x 16 tiles wrapping
    Case('L16_relu', 16, 2, 8, 2.0, 'relu', None, False),
    Case('L16_leaky', 16, 2, 8, 2.0, 'leaky_relu', None, False),
    Case('L32_silu', 32, 1, 4, 3.0, 'silu', None, False),             # tiles side by side without wrap
    Case('L12_silu', 12, 2, 4, 3.0, 'silu', None, False),             # 8 x 8 tiles do not divide 12: the plain sweep
    Case('L24_leaky', 24, 1, 3, 3.0, 'leaky_relu', None, False),      # not a power of two
    Case('L8_net', 8, 2, 4, 3.0, 'silu', ((4, 6), 5, 3), False),      # another net shape: the plain sweep
    Case('L8_tanh', 8, 2, 4, 3.0, 'silu', None, True),                # a tanh behind the last conv: the plain sweep
]
BY_NAME = {c.name: c for c in CASES}

Inputs = collections.namedtuple('Inputs', 'flow x g gS glogdet act')
_INPUTS, _ORACLE = {}, {}


def pin_links(x):
    """plaquettes at the branch cut of the wrap / of tan(P / 2)"""
    x[0, 0, 0, :] = math.pi - 1e-9
    x[0, 1, :, 0] = -math.pi + 1e-9
    return x


def inputs(case):
    """the inputs of a case, made once and never modified"""
    if case.name not in _INPUTS:
        gen = torch.Generator().manual_seed(52000 + 100 * case.L + 10 * case.nl + CASES.index(case))
        kw = {} if case.arch is None else dict(hidden=case.arch[0], k=case.arch[1], n_mix=case.arch[2])
        flow = [tuple(t * case.scale for t in lw) for lw in R.default_flow(case.nl, gen, **kw)]
        x = pin_links((torch.rand(case.B, 2, case.L, case.L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi)
        g = torch.randn(case.B, 2, case.L, case.L, generator=gen, dtype=torch.float64)
        gS = torch.randn(case.B, generator=gen, dtype=torch.float64)
        glogdet = torch.randn(case.B, generator=gen, dtype=torch.float64)
        _INPUTS[case.name] = Inputs(flow, x, g, gS, glogdet, case.act + ('+tanh' if case.tanh else ''))
    return _INPUTS[case.name]


def nudged(inp, seed):
    """every link and every weight moved by one relative 2^-52, with a seeded random sign"""
    gen = torch.Generator().manual_seed(seed)

    def move(t):
        sign = torch.randint(0, 2, t.shape, generator=gen).to(torch.float64) * 2 - 1
        return t * (1 + sign * 2.0 ** -52)
    return inp._replace(flow=[tuple(move(t) for t in lw) for lw in inp.flow], x=move(inp.x))


def sensitivity(inp, ref, seed):
    """the measure of every output between the oracle at `inp` (= ref) and at NUDGES nudged copies: the worst per entry"""
    errs = {}
    for n in range(NUDGES):
        for key, e in compare(oracle_results(nudged(inp, seed + n)), ref, inp.flow).items():
            errs[key] = max(errs.get(key, 0.0), e) if e == e else e
    return errs


def oracle_results(inp, beta=BETA):
    """The CPU double backward of oracle.ref_cpu.ft_action:
        F, Hg, gw_vjp:  the force, H g and d/dw <g, F>                       (fthmc_ft_force_vjp)
        ax, aw:         d/dx, d/dw of sum_b gS S_eff + glogdet logdet        (fthmc_ft_action_vjp)
        force_sq, gw_force:  sum over the links of F_b^2, d/dw sum_b |F_b|^2  (fthmc_train_force_grad)
    weight gradients as lists of per-layer tuples shaped like the parameters"""
    fl = [tuple(t.detach().clone().requires_grad_(True) for t in lw) for lw in inp.flow]
    params = [t for lw in fl for t in lw]
    xg = inp.x.detach().clone().requires_grad_(True)
    F, = torch.autograd.grad(R.ft_action(xg, fl, beta, inp.act).sum(), xg, create_graph=True)
    f = torch.autograd.grad((F * inp.g).sum(), [xg] + params, retain_graph=True)
    q = torch.autograd.grad((F ** 2).sum(), params)
    y, logdet = R.flow_forward(xg, fl, inp.act)
    S = R.action(y, beta) - logdet
    a = torch.autograd.grad((inp.gS * S).sum() + (inp.glogdet * logdet).sum(), [xg] + params)
    n = len(fl[0])
    rows = lambda flat: [tuple(flat[li * n:(li + 1) * n]) for li in range(len(fl))]
    Fd = F.detach()
    return {'F': Fd, 'Hg': f[0], 'gw_vjp': rows(f[1:]), 'ax': a[0], 'aw': rows(a[1:]),
            'force_sq': (Fd ** 2).sum((1, 2, 3)), 'gw_force': rows(q)}


def oracle(case):
    """oracle_results at the inputs of a case, computed once and never modified"""
    if case.name not in _ORACLE:
        _ORACLE[case.name] = oracle_results(inputs(case))
    return _ORACLE[case.name]


def split(flat, flow):
    """a flat weight gradient [layers * params] in the canonical order -> per-layer tuples shaped like the parameters of `flow`"""
    flat = torch.as_tensor(flat).detach().double().cpu().reshape(len(flow), -1)
    out = []
    for li, lw in enumerate(flow):
        o, row = 0, []
        for t in lw:
            row.append(flat[li, o:o + t.numel()].reshape(t.shape))
            o += t.numel()
        assert o == flat.shape[1], (o, flat.shape)
        out.append(tuple(row))
    return out


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def per_tensor(got, ref, what='gw'):
    """{'<what> layer l tensor p': max|got - ref| / max|ref|} over every layer's every parameter tensor"""
    assert len(got) == len(ref) and all(len(a) == len(b) for a, b in zip(got, ref))
    return {f'{what} layer {li} tensor {pi}': _rel(a, b) for li, (ga, ra) in enumerate(zip(got, ref)) for pi, (a, b) in enumerate(zip(ga, ra))}


def per_chain(got, ref, what):
    """{'<what> chain b': max|got - ref| / max|ref|} over every chain of a field output"""
    got, ref = torch.as_tensor(got), torch.as_tensor(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return {f'{what} chain {b}': _rel(got[b], ref[b]) for b in range(ref.shape[0])}


def worst(errs):
    """(name, error) of the worst entry; a NaN is the worst of all"""
    return max(errs.items(), key=lambda kv: math.inf if kv[1] != kv[1] else kv[1])


def hold(errs, bound, label=''):
    """every entry within the bound; the failure names the worst tensor / chain"""
    name, e = worst(errs)
    assert e <= bound, f'{label}: worst {name}: {e:.3e} > {bound:.0e}'
    return e


def compare(got, ref, flow):
    """every output of `got` that `ref` has, by the measure above: weight gradients (flat or per-layer tuples) per tensor, fields
    and per-chain vectors per chain"""
    errs = {}
    for key, val in got.items():
        if key in ('gw_vjp', 'aw', 'gw_force'):
            rows = val if isinstance(val, list) else split(val, flow)
            errs.update(per_tensor(rows, ref[key], key))
        else:
            errs.update(per_chain(val, ref[key], key))
    return errs


def tensor_spread(rows):
    """smallest / largest max|.| over the parameter tensors of a weight gradient"""
    m = [float(t.abs().max()) for lw in rows for t in lw]
    return min(m) / max(m)


def steep_fixture():
    """(Inputs, reference results shaped like oracle_results) of tests/golden/second_order_steep_L8.npz; its action VJP carries gS
    alone (the reference's ft_action returns S_eff): glogdet = 0"""
    g = load_golden('second_order_steep_L8')
    nl = int(g['n_layers'])
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    inp = Inputs(golden_flow(g), t(g['x']), t(g['g']), t(g['gS']), torch.zeros(2, dtype=torch.float64), str(g['act']))
    rows = lambda key: [tuple(t(g[f'{key}{li}_{pi}']) for pi in range(6)) for li in range(nl)]
    ref = {'F': t(g['F']), 'Hg': t(g['Hg']), 'gw_vjp': rows('gw'), 'ax': t(g['ga_x']), 'aw': rows('ga_w'),
           'force_sq': t(g['force_sq']), 'gw_force': rows('gq')}
    return g, inp, ref
