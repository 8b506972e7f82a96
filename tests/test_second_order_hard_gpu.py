"""GPU: the three second-order sweeps on the hard cases of tests/second_order_cases.py, tensor by tensor.

ops.ft_force_vjp (H g, d/dw <g, F>), ops.ft_action_vjp (d/dx, d/dw of sum gS S_eff + glogdet logdet) and ops.train_force_grad
(F, sum F^2, d/dw sum |F|^2) under every setting of the dual-path switch that serves the shape -- 0: the plain dual sweep
(csrc/flow_generic.hip on Dual), 2: the fused kernels of csrc/flow_dual.hip on 8 x 8 tiles, 3: on 8 x 16 tiles where they divide L,
1: the default -- against the oracle's double backward, with scaled-up weights and links pinned 1e-9 from +-pi.  Before each call
ops.train_force_path asserts which path serves it: a silent fallback cannot pass.  Measure and bound (second_order_cases.py):
max|got - ref| / max|ref| <= 1e-9 for every layer's every parameter tensor and for every chain of a field output, where
tests/test_second_order_gpu.py and tests/test_force_training_gpu.py take one norm over the concatenation of everything;
tests/test_second_order_hard.py asserts on the CPU that the oracle itself moves by at most 1e-12 per tensor at these inputs.  The
last test holds the same entry points to tests/golden/second_order_steep_L8.npz, the reference's own autograd on the L = 8, 8-layer,
scale-3 case.

Observed on an MI355X (pytest -s prints them): the worst per-tensor / per-chain error of each case, next to the reference's
sensitivity (the oracle under a move of every input by one relative 2^-52, the worst of three sets of signs):
  case        L  B layers scale  vjps     train_force_grad, path 0 / 2 / 3 / 1        fused vs plain, 2 / 3 / 1      sensitivity
  L8_silu     8  2    8    2.5   3.4e-14  2.3e-14 / 2.6e-14 / 2.6e-14 / 2.6e-14       3.0e-15 / 3.0e-15 / 3.0e-15    6.1e-14
  L16_silu   16  2    8      2   1.3e-14  7.3e-15 / 6.5e-15 / 6.6e-15 / 6.5e-15       8.6e-16 / 1.3e-15 / 8.6e-16    2.5e-14
  L16_relu   16  2    8      2   4.2e-14  2.7e-13 / 2.7e-13 / 2.7e-13 / 2.7e-13       2.2e-15 / 2.0e-15 / 2.2e-15    5.1e-13
  L16_leaky  16  2    8      2   2.7e-14  1.4e-14 / 1.5e-14 / 1.5e-14 / 1.5e-14       1.2e-15 / 1.1e-15 / 1.2e-15    7.8e-14
  L32_silu   32  1    4      3   3.2e-14  3.0e-14 / 2.9e-14 / 3.0e-14 / 2.9e-14       1.9e-15 / 1.8e-15 / 1.9e-15    1.0e-13
  L12_silu   12  2    4      3   4.0e-14  9.3e-14 / - / - / -                         - / - / -                      7.1e-13
  L24_leaky  24  1    3      3   5.0e-14  2.7e-14 / 2.7e-14 / 2.7e-14 / 2.7e-14       1.4e-15 / 1.4e-15 / 1.4e-15    1.5e-13
  L8_net      8  2    4      3   2.7e-14  2.7e-14 / - / - / -                         - / - / -                      2.2e-13
  L8_tanh     8  2    4      3   4.0e-14  8.6e-15 / - / - / -                         - / - / -                      1.4e-13
  steep reference fixture (L = 8, B = 2, 8 layers, scale 3), all entry points and paths 0 / 2 / 1: 9.5e-14 (gw_vjp layer 1 tensor 1);
  its sensitivity 2.5e-13, the oracle against it 8.1e-15.
The worst entry is a conv bias (tensor 1, 3 or 5) in most cases: the tensors the global norm hides.  "-": the fused kernels do
not serve the shape and the test asserts that.  Every figure is four orders or more inside the bound and at or below the
reference's own sensitivity.  With one defect each built into a copy of csrc/dual.h -- the tangent of operator/(double, Dual)
negated, silu'' zeroed in act_eval(Dual), the tangent of cs dropped in ft_sincos(Dual) -- 19, 13 (every silu case and the
fixture) and 19 of the 20 tests here fail, and tests/test_dual_math_gpu.py fails in the test of the overload concerned.
"""
import pytest
import torch

import second_order_cases as C
from gpu_support import D, module_defaults, ops, switches

pytestmark = pytest.mark.gpu
_defaults = module_defaults(dual=1)

IDS = [c.name for c in C.CASES]


def _arch(case):
    """the arch argument of ops.train_force_path / train_force_ws_bytes"""
    if case.arch is None:
        return ((8, 8), 3, 2, True) if case.tanh else None
    return case.arch + ((True,) if case.tanh else ())


def _fused(case):
    """whether the fused dual kernels serve a case: the default net without a final tanh on a lattice that 8 x 8 tiles divide"""
    return case.arch is None and not case.tanh and case.L % 8 == 0


def _weights(inp, tanh=False):
    return ops.pack_weights(inp.flow, device='cuda', final_tanh=tanh)


def _vjps(inp, w, beta=C.BETA, glogdet=True):
    nl = len(inp.flow)
    x = D(inp.x)
    hx, hw = ops.ft_force_vjp(x, w, nl, beta, D(inp.g), inp.act.replace('+tanh', ''))
    ax, aw = ops.ft_action_vjp(x, w, nl, beta, D(inp.gS), D(inp.glogdet) if glogdet else None, inp.act.replace('+tanh', ''))
    return {'Hg': hx, 'gw_vjp': hw, 'ax': ax, 'aw': aw}


def _force(inp, w, beta=C.BETA):
    r = ops.train_force_grad(D(inp.x), w, len(inp.flow), beta, inp.act.replace('+tanh', ''))
    return {'F': r['F'], 'force_sq': r['force_sq'], 'gw_force': r['gw']}


@pytest.mark.parametrize('case', C.CASES, ids=IDS)
def test_force_and_action_vjps_per_tensor(case):
    inp, ref = C.inputs(case), C.oracle(case)
    errs = C.compare(_vjps(inp, _weights(inp, case.tanh)), ref, inp.flow)
    print(f'{case.name} vjps: worst %.1e (%s)' % C.worst(errs)[::-1])
    C.hold(errs, C.BOUND, case.name)


@pytest.mark.parametrize('case', C.CASES, ids=IDS)
def test_train_force_grad_on_every_path_per_tensor(case):
    """every path that serves the shape against the oracle; fused against plain; plain against 2 ft_force_vjp(g = F)"""
    inp, ref = C.inputs(case), C.oracle(case)
    w = _weights(inp, case.tanh)
    arch, act, nl = _arch(case), case.act, case.nl
    with switches(dual=0):
        assert ops.train_force_path(case.B, case.L, arch) == 0
        plain = _force(inp, w)
        errs = C.compare(plain, ref, inp.flow)
        print(f'{case.name} path 0: worst %.1e (%s)' % C.worst(errs)[::-1])
        C.hold(errs, C.BOUND, f'{case.name} path 0')
        vjp = 2 * ops.ft_force_vjp(D(inp.x), w, nl, C.BETA, plain['F'], act, need_gx=False)[1]
    assert torch.equal(plain['gw_force'], vjp)                # the plain sweep IS the force VJP's, seeded with F, times two
    plain_rows = C.split(plain['gw_force'], inp.flow)
    wsb = {}
    for path in (2, 3, 1):
        with switches(dual=path):
            assert ops.train_force_path(case.B, case.L, arch) == int(_fused(case)), (case.name, path)
            if not _fused(case):
                continue
            wsb[path] = ops.train_force_ws_bytes(case.B, case.L, nl)
            on = _force(inp, w)
        assert torch.equal(on['F'], plain['F']) and torch.equal(on['force_sq'], plain['force_sq'])
        errs = C.compare(on, ref, inp.flow)
        vs_plain = C.per_tensor(C.split(on['gw_force'], inp.flow), plain_rows, 'fused vs plain')
        print(f'{case.name} path {path}: worst %.1e (%s)' % C.worst(errs)[::-1], '; fused vs plain %.1e (%s)' % C.worst(vs_plain)[::-1])
        C.hold(errs, C.BOUND, f'{case.name} path {path}')
        C.hold(vs_plain, C.BOUND, f'{case.name} path {path}')
    if _fused(case):
        # settings 2 and 3 run different tiles exactly where 8 x 16 tiles divide the lattice (their workspaces differ)
        assert (wsb[2] != wsb[3]) == (case.L % 16 == 0), wsb


def test_cases_reach_every_path():
    """the fused kernels on one wrapping tile, on wrapping 8 x 16 tiles with every (mu, off), side by side without wrap and on a
    lattice that is no power of two; the plain sweep for the lattice no tile divides and for the other nets"""
    fused = {c.name for c in C.CASES if _fused(c)}
    assert fused == {'L8_silu', 'L16_silu', 'L16_relu', 'L16_leaky', 'L32_silu', 'L24_leaky'}


def test_entry_points_match_the_steep_reference_fixture():
    """tests/golden/second_order_steep_L8.npz: the reference's own autograd at scale 3 on 8 layers with the pinned links; the
    fixture's action VJP has gS alone"""
    g, inp, ref = C.steep_fixture()
    beta = float(g['beta'])
    w = _weights(inp)
    errs = C.compare(_vjps(inp, w, beta, glogdet=False), ref, inp.flow)
    for path in (0, 2, 1):
        with switches(dual=path):
            assert ops.train_force_path(2, 8) == int(path != 0)
            e = C.compare(_force(inp, w, beta), ref, inp.flow)
        errs.update({f'{k} (path {path})': v for k, v in e.items()})
    print('steep fixture: worst %.1e (%s)' % C.worst(errs)[::-1])
    C.hold(errs, C.BOUND, 'steep fixture')
