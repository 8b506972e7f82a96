"""`torch.ops.fthmc_hip.*`: the torch operator boundary of SURVEY.md §8(b), level 2.

Every operator is a thin dispatcher entry over the C ABI (include/fthmc_hip.h):
inputs are contiguous fp64 tensors on the HIP device, outputs are allocated by torch, the launch
goes to the current HIP stream and nothing synchronises.  Only the device dispatch key is
registered: a CPU tensor raises NotImplementedError from the dispatcher (there is no CPU fallback).
The differentiable operators carry autograd formulas that call the hand-written backward kernels,
so `loss.backward()` through `torch.ops.fthmc_hip.flow_layer_fwd` never builds an ATen graph.

Two registrations of the same schemas (`BACKEND` says which one this process uses).  The schema text of an operator stands once
per side -- in csrc/torch_library.cpp's operator list and in the table `OPS` below -- and the Python registration is made from
that text (custom_op(schema=...)), not inferred from annotations; tests/test_torch_boundary.py holds the two lists and both
processes' `str(op._schema)` to each other:
  'compiled': `libfthmc_torch.so` -- a compiled TORCH_LIBRARY(fthmc_hip) (csrc/torch_library.cpp, built by csrc/Makefile next to
              libfthmc_hip.so): definitions and device implementations in C++, straight onto the C ABI; this module attaches
              the shape functions for tracing and the autograd formulas to them.  Used whenever the library is there.
  'python'  : the same operators defined with torch.library.custom_op over `ops` (ctypes), when the compiled library has not
              been built (or FTHMC_TORCH_OPS=python asks for it: the two are tested against each other).

Operators (reference call site each one replaces):
  wilson_action_charge(x, beta) -> (S, Q, plaq)      qed_helpers.py:94-116,177-186
  wilson_force(x, beta) -> F                         qed_helpers.py:265-272
  wilson_loops(x, Rmax, Tmax) -> W[B, Rmax, Tmax]    rectangular Wilson loops / Polyakov-loop correlators (ops.wilson_loops; no
                   reference counterpart).  NOT differentiable: no autograd formula is registered (a backward through such an
                   operator raises under the Python registration; under the compiled one torch's fallback only warns)
  hmc_trajectory(x, v, u, beta, dt, nstep) -> (x_new, dH, acc)          qed_helpers.py:275-311
  flow_layer_fwd(x, w, mu, off, n_mix, act, hidden=None, kernel_size=3) -> (y, logJ)      layers.py:196-202,348-371
  flow_layer_bwd_x(x, gy, glogJ, w, mu, off, n_mix, act, hidden, kernel_size) -> gx        (autograd of the above)
  flow_layer_bwd_w(x, gy, glogJ, w, mu, off, n_mix, act, hidden, kernel_size) -> gw[params]
  flow_layer_rev(y, w, mu, off, n_mix, act, tol, hidden, kernel_size) -> (x, logJ)         layers.py:204-210,294-320,373-396
  ft_action_force(x, w_all, n_layers, beta, act, n_mix=2, hidden, kernel_size) -> (S_eff, logdet, F)  qed_helpers.py:212-242
  fthmc_trajectory(x, v, u, w_all, n_layers, beta, dt, nstep, mode, act, n_mix=2, hidden, kernel_size)
                   -> (x_new, dH, acc, plaq, Q)                        ft_hmc.py:180-224 / ipynb/ft_hmc.py:394-435
  train_grad(xi, w_all, n_layers, beta, act, n_mix=2, hidden, kernel_size) -> (x, logq, logp, gw)     train.py:162-228
  ft_action_vjp(x, w_all, n_layers, beta, act, gS, glogdet=None, n_mix=2, hidden, kernel_size) -> (gx, gw)
                   d/dx, d/dw of sum_b gS_b S_eff_b + glogdet_b logdet_b        (autograd of qed_helpers.py:212-223)
  ft_force_vjp(x, w_all, n_layers, beta, act, g, n_mix=2, hidden, kernel_size) -> (gx, gw)
                   H g and d/dw <g, F> for the force F                         (autograd of qed_helpers.py:226-242, create_graph)
  train_force_grad(x, w_all, n_layers, beta, act, n_mix=2, hidden, kernel_size) -> (F, force_sq, gw)
                   the force, sum_links F_b^2 and d(sum_b |F_b|^2)/dw          ipynb/ft_hmc.py:253-299 (with_force)
  ft_trajectory_pb(x, v, u, w_all, n_layers, beta_b, dt, nstep, integrator, act, state_in=None, n_mix=2, hidden, kernel_size)
                   -> (x_new, dH, acc, plaq, Q, state)   per-chain beta (replica exchange; no reference counterpart): state is the
                   beta-free triple [3, B] = (log det J, sum cos P, Q); integrator 0 leapfrog, 1 omelyan, 2 force_gradient
  hmc_trajectory_pb(x, v, u, beta_b, dt, nstep, integrator=0) -> (x_new, dH, acc)          plain HMC, per-chain beta
  replica_swap(betas, C, u, beta_b!, rung!, chain_of!, parity) -> (swap_acc, d)            one exchange round; updates beta_b,
                   rung, chain_of in place (ops.replica_swap)
  local_update(x, beta, beta_b, seeds, n_hb=1, n_or=0, nsweep=1, sweep0=0, classes=15) -> x_new   heatbath / overrelaxation sweeps
                   of the plain Wilson action (ops.local_update; no reference counterpart); beta_b: per-chain beta or None; seeds:
                   int64 [B], None with n_hb = 0.  NOT differentiable
  instanton_hit(x, beta, beta_b, seeds, n_hit=1, hit0=0) -> (x_new, k, nacc)                  instanton hits of the plain Wilson
                   action, the Metropolis update across topological sectors (ops.instanton_hit; no reference counterpart); k, nacc:
                   int32 [B]; beta_b: per-chain beta or None; seeds: int64 [B], None with n_hit = 0.  NOT differentiable
`act` is the integer code of fthmc_hip.h (0 silu/swish, 1 relu, 2 leaky_relu); `mode` 0 = MD
semantics, 1 = literal reference leapfrog.  The s/t net's shape travels IN the schema, as plain
integers: `n_mix` mixture components, `hidden` = hidden_sizes (None = the reference default [8, 8]), `kernel_size` --
the C ABI's fthmc_arch_t of the call; a weight tensor is a plain tensor here and carries no shape of its own.
"""
import os
from typing import Callable, NamedTuple

import torch

from . import _lib, ops
from ._lib import FthmcError

_COMPILED_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'libfthmc_torch.so')
BACKEND = 'compiled' if os.path.exists(_COMPILED_PATH) and os.environ.get('FTHMC_TORCH_OPS', '') != 'python' else 'python'
if BACKEND == 'compiled':
    _lib.load()                                  # libfthmc_hip.so first: the compiled operators link against that same object
    torch.ops.load_library(_COMPILED_PATH)

_ACT = {0: 'silu', 1: 'relu', 2: 'leaky_relu'}
_MODE = {0: 'md', 1: 'literal'}
_DEV = 'cuda'       # ROCm devices live under torch's "cuda" device type / dispatch key


def _act(code: int) -> str:
    if code not in _ACT:
        raise FthmcError(f'act: unknown activation code {code}')
    return _ACT[code]


def _arch(n_mix: int, hidden, kernel_size: int):
    """(hidden_sizes, kernel_size, n_mix) of a call from the schema's integers (a net that ends in a tanh -- never built by the
    reference -- is served through `ops` with `arch=(hidden, k, n_mix, True)`, not through these schemas)"""
    return (tuple(int(h) for h in hidden) if hidden is not None else (8, 8), int(kernel_size), int(n_mix))


_INT = {v: k for k, v in _lib.INTEGRATORS.items()}


def _integrator(code: int) -> str:
    if code not in _INT:
        raise FthmcError(f'integrator: expected 0, 1 or 2, got {code}')
    return _INT[code]


# ---------------------------------------------------------------- the Python backend's implementations, over `ops`
def _local_update(x, beta, beta_b, seeds, n_hb=1, n_or=0, nsweep=1, sweep0=0, classes=15):
    return ops.local_update(x, beta if beta_b is None else beta_b, seeds, n_hb, n_or, nsweep, sweep0, classes)


def _instanton_hit(x, beta, beta_b, seeds, n_hit=1, hit0=0):
    return ops.instanton_hit(x, beta if beta_b is None else beta_b, seeds, n_hit, hit0)


def _hmc_trajectory(x, v, u, beta, dt, nstep):
    r = ops.hmc_trajectory(x, v, u, beta, dt, nstep)
    return r['x_new'], r['dH'], r['acc']


def _flow_layer_fwd(x, w, mu, off, n_mix, act, hidden=None, kernel_size=3):
    return ops.flow_layer_fwd(x, w, mu, off, _act(act), arch=_arch(n_mix, hidden, kernel_size))


def _layer_bwd(need_gw, pick):
    """the three backward schemas over ops.flow_layer_bwd: `pick` chooses what one of them returns from (gx, gw)"""
    def impl(x, gy, glogJ, w, mu, off, n_mix, act, hidden=None, kernel_size=3):
        gx, gw = ops.flow_layer_bwd(x, w, gy, glogJ, mu, off, _act(act), need_gw=need_gw, arch=_arch(n_mix, hidden, kernel_size))
        return pick(gx, gw)
    return impl


def _flow_layer_rev(y, w, mu, off, n_mix, act, tol, hidden=None, kernel_size=3):
    return ops.flow_layer_rev(y, w, mu, off, _act(act), tol, arch=_arch(n_mix, hidden, kernel_size))


def _ft_action_force(x, w_all, n_layers, beta, act, n_mix=2, hidden=None, kernel_size=3):
    a = _arch(n_mix, hidden, kernel_size)
    S, logdet, _, _ = ops.ft_action(x, w_all, n_layers, beta, _act(act), arch=a)
    return S, logdet, ops.ft_force(x, w_all, n_layers, beta, _act(act), arch=a)


def _fthmc_trajectory(x, v, u, w_all, n_layers, beta, dt, nstep, mode, act, n_mix=2, hidden=None, kernel_size=3):
    if mode not in _MODE:
        raise FthmcError(f'mode: expected 0 (md) or 1 (literal), got {mode}')
    r = ops.ft_trajectory(x, v, u, w_all, n_layers, beta, dt, nstep, _act(act), _MODE[mode], arch=_arch(n_mix, hidden, kernel_size))
    return r['x_new'], r['dH'], r['acc'], r['plaq'], r['Q']


def _train_grad(xi, w_all, n_layers, beta, act, n_mix=2, hidden=None, kernel_size=3):
    r = ops.train_grad(xi, w_all, n_layers, beta, _act(act), arch=_arch(n_mix, hidden, kernel_size))
    return r['x'], r['logq'], r['logp'], r['gw']


def _ft_action_vjp(x, w_all, n_layers, beta, act, gS, glogdet=None, n_mix=2, hidden=None, kernel_size=3):
    gx, gw = ops.ft_action_vjp(x, w_all, n_layers, beta, gS, glogdet, _act(act), arch=_arch(n_mix, hidden, kernel_size))
    return gx, gw


def _ft_force_vjp(x, w_all, n_layers, beta, act, g, n_mix=2, hidden=None, kernel_size=3):
    gx, gw = ops.ft_force_vjp(x, w_all, n_layers, beta, g, _act(act), arch=_arch(n_mix, hidden, kernel_size))
    return gx, gw


def _train_force_grad(x, w_all, n_layers, beta, act, n_mix=2, hidden=None, kernel_size=3):
    r = ops.train_force_grad(x, w_all, n_layers, beta, _act(act), arch=_arch(n_mix, hidden, kernel_size))
    gw = r['gw'] if r['gw'] is not None else x.new_zeros(w_all.numel())
    return r['F'], r['force_sq'], gw


def _ft_trajectory_pb(x, v, u, w_all, n_layers, beta_b, dt, nstep, integrator, act, state_in=None, n_mix=2, hidden=None, kernel_size=3):
    r = ops.ft_trajectory(x, v, u, w_all, n_layers, beta_b.contiguous(), dt, nstep, _act(act), 'md', state_in=state_in,
                          arch=_arch(n_mix, hidden, kernel_size), integrator=_integrator(integrator))
    return r['x_new'], r['dH'], r['acc'], r['plaq'], r['Q'], r['state']


def _hmc_trajectory_pb(x, v, u, beta_b, dt, nstep, integrator=0):
    r = ops.hmc_trajectory(x, v, u, beta_b.contiguous(), dt, nstep, integrator=_integrator(integrator))
    return r['x_new'], r['dH'], r['acc']


def _replica_swap(betas, C, u, beta_b, rung, chain_of, parity):
    r = ops.replica_swap(betas, C, u, beta_b, rung, chain_of, parity)
    return r['swap_acc'], r['d']


# ---------------------------------------------------------------- the operator table
class _Op(NamedTuple):
    name: str
    schema: str                 # '(arguments) -> returns': character for character the text of csrc/torch_library.cpp's list
    fake: Callable              # the outputs' shapes from the call's arguments (tracing, meta tensors)
    impl: Callable              # the Python backend's implementation
    mutates: tuple = ()         # the arguments updated in place (the schema's alias annotations say the same)


_like = torch.empty_like


def _b(x):
    return x.new_empty(x.shape[0])


def _gw(x, w):
    return x.new_empty(w.numel())


def _swap_shape(betas, beta_b):
    return beta_b.new_empty(beta_b.numel() // betas.numel(), betas.numel() - 1)


OPS = (
    _Op('wilson_action_charge', '(Tensor x, float beta) -> (Tensor, Tensor, Tensor)',
        lambda x, *_: (_b(x), _b(x), _b(x)), ops.wilson_action_charge),
    _Op('wilson_force', '(Tensor x, float beta) -> Tensor',
        lambda x, *_: _like(x), ops.wilson_force),
    _Op('hmc_trajectory', '(Tensor x, Tensor v, Tensor u, float beta, float dt, int nstep) -> (Tensor, Tensor, Tensor)',
        lambda x, *_: (_like(x), _b(x), _b(x)), _hmc_trajectory),
    _Op('flow_layer_fwd', '(Tensor x, Tensor w, int mu, int off, int n_mix, int act, int[]? hidden=None, int kernel_size=3) -> (Tensor, Tensor)',
        lambda x, *_: (_like(x), _b(x)), _flow_layer_fwd),
    _Op('flow_layer_bwd_x', '(Tensor x, Tensor gy, Tensor glogJ, Tensor w, int mu, int off, int n_mix, int act, int[]? hidden=None, '
        'int kernel_size=3) -> Tensor',
        lambda x, *_: _like(x), _layer_bwd(False, lambda gx, gw: gx)),
    _Op('flow_layer_bwd_w', '(Tensor x, Tensor gy, Tensor glogJ, Tensor w, int mu, int off, int n_mix, int act, int[]? hidden=None, '
        'int kernel_size=3) -> Tensor',
        lambda x, gy, glogJ, w, *_: _gw(x, w), _layer_bwd(True, lambda gx, gw: gw)),
    # both gradients from one launch (what the autograd formula of flow_layer_fwd uses)
    _Op('flow_layer_bwd', '(Tensor x, Tensor gy, Tensor glogJ, Tensor w, int mu, int off, int n_mix, int act, int[]? hidden=None, '
        'int kernel_size=3) -> (Tensor, Tensor)',
        lambda x, gy, glogJ, w, *_: (_like(x), _gw(x, w)), _layer_bwd(True, lambda gx, gw: (gx, gw))),
    _Op('flow_layer_rev', '(Tensor y, Tensor w, int mu, int off, int n_mix, int act, float tol, int[]? hidden=None, int kernel_size=3) '
        '-> (Tensor, Tensor)',
        lambda y, *_: (_like(y), _b(y)), _flow_layer_rev),
    _Op('ft_action_force', '(Tensor x, Tensor w_all, int n_layers, float beta, int act, int n_mix=2, int[]? hidden=None, int kernel_size=3) '
        '-> (Tensor, Tensor, Tensor)',
        lambda x, *_: (_b(x), _b(x), _like(x)), _ft_action_force),
    _Op('fthmc_trajectory', '(Tensor x, Tensor v, Tensor u, Tensor w_all, int n_layers, float beta, float dt, int nstep, int mode, int act, '
        'int n_mix=2, int[]? hidden=None, int kernel_size=3) -> (Tensor, Tensor, Tensor, Tensor, Tensor)',
        lambda x, *_: (_like(x), _b(x), _b(x), _b(x), _b(x)), _fthmc_trajectory),
    _Op('train_grad', '(Tensor xi, Tensor w_all, int n_layers, float beta, int act, int n_mix=2, int[]? hidden=None, int kernel_size=3) '
        '-> (Tensor, Tensor, Tensor, Tensor)',
        lambda xi, w_all, *_: (_like(xi), _b(xi), _b(xi), _gw(xi, w_all)), _train_grad),
    _Op('ft_action_vjp', '(Tensor x, Tensor w_all, int n_layers, float beta, int act, Tensor gS, Tensor? glogdet=None, int n_mix=2, '
        'int[]? hidden=None, int kernel_size=3) -> (Tensor, Tensor)',
        lambda x, w_all, *_: (_like(x), _gw(x, w_all)), _ft_action_vjp),
    _Op('ft_force_vjp', '(Tensor x, Tensor w_all, int n_layers, float beta, int act, Tensor g, int n_mix=2, int[]? hidden=None, '
        'int kernel_size=3) -> (Tensor, Tensor)',
        lambda x, w_all, *_: (_like(x), _gw(x, w_all)), _ft_force_vjp),
    _Op('train_force_grad', '(Tensor x, Tensor w_all, int n_layers, float beta, int act, int n_mix=2, int[]? hidden=None, int kernel_size=3) '
        '-> (Tensor, Tensor, Tensor)',
        lambda x, w_all, *_: (_like(x), _b(x), _gw(x, w_all)), _train_force_grad),
    _Op('ft_trajectory_pb', '(Tensor x, Tensor v, Tensor u, Tensor w_all, int n_layers, Tensor beta_b, float dt, int nstep, int integrator, '
        'int act, Tensor? state_in=None, int n_mix=2, int[]? hidden=None, int kernel_size=3) '
        '-> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)',
        lambda x, *_: (_like(x), _b(x), _b(x), _b(x), _b(x), x.new_empty(3, x.shape[0])), _ft_trajectory_pb),
    _Op('hmc_trajectory_pb', '(Tensor x, Tensor v, Tensor u, Tensor beta_b, float dt, int nstep, int integrator=0) -> (Tensor, Tensor, Tensor)',
        lambda x, *_: (_like(x), _b(x), _b(x)), _hmc_trajectory_pb),
    _Op('replica_swap', '(Tensor betas, Tensor C, Tensor u, Tensor(a!) beta_b, Tensor(b!) rung, Tensor(c!) chain_of, int parity) '
        '-> (Tensor, Tensor)',
        lambda betas, C, u, beta_b, *_: (_swap_shape(betas, beta_b), _swap_shape(betas, beta_b)), _replica_swap,
        mutates=('beta_b', 'rung', 'chain_of')),
    _Op('wilson_loops', '(Tensor x, int Rmax, int Tmax) -> Tensor',
        lambda x, Rmax, Tmax: x.new_empty(x.shape[0], Rmax, Tmax), ops.wilson_loops),
    _Op('local_update', '(Tensor x, float beta, Tensor? beta_b, Tensor? seeds, int n_hb=1, int n_or=0, int nsweep=1, int sweep0=0, '
        'int classes=15) -> Tensor',
        lambda x, *_: _like(x), _local_update),
    _Op('instanton_hit', '(Tensor x, float beta, Tensor? beta_b, Tensor? seeds, int n_hit=1, int hit0=0) -> (Tensor, Tensor, Tensor)',
        lambda x, *_: (_like(x), x.new_empty(x.shape[0], dtype=torch.int32), x.new_empty(x.shape[0], dtype=torch.int32)), _instanton_hit),
)

# the module's names are the dispatcher's operators themselves: the compiled library's, or defined here with its schema text
for _op in OPS:
    if BACKEND == 'python':
        globals()[_op.name] = torch.library.custom_op('fthmc_hip::' + _op.name, _op.impl, mutates_args=_op.mutates, device_types=_DEV,
                                                      schema=_op.schema)
    else:
        globals()[_op.name] = getattr(torch.ops.fthmc_hip, _op.name)
    torch.library.register_fake('fthmc_hip::' + _op.name, _op.fake)
__all__ = [_op.name for _op in OPS]


# ---------------------------------------------------------------- autograd formulas
def _wilson_setup(ctx, inputs, output):
    x, beta = inputs
    ctx.save_for_backward(x)
    ctx.beta = beta


def _wilson_backward(ctx, gS, gQ, gplaq):
    # S = -beta sum cos P; plaq = -S / (beta L^2); Q is piecewise constant (qed_helpers.py:108-116)
    (x,) = ctx.saved_tensors
    L = x.shape[-1]
    g = torch.zeros(x.shape[0], dtype=x.dtype, device=x.device)
    if gS is not None:
        g = g + gS
    if gplaq is not None:
        g = g - gplaq / (ctx.beta * L * L)
    return torch.ops.fthmc_hip.wilson_force(x, ctx.beta) * g.view(-1, 1, 1, 1), None


torch.library.register_autograd('fthmc_hip::wilson_action_charge', _wilson_backward, setup_context=_wilson_setup)


def _layer_setup(ctx, inputs, output):
    x, w, mu, off, n_mix, act, hidden, kernel_size = inputs
    ctx.save_for_backward(x, w)
    ctx.args = (mu, off, n_mix, act, hidden, kernel_size)


def _layer_backward(ctx, gy, glogJ):
    x, w = ctx.saved_tensors
    B = x.shape[0]
    gy = torch.zeros_like(x) if gy is None else gy.contiguous()
    glogJ = torch.zeros(B, dtype=x.dtype, device=x.device) if glogJ is None else glogJ.contiguous()
    if ctx.needs_input_grad[1]:
        gx, gw = torch.ops.fthmc_hip.flow_layer_bwd(x, gy, glogJ, w, *ctx.args)
        return gx, gw.view_as(w), None, None, None, None, None, None
    return torch.ops.fthmc_hip.flow_layer_bwd_x(x, gy, glogJ, w, *ctx.args), None, None, None, None, None, None, None


torch.library.register_autograd('fthmc_hip::flow_layer_fwd', _layer_backward, setup_context=_layer_setup)


def _action_force_setup(ctx, inputs, output):
    x, w_all, n_layers, beta, act, n_mix, hidden, kernel_size = inputs
    ctx.save_for_backward(x, w_all)
    ctx.args = (n_layers, beta, act)
    ctx.arch = (n_mix, hidden, kernel_size)


def _action_force_backward(ctx, gS, glogdet, gF):
    # S_eff and logdet: the action VJP; F: the force VJP (gx = H gF, gw = d/dw <gF, F>).  First order in this formula: the VJP
    # operators carry no autograd formula of their own
    x, w = ctx.saved_tensors
    gx, gw = torch.zeros_like(x), torch.zeros(w.numel(), dtype=x.dtype, device=x.device)
    if gS is not None or glogdet is not None:
        gS_ = gS.contiguous() if gS is not None else torch.zeros(x.shape[0], dtype=x.dtype, device=x.device)
        gld = glogdet.contiguous() if glogdet is not None else None
        a, b = torch.ops.fthmc_hip.ft_action_vjp(x, w, *ctx.args, gS_, gld, *ctx.arch)
        gx, gw = gx + a, gw + b
    if gF is not None:
        a, b = torch.ops.fthmc_hip.ft_force_vjp(x, w, *ctx.args, gF.contiguous(), *ctx.arch)
        gx, gw = gx + a, gw + b
    return gx, gw.view_as(w), None, None, None, None, None, None


torch.library.register_autograd('fthmc_hip::ft_action_force', _action_force_backward, setup_context=_action_force_setup)
