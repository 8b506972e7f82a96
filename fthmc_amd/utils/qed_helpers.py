"""fthmc/utils/qed_helpers.py on the HIP kernels: plaquettes, Wilson action, topological
charge, plain force / leapfrog / HMC, flow drivers, ft_action, ft_force, and the notebook's
physical-field ftHMC wrapper (ipynb/ft_hmc.py:420-513: ft_hmc, ft_run, flow_resize)."""
from __future__ import annotations

import time
from dataclasses import dataclass
from math import pi as PI
from typing import Optional

import torch
import torch.nn as nn

from .. import ops
from torch.autograd.function import once_differentiable

from .layers import _flow_rows, flow_activation, flow_weights, weights_generation

TWO_PI = 2 * PI


def grab(var):
    return var.detach().cpu().numpy()


def regularize(f):
    """qed_helpers.py:40-42."""
    return ops.regularize(f)


def torch_mod(x):
    """qed_helpers.py:45-46: remainder(x, 2 pi) in [0, 2 pi) (not the flow's [-pi, pi) map)."""
    return torch.remainder(x, TWO_PI)


def torch_wrap(x):
    """qed_helpers.py:49-50: [-pi, pi)."""
    return ops.wrap(x)


def _batched(x):
    return x if x.dim() == 4 else x[None]


def compute_u1_plaq(links, mu=0, nu=1):
    """qed_helpers.py:80-90."""
    assert (mu, nu) == (0, 1)
    P = ops.plaquettes(_batched(links))
    return P if links.dim() == 4 else P[0]


def batch_plaqs(x, mu: int = 0, nu: int = 1):
    """qed_helpers.py:94-105."""
    return compute_u1_plaq(x, mu, nu)


def u1_plaq(x, mu: int, nu: int):
    """qed_helpers.py:66-70 (same plaquette, other summation order)."""
    return compute_u1_plaq(x, mu, nu)


def plaq_phase(f, mu=0, nu=1):
    """qed_helpers.py:246-257 (squeezes a leading batch of 1)."""
    f = torch.squeeze(f)
    return compute_u1_plaq(f, mu, nu)


def batch_charges(x: torch.Tensor = None, plaqs: torch.Tensor = None):
    """qed_helpers.py:108-116."""
    if plaqs is None:
        if x is None:
            raise ValueError('Either `x` or `plaq` must be specified.')
        return ops.wilson_action_charge(_batched(x), 1.0)[1]
    return ops.wrap(plaqs).flatten(1).sum(1) / TWO_PI


def topo_charge(x):
    """qed_helpers.py:73-77."""
    return batch_charges(x=x)


def wilson_loops(x: torch.Tensor, Rmax: int, Tmax: Optional[int] = None):
    """The table of rectangular Wilson loops of a field [2, L, L] or a batch [B, 2, L, L] -> [B, Rmax, Tmax]
    (`ops.wilson_loops`: entry [b, R - 1, T - 1], R along axis -2, T along axis -1, wrapping).  Beyond the reference, whose
    only gauge-invariant observables are the plaquette and the charge; `utils.observables.exact_wilson_loop` is the exact value
    of its expectation.  Not differentiable."""
    return ops.wilson_loops(_batched(x), Rmax, Tmax)


def polyakov_correlator(x: torch.Tensor, Rmax: Optional[int] = None):
    """< P(i) P*(i + R) >, R = 1 .. Rmax (default L), of the Polyakov loops P(i) = exp(i sum_j x1[i][j]) -> [B, Rmax]: the column
    T = L of the loop table, where the two sides along axis -2 cancel."""
    xb = _batched(x)
    L = xb.shape[-1]
    return ops.wilson_loops(xb, L if Rmax is None else Rmax, L)[:, :, L - 1]


class _WilsonActionFn(torch.autograd.Function):
    """S_b(x) with its gradient dS_b/dx = fthmc_wilson_force (so flows trained through
    `action(x)` by autograd, train.py:202-210, see the Wilson term)."""

    @staticmethod
    def forward(ctx, x, beta):
        ctx.save_for_backward(x)
        ctx.beta = beta
        return ops.wilson_action_charge(x, beta)[0]

    @staticmethod
    def backward(ctx, gS):
        (x,) = ctx.saved_tensors
        return ops.wilson_force(x, ctx.beta) * gS[:, None, None, None], None


class BatchAction:
    """qed_helpers.py:166-186: S_b = -beta sum cos P."""

    def __init__(self, beta):
        self.beta = beta

    def __call__(self, x: torch.Tensor):
        if x.requires_grad:
            return _WilsonActionFn.apply(x, self.beta)
        return ops.wilson_action_charge(x, self.beta)[0]


@dataclass
class LatticeMetrics:
    beta: float
    plaqs: torch.Tensor
    action: torch.Tensor
    charges: torch.Tensor


class BatchObservables:
    """qed_helpers.py:130-163."""

    def __init__(self, beta: float = 1.):
        self.beta = beta

    def get_plaqs(self, x):
        return torch.cos(batch_plaqs(x))

    def get_action(self, x=None, plaqs=None):
        if x is None:
            raise ValueError('`x` must be specified.')
        return ops.wilson_action_charge(x, self.beta)[0]

    def get_charges(self, x=None, plaqs=None):
        return batch_charges(x=x, plaqs=plaqs)

    def get_observables(self, x):
        S, Q, _ = ops.wilson_action_charge(x, self.beta)
        return LatticeMetrics(self.beta, self.get_plaqs(x), S, Q)


# ---------------------------------------------------------------- flow drivers
def ft_flow(flow: nn.ModuleList, x: torch.Tensor):
    """qed_helpers.py:191-198: x -> F(x)."""
    return ops.flow_forward(x, flow_weights(flow, x.device), len(flow), flow_activation(flow))[0]


def ft_flow_inv(flow: nn.ModuleList, x: torch.Tensor, tol: float = 1e-12):
    """qed_helpers.py:201-209: x -> F^-1(x)."""
    return ops.flow_reverse(x, flow_weights(flow, x.device), len(flow), flow_activation(flow), tol=tol)[0]


# ---------------------------------------------------------------- autograd through S_eff and the force
# meta of a flow call: (n_layers, beta, activation, net shape); the conv parameters go in as inputs of their own, so that their
# gradients land in each one's .grad as torch puts them (plain flows and flows flattened by flatten_flow alike)
def _flow_call(flow, beta, dev, w=None):
    w = flow_weights(flow, dev) if w is None else w
    params = [p for row in _flow_rows(flow) for p in row]
    return w, (len(flow), float(beta), flow_activation(flow), ops.arch_of(w)), params


def _split_params(gw, meta, nparams: int):
    """flat [n_layers * params] -> one gradient per conv parameter, in the order _flow_call lists them"""
    nl, _, _, arch = meta
    return [g for row in ops.unpack_weight_grads(gw, nl, arch=arch) for g in row] if nl else [None] * nparams


class _FtForceFn(torch.autograd.Function):
    """F = d(sum_b S_eff)/dx (the tuned ft_force) attached to autograd wrt the field and every conv parameter: the backward is
    the force VJP (fthmc_ft_force_vjp: gx = H g, gw = d/dw <g, F>).  Third order raises (once_differentiable)."""

    @staticmethod
    def forward(ctx, x, w, meta, *params):
        nl, beta, act, arch = meta
        ctx.save_for_backward(x, w)
        ctx.meta = meta
        return ops.ft_force(x, w, nl, beta, act, arch=arch)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        nl, beta, act, arch = ctx.meta
        need_gx, need_gw = ctx.needs_input_grad[0], any(ctx.needs_input_grad[3:])
        if not (need_gx or need_gw):
            return (None, None, None) + (None,) * (len(ctx.needs_input_grad) - 3)
        gx, gw = ops.ft_force_vjp(x, w, nl, beta, g.contiguous(), act, arch=arch, need_gx=need_gx, need_gw=need_gw)
        npar = len(ctx.needs_input_grad) - 3
        gparams = _split_params(gw, ctx.meta, npar) if need_gw else [None] * npar
        return (gx, None, None, *gparams)


class _ActionGwFn(torch.autograd.Function):
    """d/dw sum_b gS_b S_eff_b (the action VJP) as a node whose own derivative raises: second derivatives of S_eff with respect
    to the flow weights are not part of the HIP path"""

    @staticmethod
    def forward(ctx, x, w, gS, meta, *params):
        nl, beta, act, arch = meta
        return ops.ft_action_vjp(x, w, nl, beta, gS.contiguous(), None, act, arch=arch, need_gx=False)[1]

    @staticmethod
    def backward(ctx, ggw):
        raise RuntimeError('ft_action: second derivatives with respect to the flow weights are not supported '
                           '(only the force, d S_eff / dx, can be differentiated again)')


class _FtActionFn(torch.autograd.Function):
    """S_eff per chain, differentiable in the field and every conv parameter: gx = gS_b F_b through _FtForceFn (so that
    autograd.grad(S.sum(), x, create_graph=True) is the differentiable force), gw from the action VJP"""

    @staticmethod
    def forward(ctx, x, w, meta, *params):
        nl, beta, act, arch = meta
        ctx.save_for_backward(x, w, *params)
        ctx.meta = meta
        return ops.ft_action(x, w, nl, beta, act, arch=arch)[0]

    @staticmethod
    def backward(ctx, gS):
        x, w, *params = ctx.saved_tensors
        meta = ctx.meta
        gx = None
        if ctx.needs_input_grad[0]:
            gx = _FtForceFn.apply(x, w, meta, *params) * gS[:, None, None, None]
        gparams = [None] * len(params)
        if any(ctx.needs_input_grad[3:]):
            gparams = _split_params(_ActionGwFn.apply(x, w, gS, meta, *params), meta, len(params))
        return (gx, None, None, *gparams)


def _wants_graph(x, params):
    return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))


def flowed_action(flow, x: torch.Tensor, beta: float, w: Optional[torch.Tensor] = None):
    """S_eff = S_W(F(x)) - log det J per chain; attached to autograd (field and conv parameters) when grad mode is on and either
    requires grad, plain numbers otherwise.  `w`: the flow's flat weights when the caller has them."""
    w, meta, params = _flow_call(flow, beta, x.device, w)
    if _wants_graph(x, params):
        return _FtActionFn.apply(x, w, meta, *params)
    return ops.ft_action(x, w, meta[0], beta, meta[2], arch=meta[3])[0]


def ft_action(param, flow, x: torch.Tensor):
    """qed_helpers.py:212-223: S_W(F(x)) - sum_l logJ_l, per chain.  Differentiable in the field and every conv parameter (as
    the reference's) when grad mode is on and either requires grad; the same numbers either way."""
    return flowed_action(flow, x, param.beta)


def ft_force(param, flow, field: torch.Tensor, create_graph=False):
    """qed_helpers.py:226-242: d(sum_b S_eff)/dx.  create_graph=True: the same numbers, attached to autograd with respect to the
    field (when it requires grad) and every conv parameter, whose backward is the force VJP (fthmc_ft_force_vjp): losses of the
    force, Hessian-vector products of S_eff.  Third derivatives raise."""
    w, meta, params = _flow_call(flow, param.beta, field.device)
    if create_graph:
        return _FtForceFn.apply(field, w, meta, *params)
    return ops.ft_force(field, w, meta[0], param.beta, meta[2], arch=meta[3])


# ---------------------------------------------------------------- plain HMC
def action(param, x: torch.Tensor):
    """qed_helpers.py:261-262: one scalar for the whole tensor."""
    return ops.wilson_action_charge(_batched(x), param.beta)[0].sum()


def force(param, x: torch.Tensor):
    """qed_helpers.py:265-272."""
    return ops.wilson_force(_batched(x), param.beta).reshape(x.shape)


def leapfrog(param, x: torch.Tensor, p: torch.Tensor, verbose: bool = True, integrator: str = 'leapfrog'):
    """qed_helpers.py:275-295.  integrator: 'leapfrog' | 'omelyan' | 'force_gradient' (beyond the reference: csrc/integrator.h)."""
    xo, po = ops.leapfrog(_batched(x), _batched(p), param.beta, param.dt, param.nstep, integrator=integrator)
    return xo.reshape(x.shape), po.reshape(p.shape)


def hmc(param, x, verbose=True, v: Optional[torch.Tensor] = None, u: Optional[torch.Tensor] = None, integrator: str = 'leapfrog'):
    """qed_helpers.py:298-311: one trajectory; the whole tensor is ONE system (one H, one
    accept), as in the reference.  `v`, `u` may be supplied for reproducible checks."""
    xb = _batched(x)
    if v is None:
        v = torch.randn_like(xb)
    if u is None:
        u = torch.rand([], dtype=torch.float64, device=x.device)
    vb = _batched(v)
    if xb.shape[0] == 1:
        r = ops.hmc_trajectory(xb, vb, u.reshape(1), param.beta, param.dt, param.nstep, integrator=integrator)
        dH = r['dH'][0]
        acc = r['acc'][0] > 0.5
        return dH, torch.exp(-dH), acc, r['x_new'].reshape(x.shape)
    h0 = ops.wilson_action_charge(xb, param.beta)[0].sum() + 0.5 * ops.kinetic(vb).sum()
    x_, v_ = ops.leapfrog(xb, vb, param.beta, param.dt, param.nstep, integrator=integrator)
    xr = ops.regularize(x_)
    dH = ops.wilson_action_charge(xr, param.beta)[0].sum() + 0.5 * ops.kinetic(v_).sum() - h0
    exp_mdH = torch.exp(-dH)
    acc = u < exp_mdH
    newx = xr if bool(acc) else xb
    return dH, exp_mdH, acc, newx.reshape(x.shape)


# ---------------------------------------------------------------- local updates (beyond the reference, which updates by MD only)
def heatbath(param, x: torch.Tensor, seeds: Optional[torch.Tensor] = None):
    """One heatbath sweep at param.beta: every link drawn from its conditional von Mises distribution (ops.local_update; no step
    size, acceptance 1).  seeds: int64 per chain (ops.chain_seeds); None: drawn from torch's generator."""
    xb = _batched(x)
    if seeds is None:
        seeds = torch.randint(0, 2 ** 63 - 1, (xb.shape[0],), dtype=torch.int64, device=xb.device)
    return ops.local_update(xb, param.beta, seeds, n_hb=1, n_or=0).reshape(x.shape)


def overrelax(param, x: torch.Tensor, n: int = 1):
    """`n` overrelaxation sweeps: every link reflected about its conditional mode; the action is unchanged (to rounding), nothing is
    drawn.  Not ergodic on its own: mixed with heatbath or HMC (run_local, run_hmc(overrelax=n))."""
    return ops.local_update(_batched(x), param.beta, None, n_hb=0, n_or=int(n)).reshape(x.shape)


def instanton_hit(param, x: torch.Tensor, n_hit: int = 1, seeds: Optional[torch.Tensor] = None):
    """`n_hit` instanton hits at param.beta (ops.instanton_hit): Metropolis steps in the net charge k of the proposal x + k A, A the
    constant-field-strength configuration of charge 1 -> (x_new, k, nacc), k and nacc int32 per chain.  The update that moves the
    topological charge where HMC and the local updates freeze; exact for the plain Wilson action.  seeds: int64 per chain
    (ops.chain_seeds); None: drawn from torch's generator."""
    xb = _batched(x)
    if seeds is None:
        seeds = torch.randint(0, 2 ** 63 - 1, (xb.shape[0],), dtype=torch.int64, device=xb.device)
    xn, k, nacc = ops.instanton_hit(xb, param.beta, seeds, n_hit=int(n_hit))
    return xn.reshape(x.shape), k, nacc


def ft_leapfrog(param, flow, x: torch.Tensor, p: torch.Tensor, integrator: str = 'leapfrog'):
    """ipynb/ft_hmc.py:394-418: the MD in the latent field with the flowed force -> (x', p').
    integrator: 'leapfrog' | 'omelyan' | 'force_gradient' (beyond the reference: csrc/integrator.h)."""
    xb = _batched(x)
    w, nl, act = flow_weights(flow, xb.device), len(flow), flow_activation(flow)
    xo, po = ops.ft_leapfrog(xb, _batched(p), w, nl, param.beta, param.dt, param.nstep, act, integrator=integrator)
    return xo.reshape(x.shape), po.reshape(p.shape)


# ---------------------------------------------------------------- ftHMC on the physical field
def ft_hmc(param, flow, field: torch.Tensor, v: Optional[torch.Tensor] = None, u: Optional[torch.Tensor] = None,
           tol: float = 1e-12, integrator: str = 'leapfrog'):
    """ipynb/ft_hmc.py:420-435: one ftHMC trajectory that starts and ends on the PHYSICAL field:
    x = F^-1(field); momenta; leapfrog in the latent field with ft_force (`:394-418`); xr = regularize(x_);
    accept on u < exp(-dH); return F(newx).  Like the notebook the whole tensor is ONE system (one H,
    one accept; the notebook always passes [1, 2, L, L]).  -> (dH, exp_mdH, acc, newfield).

    `v`, `u` may be supplied for reproducible checks (the notebook draws randn_like(x), then rand([])).
    `tol`: tolerance of the inverse flow (the reference bisects to a global 1e-6)."""
    fb = _batched(field)
    w, nl, act = flow_weights(flow, fb.device), len(flow), flow_activation(flow)
    x = ops.flow_reverse(fb, w, nl, act, tol=tol)[0]
    if v is None:
        v = torch.randn_like(x)
    if u is None:
        u = torch.rand([], dtype=torch.float64, device=x.device)
    vb = _batched(v)
    if x.shape[0] == 1:
        r = ops.ft_trajectory(x, vb, u.reshape(1), w, nl, param.beta, param.dt, param.nstep, act, mode='md', integrator=integrator)
        dH, acc, newx = r['dH'][0], r['acc'][0] > 0.5, r['x_new']
    else:
        h0 = ops.ft_action(x, w, nl, param.beta, act)[0].sum() + 0.5 * ops.kinetic(vb).sum()
        x_, v_ = ops.ft_leapfrog(x, vb, w, nl, param.beta, param.dt, param.nstep, act, integrator=integrator)
        xr = ops.regularize(x_)
        dH = ops.ft_action(xr, w, nl, param.beta, act)[0].sum() + 0.5 * ops.kinetic(v_).sum() - h0
        acc = u < torch.exp(-dH)
        newx = xr if bool(acc) else x
    exp_mdH = torch.exp(-dH)
    newfield = ops.flow_forward(newx, w, nl, act)[0]
    return float(dH), float(exp_mdH), acc, newfield.reshape(field.shape)


def ft_run(param, flow, field: Optional[torch.Tensor] = None, logfile: Optional[str] = None, verbose: bool = False,
           use_graph: Optional[bool] = None, integrator: str = 'leapfrog', instanton: int = 0):
    """ipynb/ft_hmc.py:437-487: `param.nrun` x `param.ntraj` physical-field ftHMC trajectories of one
    configuration [2, L, L].  Returns (field, history) with per-trajectory dH, exp_mdH, acc, plaq, topo
    (the notebook returns the field and keeps the histories in module globals); the status lines it prints
    go to `logfile` when given.

    On the device the trajectory sequence (inverse flow, momenta and the uniform from torch's generator, the fused trajectory,
    forward flow, observables) is captured once in a hipGraph and replayed (`use_graph`, default on; FTHMC_RUN_GRAPH=0 turns it
    off): the notebook's loop synchronises five times per trajectory, this one not at all; the histories and the log are
    written when the loop has run.  Same draws, identical numbers.

    instanton = k (default 0: nothing changes): k instanton hits (instanton_hit) behind every trajectory, before it is measured; the
    history gains 'inst_acc' (accepted / k) and 'inst_dq' (the applied charge).  The chain's state here is the PHYSICAL field, and
    the flow only changes how the molecular dynamics proposes: the target density of that field is exp(-S_W).  The hit's proposal
    x -> x +- A is symmetric and volume-preserving in that field, so its acceptance with the plain Wilson action is exact between
    flowed trajectories; no Jacobian of the flow enters."""
    from ..graph_loop import instanton_arg, run_graph_default
    ops.integrator_code(integrator)                                      # an unknown name raises before anything runs
    instanton = instanton_arg(instanton)
    if field is None:
        field = param.initializer()[0]
    history = {k: [] for k in ('dH', 'exp_mdH', 'acc', 'plaq', 'topo')}
    out = open(logfile, 'w') if logfile else None
    use_graph = run_graph_default() if use_graph is None else use_graph

    def put(s):
        if out is not None:
            out.write(s)
        if verbose:
            print(s, end='', flush=True)

    def record(k, dH, exp_mdH, acc, plaq, topo, hits=None):
        """trajectory k into the history and the log; hits: (applied charge, accepted hits) of the instanton hits behind it"""
        for key, val in zip(history, (dH, exp_mdH, float(acc), plaq, topo)):
            history[key].append(val)
        if hits is not None:
            history.setdefault('inst_dq', []).append(int(hits[0]))
            history.setdefault('inst_acc', []).append(hits[1] / instanton)
        put(f'Traj: {k:4}  {"ACCEPT" if acc else "REJECT"}  dH: {dH:< 12.8}  '
            f'exp(-dH): {exp_mdH:< 12.8}  plaq: {plaq:< 12.8}  topo: {topo:< 3.3}\n')
    try:
        S, Q, plaq = ops.wilson_action_charge(_batched(field), param.beta)
        put(f'Initial configuration:  plaq: {float(plaq[0])}  topo: {float(Q[0])} {tuple(field.shape)}\n')
        ntot = param.nrun * param.ntraj
        if use_graph and field.is_cuda and ntot > 0:
            field, cols = _ft_run_captured(param, flow, field, ntot, integrator=integrator, instanton=instanton)
            c = {name: col.reshape(-1).tolist() for name, col in cols.items()}
            for k in range(ntot):
                record(k + 1, c['dH'][k], c['exp_mdH'][k], c['acc'][k] > 0.5, c['plaq'][k], c['Q'][k],
                       (c['k'][k], c['nacc'][k]) if instanton else None)
        else:
            for k in range(ntot):
                dH, exp_mdH, acc, field_run = ft_hmc(param, flow, field.reshape((1,) + tuple(field.shape[-3:])), integrator=integrator)
                hits = None
                if instanton:
                    field_run, ik, ina = instanton_hit(param, field_run, instanton)
                    hits = (ik[0], int(ina[0]))
                field = field_run[0]
                S, Q, plaq = ops.wilson_action_charge(field_run, param.beta)
                record(k + 1, dH, exp_mdH, bool(acc), float(plaq[0]), float(Q[0]), hits)
    finally:
        if out is not None:
            out.close()
    return field, history


def _ft_run_captured(param, flow, field: torch.Tensor, ntot: int, tol: float = 1e-12, integrator: str = 'leapfrog', instanton: int = 0):
    """the loop of ft_run as one captured sequence per trajectory -> (final field [2, L, L], {name: [ntot, 1]} on the host) of the
    row dH, acc, plaq, Q, exp_mdH and, with instanton > 0, the applied charge k and the accepted hits nacc."""
    from ..graph_loop import GraphLoop, Row
    dev = field.device
    fs = field.detach().reshape((1,) + tuple(field.shape[-3:])).clone()
    L = fs.shape[-1]
    w, nl, act = flow_weights(flow, dev), len(flow), flow_activation(flow)
    # the weights do not change inside this loop: every launch states one content version, the library expands them once
    # (the first call) and checks the stamp on the device afterwards (include/fthmc_hip.h "Weight versions")
    wkey = ('ft_run', id(flow), w.data_ptr(), w._version, weights_generation(w), time.monotonic_ns())
    v = torch.empty_like(fs)
    u = torch.empty(1, dtype=torch.float64, device=dev)
    row = Row(dev, dH=1, acc=1, plaq=1, Q=1, exp_mdH=1, k=1 if instanton else 0, nacc=1 if instanton else 0)
    if instanton:
        iseeds = torch.empty(1, dtype=torch.int64, device=dev)
        iout = {'x': fs, 'k': torch.empty(1, dtype=torch.int32, device=dev), 'nacc': torch.empty(1, dtype=torch.int32, device=dev)}
    res = {'x_new': torch.empty_like(fs), 'dH': row['dH'], 'acc': row['acc'],
           **{k: torch.empty(1, dtype=torch.float64, device=dev) for k in ('plaq', 'Q', 'H0', 'H1')}}
    obs = {'S': torch.empty(1, dtype=torch.float64, device=dev), 'Q': row['Q'], 'plaq': row['plaq']}

    def enqueue():
        x = ops.flow_reverse(fs, w, nl, act, tol=tol, wkey=wkey)[0]      # x = F^-1(field)
        v.normal_()                                                      # randn_like(x), then rand([]): ipynb/ft_hmc.py:423-424
        u.uniform_()
        ops.ft_trajectory(x, v, u, w, nl, param.beta, param.dt, param.nstep, act, mode='md', out=res, wkey=wkey, integrator=integrator)
        fs.copy_(ops.flow_forward(res['x_new'], w, nl, act, wkey=wkey)[0])   # newfield = F(newx)
        if instanton:
            torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64, device=dev, out=iseeds)
            ops.instanton_hit(fs, param.beta, iseeds, n_hit=instanton, out=iout)
            row['k'].copy_(iout['k'])
            row['nacc'].copy_(iout['nacc'])
        ops.wilson_action_charge(fs, param.beta, out=obs)
        torch.exp(torch.neg(row['dH']), out=row['exp_mdH'])
    loop = GraphLoop(enqueue, row.flat, use_graph=True)
    for k in range(ntot):
        loop.step()
    cols = row.split(loop.rows())
    loop.join()
    return fs[0].clone(), cols


def flow_resize(flow: nn.ModuleList, lat_new):
    """ipynb/ft_hmc.py:489-513: the same (translation-equivariant) conv nets with masks of another lattice."""
    from .layers import get_nets, make_net_from_layers
    return make_net_from_layers(lattice_shape=tuple(lat_new), nets=get_nets(flow))
