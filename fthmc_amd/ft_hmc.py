"""fthmc/ft_hmc.py on the HIP path: `FieldTransformation` (HMC in the latent field of a trained
flow) and `run_ftHMC`.  Same constructor, methods and metric keys as the reference; no
tensorboard / plotting side effects.

Two reference quirks are explicit switches, defaults = what the method describes:
  leapfrog_mode = 'md'               real MD integrator (ipynb/ft_hmc.py:394-418);
                  'reference_literal' reproduces ft_hmc.py:180-188 (evolution discarded:
                                      proposal = x + dt/2 v with the initial v)
  energy_mode   = 'per_chain'        H_b = S_eff,b + v_b^2 / 2;
                  'reference_literal' reproduces calc_energy ft_hmc.py:177-178
                                      (no 1/2, kinetic term summed over the whole batch)
Beyond the reference: integrator = 'leapfrog' (default) | 'omelyan' | 'force_gradient' chooses the MD between the two energies
(csrc/integrator.h; lfconfig.nstep steps of it cost ops.integrator_forces(integrator, nstep) force evaluations).
`run(..., loops=(Rmax, Tmax))` adds the table of Wilson loops of the PHYSICAL field F(x) to the history ('wloops').
"""
from __future__ import annotations

import functools
import time
from dataclasses import dataclass
from math import pi as PI
from typing import Callable, Optional

import torch
import torch.nn as nn

from . import ops
from .config import DTYPE, TrainConfig, device, lfConfig
from .graph_loop import GraphLoop, LazyHistory, Row, loops_arg, run_graph_default     # (LazyHistory is imported from here too)
from .utils import qed_helpers as qed
from .utils.layers import flow_activation, flow_weights, weights_generation

TWO_PI = 2. * PI


@dataclass
class _CapturedRun:
    """the captured run loop of a FieldTransformation and what it was captured for"""
    sig: tuple                            # everything the capture depends on (see _run_captured)
    loop: GraphLoop
    x: torch.Tensor                       # the field the trajectory advances in place
    state: torch.Tensor                   # its carried (S_eff, plaq, Q) [3, B]
    row: Row
    sides: list                           # the chain groups' side streams
    token: object = None                  # the workspaces the capture saw (ops.trajectory_workspaces)
    pending: Optional[Callable] = None    # reads the history of the last run while the ring still holds it


class FieldTransformation(nn.Module):
    def __init__(self, flow: nn.ModuleList, config: TrainConfig, lfconfig: lfConfig,
                 leapfrog_mode: str = 'md', energy_mode: str = 'per_chain', integrator: str = 'leapfrog'):
        super().__init__()
        assert leapfrog_mode in ('md', 'reference_literal') and energy_mode in ('per_chain', 'reference_literal')
        if ops.integrator_code(integrator) and leapfrog_mode != 'md':       # (an unknown name: ValueError)
            raise ValueError(f'leapfrog_mode {leapfrog_mode!r} discards the MD: it goes with integrator=\'leapfrog\' only')
        self.integrator = integrator
        self.flow = flow
        self.config = config
        self.lfconfig = lfconfig
        self.dt, self.tau, self.nstep = lfconfig.dt, lfconfig.tau, lfconfig.nstep
        self.leapfrog_mode, self.energy_mode = leapfrog_mode, energy_mode
        self._denom = self.config.beta * self.config.volume
        self._w = None
        self._w_versions = None
        self._params = None
        self._flow_key = None
        # (field tensor, its version, weight key, beta, state [3, B]) of the last trajectory's result
        self._carry = None
        self._last_obs = None         # (plaq, Q) of the flowed accepted field of the last trajectory (run() reads them)
        self._loop = None             # the captured run loop (_CapturedRun)
        self._loop_streams = None     # its stream and the chain groups' side streams: made once, reused by every re-capture
        self.use_graph = run_graph_default()

    # ---- weights: packed once, refreshed when a parameter changed in place -----------
    def weights(self, dev) -> torch.Tensor:
        # the parameter list is gathered once per flow (Module.parameters() walks the module tree: it was two thirds of the host
        # time of a trajectory at L = 16) and again when the flow object, its length or one of its conv nets was replaced
        fkey = (id(self.flow), tuple(id(layer.plaq_coupling.net) for layer in self.flow))
        if self._params is None or self._flow_key != fkey:
            self._params = list(self.flow.parameters())
            self._flow_key = fkey
            self._w = None
        vers = tuple(p._version for p in self._params)
        if self._w is None or self._w_versions != vers or self._w.device != dev:
            self._w = flow_weights(self.flow, dev)
            self._w_versions = vers
        return self._w

    def _wkey(self, w: torch.Tensor):
        """What the weights' CONTENT is keyed by: the flow's identity, every parameter's version (torch optimizers,
        load_state_dict), the flat buffer's generation (FlatAdam / graph replays write it through raw pointers) and its own
        version.  The tensor's identity says nothing: a flattened flow hands out the same buffer before and after a step."""
        return (self._flow_key, self._w_versions, w.data_ptr(), w._version, weights_generation(w))

    def _carried_state(self, x: torch.Tensor, wkey):
        """(S_eff, plaq, Q) of x if x IS the field the previous trajectory returned, untouched, under the same weights and beta"""
        c = self._carry
        if c is not None and c[0] is x and c[1] == x._version and c[2] == wkey and c[3] == self.config.beta:
            return c[4]
        return None

    @property
    def _act(self):
        return flow_activation(self.flow)

    # ---- reference methods ----------------------------------------------------------
    def action(self, x: torch.Tensor):
        """ft_hmc.py:135-141: S_W(F(x)) - sum logJ, per chain.  Differentiable in x and every conv parameter (as the reference's)
        when grad mode is on and either requires grad: autograd.grad(action(x).sum(), x, create_graph=True) is the force, and
        differentiable again (qed_helpers.flowed_action)."""
        return qed.flowed_action(self.flow, x, self.config.beta, self.weights(x.device))

    def _action(self, x: torch.Tensor):
        """S_eff without an autograd graph: what the drivers (calc_energy, hmc, run) use"""
        return ops.ft_action(x, self.weights(x.device), len(self.flow), self.config.beta, self._act)[0]

    def flow_forward(self, x: torch.Tensor):
        """ft_hmc.py:143-150 -> (F(x), logdet)."""
        return ops.flow_forward(x, self.weights(x.device), len(self.flow), self._act)

    def flow_backward(self, x: torch.Tensor, tol: float = 1e-12):
        """ft_hmc.py:152-160 -> (F^-1(x), logdet)."""
        return ops.flow_reverse(x, self.weights(x.device), len(self.flow), self._act, tol=tol)

    def force(self, x: torch.Tensor):
        """ft_hmc.py:162-171 (the reference only works for B = 1; any B here)."""
        return ops.ft_force(x.detach(), self.weights(x.device), len(self.flow), self.config.beta, self._act)

    @staticmethod
    def wrap(x: torch.Tensor):
        """ft_hmc.py:173-175."""
        return ops.wrap(x)

    def calc_energy(self, x: torch.Tensor, v: torch.Tensor):
        """ft_hmc.py:177-178 (literal) or the per-chain Hamiltonian."""
        if self.energy_mode == 'reference_literal':
            return self._action(x) + ops.kinetic(v).sum()
        return self._action(x) + 0.5 * ops.kinetic(v)

    def leapfrog(self, x: torch.Tensor, v: torch.Tensor):
        """ft_hmc.py:180-188."""
        if self.leapfrog_mode == 'reference_literal':
            return x + 0.5 * self.dt * v, v
        return ops.ft_leapfrog(x, v, self.weights(x.device), len(self.flow), self.config.beta, self.dt,
                               self.nstep, self._act, integrator=self.integrator)

    def _mode(self):
        return 'md' if self.leapfrog_mode == 'md' else 'literal'

    def _trajectory(self, x, v, u, groups: int = 1):
        """The fused trajectory of hmc() and _batch_hmc() -> (accepted field, the results of ops.ft_trajectory).
        (S_eff, plaq, Q) of x is carried over when x IS the field the previous call returned, untouched, under the same
        weights (by content: _wkey) and beta: that call's H1 sweep computed exactly what this call's H0 sweep would
        (bit-identical; bench.py's `stateless` figure is the price of recomputing it, as the reference does at ft_hmc.py:205).
        plaq / Q of the flowed accepted field come with the trajectory: run() need not flow x again for its metrics
        (kept out of the returned metrics: those are the reference's keys, ft_hmc.py:244-257)."""
        w = self.weights(x.device)
        wkey = self._wkey(w)
        r = ops.ft_trajectory(x, v, u, w, len(self.flow), self.config.beta, self.dt, self.nstep, self._act, mode=self._mode(),
                              state_in=self._carried_state(x, wkey), groups=groups, wkey=wkey, integrator=self.integrator)
        xnew = r['x_new'].detach()
        self._carry = (xnew, xnew._version, wkey, self.config.beta, r['state'])
        self._last_obs = (r['plaq'], r['Q'])
        return xnew, r

    def hmc(self, x: torch.Tensor, step: int = None, v: Optional[torch.Tensor] = None,
            u: Optional[torch.Tensor] = None):
        """ft_hmc.py:190-224: the tensor is one system (one scalar H, one accept).  For the usual
        [1, 2, L, L] field this is a single fused trajectory launch sequence."""
        x = x.to(device()) if not x.is_cuda else x
        t0 = time.time()
        metrics = {} if step is None else {'traj': step}
        v = torch.randn_like(x) if v is None else v
        u = torch.rand([], dtype=torch.float64, device=x.device) if u is None else u
        self._last_obs = None
        if x.shape[0] == 1:
            # the packaged code maps the end point with wrap, the notebook with regularize: same set
            xnew, r = self._trajectory(x, v, u.reshape(1))
            acc, dh = r['acc'][0] > 0.5, r['dH'][0]
        else:
            h0 = self._action(x).sum() + 0.5 * ops.kinetic(v).sum()
            x_, v_ = self.leapfrog(x, v)
            x_ = self.wrap(x_)
            dh = self._action(x_).sum() + 0.5 * ops.kinetic(v_).sum() - h0
            acc = u < torch.exp(-dh)
            xnew = x_ if bool(acc) else x
        metrics.update({'dt': time.time() - t0, 'acc': acc.detach(), 'dh': dh.detach()})
        return xnew, metrics

    def _batch_hmc(self, x: torch.Tensor, step: int = None, v: Optional[torch.Tensor] = None,
                   u: Optional[torch.Tensor] = None):
        """ft_hmc.py:226-257: independent chains, per-chain accept (dead code in the reference
        for B > 1 because its force only works for B = 1)."""
        t0 = time.time()
        metrics = {} if step is None else {'traj': step}
        v = torch.randn_like(x) if v is None else v
        u = torch.rand(x.shape[0], dtype=torch.float64, device=x.device) if u is None else u
        self._last_obs = None
        if self.energy_mode == 'per_chain':
            x_, r = self._trajectory(x, v, u, groups=ops.default_groups(x.shape[0], x.shape[-1]))
            dh, acc = r['dH'], r['acc']
        else:
            h = self.calc_energy(x, v)
            xp, v_ = self.leapfrog(x, v)
            xp = self.wrap(xp)
            dh = self.calc_energy(xp, v_) - h
            acc = (u < torch.exp(-dh)).to(DTYPE)
            x_ = torch.where(acc[:, None, None, None] > 0.5, xp, x)
        metrics.update({'dt': time.time() - t0, 'acc': acc, 'dh': dh, 'exp_mdh': torch.exp(-dh)})
        return x_.detach() if x_.requires_grad else x_, metrics

    def initializer(self, rand: bool = True):
        """ft_hmc.py:259-264: U(0, 2 pi) latent start."""
        x = torch.zeros([self.config.nd] + self.config.lat, dtype=DTYPE, device=device())
        if rand:
            x = x.uniform_(0, TWO_PI)
        return x[None, :]

    def lattice_metrics(self, x: torch.Tensor, qold: torch.Tensor):
        """ft_hmc.py:266-270."""
        S, q, p = ops.wilson_action_charge(x, self.config.beta)
        return {'plaq': p, 'q': q, 'dq': torch.sqrt((q - qold) ** 2)}

    def run(self, x: torch.Tensor = None, nprint: int = 25, nplot: int = 25, window: int = 10,
            num_trajs: int = 1024, writer=None, plotdir: str = None, batch: bool = False, use_graph: bool = None,
            loops=None, loops_every: int = 1, **kwargs):
        """ft_hmc.py:272-346 without plotting: returns the history dict of per-trajectory metrics.
        batch=True advances a batch of independent chains with per-chain accepts.

        On the device the trajectory sequence (momenta and uniforms from torch's generator, the fused trajectory with the
        carried state, in place) is captured once in a hipGraph and replayed (`use_graph`, default on; FTHMC_RUN_GRAPH=0
        turns it off): the host issues one graph launch and one small copy per trajectory, the history is read back when it
        is first looked at.  Same draws and bit-identical histories as the eager loop.

        loops = (Rmax, Tmax) (default None: nothing is measured, nothing changes): after every `loops_every`-th trajectory
        (0, loops_every, ...) the Wilson loops W(R, T), R <= Rmax, T <= Tmax, of the PHYSICAL field F(x) of the accepted latent
        field are measured (ops.flow_forward, ops.wilson_loops) and history['wloops'] gains their mean over the chains, one
        [Rmax, Tmax] table per measured trajectory.  In the captured loop the measurement is a captured sequence of its own
        behind the trajectory's and the table rides in the loop's row.  utils.observables has the exact values and the analysis."""
        if x is None:
            x = self.initializer()
        loops = self._loops_arg(loops, x.shape[-1])
        loops_every = max(1, int(loops_every))
        use_graph = self.use_graph if use_graph is None else bool(use_graph)
        fused = (self.energy_mode == 'per_chain') if batch else (x.shape[0] == 1)
        if use_graph and fused and x.is_cuda and num_trajs > 0:
            return self._run_captured(x, nprint, num_trajs, batch, loops, loops_every)
        history = {}
        q = qed.batch_charges(self.flow_forward(x)[0]) if batch else qed.batch_charges(x)
        for i in range(num_trajs):
            x, metrics_ = (self._batch_hmc(x, step=i) if batch else self.hmc(x, step=i))
            qold = history['q'][-1] if 'q' in history else q
            if self._last_obs is not None:                                # the trajectory's own observables (ft_hmc.py:266-270 on F(x))
                p_, q_ = self._last_obs
                metrics = {**metrics_, 'plaq': p_, 'q': q_, 'dq': torch.sqrt((q_ - qold) ** 2)}
            else:
                x_phys, _ = self.flow_forward(x)
                metrics = {**metrics_, **self.lattice_metrics(x_phys, qold)}
            for key, val in metrics.items():
                history.setdefault(key, []).append(val)
            if loops is not None and i % loops_every == 0:
                table = torch.empty(loops, dtype=DTYPE, device=x.device)
                self._measure_loops(x, self.weights(x.device), loops, None, table)
                history.setdefault('wloops', []).append(table)
            if nprint and i % nprint == 0:
                self._print_line(i, metrics['acc'], metrics['dh'], metrics['plaq'], metrics['q'])
        self.x_last = x
        return history

    _loops_arg = staticmethod(loops_arg)

    def _measure_loops(self, x, w, loops, W, table, wkey=None):
        """the loop table of F(x): per chain into W [B, Rmax, Tmax] (or a fresh tensor), its batch mean into `table` [Rmax, Tmax]"""
        x_phys = ops.flow_forward(x, w, len(self.flow), self._act, wkey=wkey)[0]
        ops.wilson_loops(x_phys, loops[0], loops[1], out=W, mean_out=table)

    @staticmethod
    def _print_line(i, acc, dh, plaq, q):
        print(f"traj {i}: acc={float(torch.as_tensor(acc, dtype=torch.float64).mean()):.3f} "
              f"dh={float(torch.as_tensor(dh).mean()):.4g} plaq={float(torch.as_tensor(plaq).mean()):.6f} "
              f"q={float(torch.as_tensor(q).mean()):.3f}", flush=True)

    # ---- the captured loop ----------------------------------------------------------
    @property
    def captured(self) -> bool:
        """whether run() holds a captured loop (it has run through the graph at least once)"""
        return self._loop is not None and self._loop.loop.captured

    def _run_captured(self, x: torch.Tensor, nprint: int, num_trajs: int, batch: bool, loops=None, loops_every: int = 1):
        dev = x.device
        caller = torch.cuda.current_stream(dev)
        B, L = x.shape[0], x.shape[-1]
        w = self.weights(dev)
        wkey = self._wkey(w)
        carried = self._carried_state(x, wkey)                            # by the identity of the tensor the caller passed
        xd = x.detach()
        nl, act, mode, beta = len(self.flow), self._act, self._mode(), self.config.beta
        G = ops.default_groups(B, L) if batch else 1
        # the weights' content version is part of what a capture is FOR: its launches carry it to the library, which checks
        # it on the device against the stamps in the workspaces (include/fthmc_hip.h "Weight versions")
        sig = (tuple(x.shape), dev, w.data_ptr(), nl, act, mode, beta, self.dt, self.nstep, G, batch,
               ops.get_variant(), ops.get_small_path(), ops.weights_version(wkey), self.integrator, loops, loops_every if loops else 1)
        lp = self._loop
        if lp is not None and lp.pending is not None:
            lp.pending()                              # an unread history of the previous run: read it before its ring is reused
            lp.pending = None
        while True:
            if lp is None or lp.sig != sig:
                lp = self._loop = self._make_loop(xd, w, wkey, sig, G, loops, loops_every)
            # start field, start state and the weight expansion on the loop's stream
            lp.loop.stream.wait_stream(caller)
            with torch.cuda.stream(lp.loop.stream):
                if carried is not None:
                    lp.state.copy_(carried.reshape(3, B))
                else:
                    S, _, p_, q_ = ops.ft_action(xd, w, nl, beta, act)
                    torch.stack([S, p_, q_], out=lp.state)
                # the start of the q history: Q of the flowed start field for a batch (ft_hmc.py:311-313), of the field itself otherwise
                q0 = lp.state[2].clone() if batch else qed.batch_charges(xd)
                lp.x.copy_(xd)
                # the workspaces of the loop's streams at their final size, holding the expansion of these weights: the
                # replays' own expansion launches find the stamps and leave at once
                token = ops.trajectory_workspaces(lp.x, w, nl, groups=G, side_streams=lp.sides, wkey=wkey)
            if not (lp.loop.captured and lp.token != token):
                break
            lp = None                   # a workspace moved since the capture (grown by another caller of these streams): capture again
        loop, xs, state, row = lp.loop, lp.x, lp.state, lp.row
        lp.token = token
        loop.reset_history()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(loop.stream)
        for i in range(num_trajs):
            was_captured = loop.captured
            loop.step()
            if loop.captured and not was_captured:
                # the eager first step may have grown a workspace: the capture that followed saw the final ones
                with torch.cuda.stream(loop.stream):
                    lp.token = ops.trajectory_workspaces(xs, w, nl, groups=G, side_streams=lp.sides, wkey=wkey)
            if nprint and i % nprint == 0:
                loop.stream.synchronize()
                r = row.split(row.flat.cpu())
                self._print_line(i, r['acc'], r['dH'], r['plaq'], r['Q'])
        ev1.record(loop.stream)
        with torch.cuda.stream(loop.stream):
            x_out, st_out = xs.clone(), state.clone()
        loop.join()
        self._carry = (x_out, x_out._version, wkey, beta, st_out)
        self._last_obs = None
        self.x_last = x_out
        lp.pending = loop_rows = functools.cache(loop.rows)               # read once: by the history or before the ring is reused

        def fill():
            c = row.split(torch.from_numpy(loop_rows()).to(dev))
            ev1.synchronize()
            dt = ev0.elapsed_time(ev1) * 1e-3 / num_trajs                 # per trajectory, on the device's clock
            qs = torch.cat([q0.reshape(1, -1).to(c['Q'].dtype), c['Q']], 0)
            dq = torch.sqrt((qs[1:] - qs[:-1]) ** 2)
            h = {'traj': list(range(num_trajs)), 'dt': [dt] * num_trajs}
            if batch:
                h.update({'acc': list(c['acc']), 'dh': list(c['dH']), 'exp_mdh': [torch.exp(-dh) for dh in c['dH']]})
            else:
                h.update({'acc': [a[0] > 0.5 for a in c['acc']], 'dh': [dh[0] for dh in c['dH']]})
            h.update({'plaq': list(c['plaq']), 'q': list(c['Q']), 'dq': list(dq)})
            if loops is not None:                                         # the table of the last measured trajectory
                h['wloops'] = list(c['wloops'][::loops_every])
            return h
        return LazyHistory(fill)

    def _make_loop(self, x, w, wkey, sig, G, loops, loops_every) -> _CapturedRun:
        dev, B = x.device, x.shape[0]
        # what this capture is for (all part of `sig`)
        nl, act, mode, beta, integrator = len(self.flow), self._act, self._mode(), self.config.beta, self.integrator
        xs, v = torch.empty_like(x), torch.empty_like(x)
        u = torch.empty(B, dtype=torch.float64, device=dev)
        # acc, dH, plaq, Q of the trajectory; with loops, the batch-mean table [Rmax, Tmax] behind them
        row = Row(dev, acc=B, dH=B, plaq=B, Q=B, wloops=loops)
        state = torch.empty(3, B, dtype=torch.float64, device=dev)
        out = {'x_new': xs, 'acc': row['acc'], 'dH': row['dH'], 'plaq': row['plaq'], 'Q': row['Q'], 'state': state,
               'H0': torch.empty(B, dtype=torch.float64, device=dev), 'H1': torch.empty(B, dtype=torch.float64, device=dev)}

        # the loop's own streams (its own and one per chain group beyond the first), made once per FieldTransformation and
        # reused by every re-capture (a beta scan re-captures per beta: a new stream each time would leave a workspace of
        # 0.3-0.4 GB behind per stream until torch's stream pool wraps)
        if self._loop_streams is None or self._loop_streams[0] != dev:
            self._loop_streams = (dev, torch.cuda.Stream(device=dev), [])
        _, lstream, pool = self._loop_streams
        while len(pool) < max(G, 1) - 1:
            pool.append(torch.cuda.Stream(device=dev))
        sides = pool[:max(G, 1) - 1]

        def enqueue():
            v.normal_()                                                   # = torch.randn_like(x), then torch.rand(B): ft_hmc.py:204, 243
            u.uniform_()
            # in place: the accepted field replaces x, its (S_eff, plaq, Q) the carried state (both read before they are written)
            ops.ft_trajectory(xs, v, u, w, nl, beta, self.dt, self.nstep, act, mode=mode, out=out, state_in=state, groups=G,
                              side_streams=sides, wkey=wkey, integrator=integrator)
        measure = None
        if loops is not None:
            W = torch.empty(B, loops[0], loops[1], dtype=torch.float64, device=dev)

            def measure():
                self._measure_loops(xs, w, loops, W, row['wloops'], wkey=wkey)    # of F(accepted latent field)
        loop = GraphLoop(enqueue, row.flat, use_graph=True, stream=lstream, extra=measure, extra_every=loops_every)
        return _CapturedRun(sig, loop, xs, state, row, sides)


def run_ftHMC(flow: torch.nn.Module, config: TrainConfig, tau: float, nstep: int, num_trajs: int = 1024,
              nprint: int = 50, **kwargs):
    """ft_hmc.py:349-380 -> (ft, history, dirs)."""
    lfconfig = lfConfig(tau=tau, nstep=nstep)
    flow.eval()
    ft = FieldTransformation(flow=flow, config=config, lfconfig=lfconfig, **kwargs)
    history = ft.run(nprint=nprint, num_trajs=num_trajs)
    fthmcdir = f"{config.logdir}/ftHMC/{lfconfig.uniquestr()}"
    dirs = {'logdir': fthmcdir, 'plotsdir': f'{fthmcdir}/plots', 'summarydir': f'{fthmcdir}/summaries'}
    return ft, history, dirs
