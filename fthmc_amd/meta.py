"""Metadynamics HMC of 2D U(1) (beyond the reference, which samples the unbiased action only): HMC under a history-dependent bias
potential V(Q_m) in the continuous charge Q_m = sum sin P / 2 pi (csrc/meta.hip).

While the potential is built, every trajectory is followed by a deposit: each walker adds a hill of height w to the table at its
Q_m, so the barriers between the topological sectors fill up.  Under the frozen table the chain samples exp(-S - V(Q_m)) and
    <O> = sum O e^{V(Q_m)} / sum e^{V(Q_m)}          (utils.observables.reweighted_mean)
is the unbiased expectation value.  Laio & Parrinello 2002; Laio, Martinelli & Sanfilippo 2016 for topology; Eichhorn, Hoelbling
et al. 2021-23 compare it in 2D U(1) with the instanton update (csrc/topo.hip) and tempering (tempering.py) this tree also has."""
from __future__ import annotations

import math
import time
from typing import Optional

import numpy as np

from .config import DTYPE, Param


class MetaPotential:
    """The bias potential: a table V[groups][nb] on the nodes q_i = -qmax + i delta, delta = 2 qmax / (nb - 1), linear between the
    nodes, and outside them V_edge + wall d^2 / 2, d = |q| - qmax.  `groups` rows: chain b of a batch of B reads row
    b // (B // groups) -- 1: all walkers share one potential, B: one per chain.
    `table` is the device tensor the kernels read and ops.meta_deposit updates in place (made on first use); value / slope evaluate
    the same definitions on the host in numpy (float64)."""

    def __init__(self, nb: int, qmax: float, wall: float, groups: int = 1):
        nb, groups, qmax, wall = int(nb), int(groups), float(qmax), float(wall)
        if not 2 <= nb <= 65536 or groups < 1 or not (math.isfinite(qmax) and qmax > 0) or not (math.isfinite(wall) and wall >= 0):
            raise ValueError(f'MetaPotential: 2 <= nb <= 65536, groups >= 1, finite qmax > 0 and wall >= 0 expected, got nb={nb}, '
                             f'groups={groups}, qmax={qmax}, wall={wall}')
        self.nb, self.qmax, self.wall, self.groups = nb, qmax, wall, groups
        self._host = np.zeros((groups, nb))
        self._table = None

    @property
    def delta(self) -> float:
        return (2.0 * self.qmax) / float(self.nb - 1)

    @property
    def nodes(self) -> np.ndarray:
        return -self.qmax + np.arange(self.nb) * self.delta

    @property
    def table(self):
        """float64 [groups, nb] on the device"""
        if self._table is None:
            import torch
            from .config import device
            self._table = torch.from_numpy(self._host).to(device=device(), dtype=DTYPE).contiguous()
        return self._table

    def numpy(self) -> np.ndarray:
        """the table on the host, [groups, nb] (synchronises when it lives on the device)"""
        return self._host.copy() if self._table is None else self._table.detach().cpu().numpy()

    def _locate(self, q):
        q = np.asarray(q, dtype=np.float64)
        t = (q + self.qmax) / self.delta
        fl = np.floor(t)
        inside = (t >= 0.0) & (fl <= self.nb - 2)
        i = np.where(inside, fl, 0).astype(np.int64)
        return q, inside, i, t - fl

    def value(self, q, group: int = 0) -> np.ndarray:
        """V(q) of row `group`"""
        V = self.numpy()[group]
        q, inside, i, f = self._locate(q)
        d = np.abs(q) - self.qmax
        edge = np.where(q < 0.0, V[0], V[-1])
        return np.where(inside, V[i] + f * (V[i + 1] - V[i]), edge + ((0.5 * self.wall) * d) * d)

    def slope(self, q, group: int = 0) -> np.ndarray:
        """V'(q) of row `group`"""
        V = self.numpy()[group]
        q, inside, i, _ = self._locate(q)
        d = np.abs(q) - self.qmax
        return np.where(inside, (V[i + 1] - V[i]) / self.delta, np.where(q < 0.0, -(self.wall * d), self.wall * d))

    def state_dict(self) -> dict:
        return {'nb': self.nb, 'qmax': self.qmax, 'wall': self.wall, 'groups': self.groups, 'table': self.numpy()}

    def load_state_dict(self, state: dict):
        shape = (int(state['groups']), int(state['nb']))
        tab = np.asarray(state['table'], dtype=np.float64)
        if shape != (self.groups, self.nb) or tab.shape != shape:
            raise ValueError(f'MetaPotential.load_state_dict: a table of shape {(self.groups, self.nb)} expected, got {tab.shape}')
        self.qmax, self.wall = float(state['qmax']), float(state['wall'])
        self._host = tab.copy()
        if self._table is not None:
            import torch
            self._table.copy_(torch.from_numpy(self._host))
        return self


def run_meta(param: Param, x=None, potential: Optional[MetaPotential] = None, n_build: int = 0, w: float = 0.0,
             integrator: str = 'leapfrog', use_graph: Optional[bool] = None):
    """`param.nrun` runs of `param.ntraj` HMC trajectories each under the bias `potential` (default: a zero table on
    |Q_m| <= L^2 / 2 pi, which no field leaves: plain HMC).  The first `n_build` trajectories of the experiment (counted through the
    runs) are each followed by a deposit of height `w` per walker at its Q_m (ops.meta_deposit); the rest run on the frozen table.
    x: the start of every run, [2, L, L] or a batch [B, 2, L, L] (default param.initializer()).
    -> (fields_arr, histories, potential): fields_arr[n] is the last field of run n; histories[n] has run_hmc's keys -- 'traj', 'dt',
    'acc', 'dH', 'plaq', 'q', 'dq' -- plus 'qm' and 'vbias' (Q_m and V(Q_m) of the trajectory's field under the table the
    trajectory ran on: the weights of utils.observables.reweighted_mean are exp(vbias)) and 'build' (whether a deposit followed).
    The seeds of trajectory t are ops.chain_seeds(param.seed, chain, t), formed on the device; momenta and accept uniforms come
    from ops.random_momenta; trajectory, deposit and measurement are captured once per phase (graph_loop) and replayed
    (`use_graph`, default on; FTHMC_RUN_GRAPH=0 turns it off): the same bits either way."""
    return _run(param, x, potential, n_build, w, integrator, use_graph, None, 'silu')


def run_ft_meta(param: Param, flow, x=None, potential: Optional[MetaPotential] = None, n_build: int = 0, w: float = 0.0,
                integrator: str = 'leapfrog', use_graph: Optional[bool] = None, act: str = 'silu'):
    """run_meta through a flow: field-transformation HMC under the bias in the charge of the PHYSICAL field F(x)
    (ops.ft_meta_trajectory).  flow: what FieldTransformation takes, an nn.ModuleList of coupling layers (its weights
    through utils.layers.flow_weights; act: their activation); an empty one is plain HMC under the bias.  The loop runs in the
    latent field with the carried table-free state [4, B]; a deposit at the trajectory's own `qm` follows while the table is built;
    plaq, Q, qm, vbias of the physical field come out of the trajectory itself, with no measurement launch.  One captured sequence
    per phase, as run_meta.  -> (fields_arr, histories, potential) with run_meta's history keys; fields_arr[n] is the LATENT field,
    as FieldTransformation.run returns it."""
    if flow is None:
        raise ValueError('run_ft_meta: a flow (a list of coupling layers, possibly empty) expected; run_meta is the driver without one')
    return _run(param, x, potential, n_build, w, integrator, use_graph, flow, act)


def _run(param, x, potential, n_build, w, integrator, use_graph, flow, act):
    """the one loop behind run_meta (flow None) and run_ft_meta"""
    import torch
    from . import ops
    from .graph_loop import GraphLoop, Row, batched_start, chain_history, run_graph_default
    ops.integrator_code(integrator)                                      # an unknown name raises before anything runs
    n_build, w = int(n_build), float(w)
    if n_build < 0 or not (math.isfinite(w) and w >= 0):
        raise ValueError(f'run_meta: n_build >= 0 and a finite w >= 0 expected, got {n_build}, {w}')
    use_graph = run_graph_default() if use_graph is None else use_graph
    x0 = batched_start(param, x)
    dev, B = x0.device, x0.shape[0]
    if potential is None:
        potential = MetaPotential(2, param.L * param.L / (2 * math.pi) + 1.0, 0.0)
    if B % potential.groups:
        raise ValueError(f'run_meta: the potential has {potential.groups} rows, which do not divide the {B} chains')
    table = potential.table
    if flow is not None:
        from .utils.layers import flow_weights
        nl = len(flow)
        wflow = flow_weights(flow, dev) if nl else None
    histories, fields_arr = {}, []
    for n in range(param.nrun):
        t0 = time.time()
        xs, xn, v = x0.clone(), torch.empty_like(x0), torch.empty_like(x0)
        seeds = torch.empty(B, dtype=torch.int64, device=dev)
        u = torch.empty(B, dtype=DTYPE, device=dev)
        counter = torch.full((1,), n * param.ntraj, dtype=torch.int64, device=dev)      # trajectory t of the whole experiment
        row = Row(dev, acc=B, dH=B, plaq=B, Q=B, qm=B, vbias=B)
        out = {'x_new': xn, 'acc': row['acc'], 'dH': row['dH'], 'qm': row['qm'], 'vbias': row['vbias']}
        if flow is not None:
            # both state buffers exist before the capture; which one a trajectory reads is fixed per enqueue (they alternate by copy)
            state = torch.empty(4, B, dtype=DTYPE, device=dev)
            out.update(plaq=row['plaq'], Q=row['Q'], state=torch.empty(4, B, dtype=DTYPE, device=dev))
            S0, _, plaq0, Q0 = ops.ft_action(xs, wflow, nl, param.beta, act)
            _, _, qm0, _ = ops.ft_meta_action(xs, wflow, nl, param.beta, table, potential.qmax, potential.wall, act)
            state.copy_(torch.stack([S0, plaq0, Q0, qm0]))
            q0 = Q0.cpu().numpy()
        else:
            q0 = ops.wilson_action_charge(xs, param.beta)[1].cpu().numpy()

        def enqueue_flow(deposit):
            ops.chain_seeds(param.seed, 0, B, 0, counter=counter, advance=True, out=seeds)
            ops.random_momenta(seeds, xs.shape, out_v=v, out_u=u)
            ops.ft_meta_trajectory(xs, v, u, wflow, nl, param.beta, param.dt, param.nstep, table, potential.qmax, potential.wall, act,
                                   integrator, out=out, state_in=state)
            xs.copy_(xn)
            state.copy_(out['state'])
            if deposit:
                ops.meta_deposit(out['qm'], table, potential.qmax, w)

        def enqueue(deposit):
            if flow is not None:
                return enqueue_flow(deposit)
            ops.chain_seeds(param.seed, 0, B, 0, counter=counter, advance=True, out=seeds)
            ops.random_momenta(seeds, xs.shape, out_v=v, out_u=u)
            ops.meta_trajectory(xs, v, u, param.beta, param.dt, param.nstep, table, potential.qmax, potential.wall, integrator=integrator,
                                out=out)
            xs.copy_(xn)
            if deposit:
                ops.meta_deposit(out['qm'], table, potential.qmax, w)
            ops.wilson_action_charge(xs, param.beta, out={'plaq': row['plaq'], 'Q': row['Q']})
        nbuild = min(max(n_build - n * param.ntraj, 0), param.ntraj)
        stream = torch.cuda.Stream(device=dev)
        parts = []
        for count, deposit in ((nbuild, True), (param.ntraj - nbuild, False)):       # one captured sequence per phase
            if count == 0:
                continue
            loop = GraphLoop(lambda deposit=deposit: enqueue(deposit), row.flat, use_graph=use_graph, stream=stream)
            for _ in range(count):
                loop.step()
            parts.append(loop.rows())
            loop.join()
        c = row.split(np.concatenate(parts + [np.zeros((0, row.width))], axis=0))
        dt = (time.time() - t0) / max(1, param.ntraj)
        cols = {'acc': c['acc'], 'dH': c['dH'], 'plaq': c['plaq'], 'q': c['Q'], 'qm': c['qm'], 'vbias': c['vbias'],
                'build': [i < nbuild for i in range(param.ntraj)]}
        histories[n] = chain_history(n * param.ntraj + 1, dt, q0, cols)
        fields_arr.append(xs.clone())
    return fields_arr, histories, potential
