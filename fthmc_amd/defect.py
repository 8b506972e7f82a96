"""Parallel tempering on boundary conditions (PTBC): plain HMC of a ladder of replicas at ONE beta that differ in the coupling of a
short line of plaquettes, the defect.

K replicas with defect couplings g_k = beta c_k, 0 <= c_0 < ... < c_{K-1} = 1, form a ladder: at c = 0 the line is open and
topological charge flows through it freely, at c = 1 the lattice is the periodic one that is measured, as it is -- no reweighting.
M ladders of K consecutive chains are one batch of B = M K chains that a single trajectory call moves (ops.defect_trajectory: C ABI
fthmc_defect_trajectory).  Every `swap_every`-th trajectory a swap round offers the exchange of neighbouring rungs; for chain a on
rung k and c on rung k + 1

    A = min(1, exp((g_k - g_{k+1}) (Dsum_c - Dsum_a))),     Dsum = sum over the defect of cos P,

which is ops.replica_swap unchanged, given the ladder of g for its betas, Dsum for its C and g_b for its beta_b; fields never move.
Behind every iteration the chains on the top rung are translated by a random shift (ops.defect_translate): a symmetry of the
periodic rung only, which moves the defect relative to the field.

The reference (nftqcd/fthmc) samples the periodic lattice only and has no counterpart (Hasenbusch 2017; Bonanno, Bonati, D'Elia
2021; Luescher, Schaefer 2011: PAPERS.md).

Random numbers: momenta, accept uniforms and swap uniforms as tempering.run_tempered draws them (the same seed and key-domain rules);
the shifts of iteration t come from a stream of their own key domain, (shift_seed(seed), GLOBAL chain id, t), as floor(U[0, 1) L)
formed on the device: a replay of the captured loop draws new ones.

run_ft_ptbc is the same ladder through a flow: the loop runs in the latent field of ftHMC, the defect sits on the
physical field F(x) (ops.ft_defect_trajectory), the swaps read Dsum of the physical field.  The coupling layers' stripe masks have
period 4 across the stripes, so the flow commutes with the translations by multiples of 4 in both directions and with no others: the
shifts there are 4 floor(U[0, 1) L / 4), from the same stream.
"""
from __future__ import annotations

from math import pi as PI
from typing import Optional, Sequence

import numpy as np
import torch

from . import ops
from .config import DTYPE, Param, device
from .graph_loop import GraphLoop, LazyHistory, Row
from .parallel import shard_range, world
from .tempering import _SEED_MASK, init_seed, round_trips, swap_seed

SHIFT_DOMAIN = 0x53484654 << 20         # 'SHFT'


def shift_seed(seed: int) -> int:
    """the seed of the translation-shift stream of a run: key (shift_seed(seed), global chain id, iteration)"""
    return (int(seed) + SHIFT_DOMAIN + 5) & _SEED_MASK


def default_defect(L: int) -> tuple:
    return (0, 0, max(1, int(L) // 4))


def run_ptbc(param: Param, cs: Sequence[float], n_ladders: int, ntraj: int, defect=None, swap_every: int = 1, translate: bool = True,
             integrator: str = 'leapfrog', seed: Optional[int] = None, x: Optional[torch.Tensor] = None, captured: bool = True,
             shard=None):
    """PTBC of `n_ladders` ladders over the defect couplings param.beta * cs (cs strictly increasing in [0, 1], ending at 1) for
    `ntraj` trajectories of param.tau / param.nstep.  defect = (i0, j0, Ld), default (0, 0, max(1, L // 4)).  One iteration: momenta
    and uniforms -> one trajectory of all chains (ops.defect_trajectory, path 0) -> every `swap_every`-th iteration one swap round on
    Dsum, parities alternating -> the translation of the top rung (translate).

    x, shard, captured: as tempering.run_tempered takes them; the captured and the eager run give bit-equal histories.

    -> history (read back lazily), every series sorted BY RUNG: 'plaq' (sum cos P / L^2), 'Q' (the integer charge: it has a meaning on
    rung K - 1), 'acc', 'dH' and 'dsum' (the defect's sum of cos P, what the swaps read) [ntraj, K, M_local]; 'swap_acc' [K - 1]
    acceptance per neighbouring pair, 'swap_tried' [K - 1] and 'swap_rounds' [ntraj, M_local, K - 1] the rounds themselves (1, 0, or -1:
    not tried); 'rung' [ntraj, B_local] the rung each chain ran on; 'round_trips' [B_local]; 'cs' and 'defect' as the run used them;
    'x' the final fields, 'g_b' / 'rung_last' their ladder positions (run_tempered's 'beta_b' / 'rung_last')."""
    return _run(param, None, cs, n_ladders, ntraj, defect, swap_every, translate, integrator, seed, x, captured, shard, 'silu')


def run_ft_ptbc(param: Param, flow, cs: Sequence[float], n_ladders: int, ntraj: int, defect=None, swap_every: int = 1,
                translate: bool = True, integrator: str = 'leapfrog', seed: Optional[int] = None, x: Optional[torch.Tensor] = None,
                captured: bool = True, shard=None, act: str = 'silu'):
    """run_ptbc through a flow: field-transformation HMC whose PHYSICAL field F(x) carries the defect (ops.ft_defect_trajectory,
    DESIGN 4.19).  flow: an nn.ModuleList of coupling layers (its weights through utils.layers.flow_weights; act: their activation);
    an empty one is run_ptbc's sequenced trajectory.  The loop runs in the latent field; the swaps are ops.replica_swap on Dsum of the
    physical field; the translation of the top rung is ops.defect_translate on the latent field by multiples of 4 in both directions,
    the translations the flow commutes with.  A translation changes Dsum of the translated chains: with translate=True every trajectory
    evaluates its own start, with translate=False the g-free state [4, B] is carried from trajectory to trajectory (bit-equal).

    -> run_ptbc's history; 'plaq', 'Q', 'acc', 'dH', 'dsum' are of the PHYSICAL field, 'x' is the final LATENT field."""
    if flow is None:
        raise ValueError('run_ft_ptbc: a flow (a list of coupling layers, possibly empty) expected; run_ptbc is the driver without one')
    return _run(param, flow, cs, n_ladders, ntraj, defect, swap_every, translate, integrator, seed, x, captured, shard, act)


def _run(param, flow, cs, n_ladders, ntraj, defect, swap_every, translate, integrator, seed, x, captured, shard, act):
    """the one loop behind run_ptbc (flow None) and run_ft_ptbc"""
    ops.integrator_code(integrator)
    cl = [float(c) for c in cs]
    K, M_all = len(cl), int(n_ladders)
    if K < 2 or any(not (cl[k] < cl[k + 1]) for k in range(K - 1)) or cl[0] < 0.0 or cl[-1] != 1.0:
        raise ValueError(f'cs: at least two strictly increasing values in [0, 1] that end at 1 expected, got {cl}')
    if M_all < 1 or ntraj < 1 or swap_every < 1:
        raise ValueError('n_ladders, ntraj and swap_every must be >= 1')
    L, beta = param.L, float(param.beta)
    df = default_defect(L) if defect is None else tuple(int(t) for t in defect)
    if len(df) != 3 or not (0 <= df[2] <= L and 0 <= df[0] < L and 0 <= df[1] < L):
        raise ValueError(f'defect: (i0, j0, Ld) with 0 <= Ld <= L = {L} and 0 <= i0, j0 < L expected, got {defect!r}')
    rank, wsz = (world()[:2] if shard is None else (int(shard[0]), int(shard[1])))
    lo, hi = shard_range(M_all * K, rank, wsz)
    B = hi - lo
    if B < K or B % K != 0 or lo % K != 0:
        raise ValueError(f'rank {rank} of {wsz}: chains [{lo}, {hi}) do not form whole ladders of {K} rungs (ladders never span ranks)')
    M, ladder_lo = B // K, lo // K
    seed = int(param.seed if seed is None else seed)
    dev = device() if x is None else x.device
    dt, nstep = param.tau / param.nstep, param.nstep
    if flow is not None:
        ops.act_code(act)
        nl = len(flow)
        if nl:
            from .utils.layers import flow_weights
            wflow = flow_weights(flow, dev).detach()
        else:
            wflow = None

    if x is None:
        xs = torch.zeros(B, 2, L, L, dtype=DTYPE, device=dev)
        if param.randinit:
            ops.random_uniform(ops.chain_seeds(init_seed(seed), lo, B, 0, device=dev), (B, 2, L, L), -PI, PI, out=xs)
    else:
        if tuple(x.shape) != (B, 2, L, L):
            raise ValueError(f'x: expected this shard\'s fields [{B}, 2, {L}, {L}], got {tuple(x.shape)}')
        xs = x.detach().to(DTYPE).contiguous().clone()

    lad = ops.ladder_init([beta * c for c in cl], M, device=dev)         # the ladder of g: g_0 = 0 is a rung like any other
    g_b, rung, chain_of, dg = lad['beta_b'], lad['rung'], lad['chain_of'], lad['betas']
    P = 2 * int(swap_every)                                              # one period: both parities once
    pk = 'csum' if flow is None else 'plaq'                              # what the trajectory hands out: sum cos P, or its mean
    layout = Row(None, acc=B, dH=B, **{pk: B}, dsum=B, Q=B, rung=B, swap_acc=(M, K - 1))   # swap_acc: of the round behind the trajectory
    rows = torch.empty(P, layout.width, dtype=torch.float64, device=dev)
    xn, v = torch.empty_like(xs), torch.empty_like(xs)                   # the trajectory goes xs -> xn, the translation xn -> xs
    u = torch.empty(B, dtype=torch.float64, device=dev)
    us = torch.empty(M, K - 1, dtype=torch.float64, device=dev)
    ush = torch.empty(B, 2, dtype=torch.float64, device=dev)
    shift = torch.zeros(B, 2, dtype=torch.int32, device=dev)
    seeds = torch.empty(B, dtype=torch.int64, device=dev)
    sseeds = torch.empty(M, dtype=torch.int64, device=dev)
    hseeds = torch.empty(B, dtype=torch.int64, device=dev)
    t_cnt = torch.zeros(1, dtype=torch.int64, device=dev)                # trajectories done: the `t` of the chain streams
    r_cnt = torch.zeros(1, dtype=torch.int64, device=dev)                # swap rounds done
    h_cnt = torch.zeros(1, dtype=torch.int64, device=dev)                # translations done
    scratch = {k: torch.empty(B, dtype=torch.float64, device=dev) for k in ('H0', 'H1')}
    dscr = torch.empty(M, K - 1, dtype=torch.float64, device=dev)
    state = torch.empty(4, B, dtype=torch.float64, device=dev) if flow is not None else None
    have_state = [False]                                                 # translate=False: the g-free state is carried

    def one(j: int):
        """trajectory j of a period, the swap round and the translation behind it -> rows[j]"""
        row = layout.over(rows[j])
        out = {'x_new': xn, 'acc': row['acc'], 'dH': row['dH'], pk: row[pk], 'dsum': row['dsum'], 'Q': row['Q'],
               'H0': scratch['H0'], 'H1': scratch['H1']}
        ops.chain_seeds(seed, lo, B, 0, counter=t_cnt, advance=True, out=seeds)
        ops.random_momenta(seeds, (B, 2, L, L), out_v=v, out_u=u)
        if flow is None:
            ops.defect_trajectory(xs, v, u, beta, g_b, df, dt, nstep, integrator=integrator, path=0, out=out)
        else:
            out['state'] = state
            ops.ft_defect_trajectory(xs, v, u, wflow, nl, beta, g_b, df, dt, nstep, act, integrator, out=out,
                                     state_in=state if have_state[0] else None)
            have_state[0] = not translate
        row['rung'].copy_(rung)                                          # the rung this trajectory ran on
        sw = row['swap_acc']
        if (j + 1) % swap_every == 0:
            parity = ((j + 1) // swap_every - 1) % 2
            ops.chain_seeds(swap_seed(seed), ladder_lo, M, 0, counter=r_cnt, advance=True, out=sseeds)
            ops.random_uniform(sseeds, (M, K - 1), 0.0, 1.0, out=us)
            ops.replica_swap(dg, row['dsum'], us, g_b, rung, chain_of, parity, out={'swap_acc': sw, 'd': dscr})
        else:
            sw.fill_(-1.0)
        if translate:
            ops.chain_seeds(shift_seed(seed), lo, B, 0, counter=h_cnt, advance=True, out=hseeds)
            ops.random_uniform(hseeds, (B, 2), 0.0, 1.0, out=ush)
            if flow is None:
                shift.copy_(ush.mul_(float(L)).floor_())                 # floor(U[0, 1) L), on the device
            else:
                shift.copy_(ush.mul_(float(L // 4)).floor_().mul_(4.0))  # 4 floor(U[0, 1) L / 4): what the flow commutes with
            ops.defect_translate(xn, rung, K - 1, shift, out=xs)
        else:
            xs.copy_(xn)

    def period():
        for j in range(P):
            one(j)

    n_full, rem = divmod(int(ntraj), P)
    caller = torch.cuda.current_stream(dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(caller)
    tail = torch.empty(max(rem, 1), layout.width, dtype=torch.float64, device=dev)
    loop = GraphLoop(period, rows, chunk=max(1, 256 // P), use_graph=bool(captured), stream=stream)
    for _ in range(n_full):
        loop.step()
    with torch.cuda.stream(stream):
        for j in range(rem):                                             # what is left of the last period: the same calls, eagerly
            one(j)
            tail[j].copy_(rows[j])
        x_out, gb_out, rung_out = xs.clone(), g_b.clone(), rung.clone()
    loop.join()

    def fill():
        H = loop.rows().reshape(n_full * P, layout.width)
        if rem:
            stream.synchronize()
            H = np.concatenate([H, tail[:rem].cpu().numpy()], axis=0)
        n, c = H.shape[0], layout.split(H)
        rg = np.rint(c['rung']).astype(np.int64)                                          # [n, B]
        # chain on rung k of ladder m at trajectory t: the inverse permutation of rg within every ladder
        order = np.argsort(rg.reshape(n, M, K), axis=2) + (np.arange(M) * K)[None, :, None]   # [n, M, K] -> chain index
        h = {}
        for key in ('acc', 'dH', pk, 'dsum', 'Q'):
            h[key] = np.take_along_axis(c[key], order.reshape(n, B), axis=1).reshape(n, M, K).transpose(0, 2, 1)   # [n, K, M]
        if flow is None:
            h['plaq'] = h.pop('csum') / float(L * L)
        sw = c['swap_acc']
        tried = (sw >= 0).sum(axis=(0, 1))
        h['swap_tried'] = tried
        h['swap_acc'] = np.where(tried > 0, (sw > 0.5).sum(axis=(0, 1)) / np.maximum(tried, 1), np.nan)
        h['swap_rounds'] = sw
        h['rung'] = rg
        h['round_trips'] = round_trips(rg, K)
        h['cs'], h['defect'] = np.array(cl), df
        h['x'], h['g_b'], h['rung_last'] = x_out, gb_out, rung_out
        return h
    return LazyHistory(fill)
