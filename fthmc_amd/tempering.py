"""Replica exchange (parallel tempering) over a beta ladder: tempered HMC and tempered ftHMC in ONE batch.

K replicas at beta_0 < ... < beta_{K-1} form a ladder; M ladders of K consecutive chains are one batch of B = M K chains that a
single per-chain-beta trajectory call moves (ops.ft_trajectory with a beta TENSOR: C ABI fthmc_ft_trajectory_pb_v), at the
occupancy of an untempered batch of the same size.  Every `swap_every`-th trajectory a swap round (ops.replica_swap, kernel
k_replica_swap) offers the exchange of neighbouring rungs, pairs (0,1),(2,3).. and (1,2),(3,4).. in alternation.  With ONE flow
shared by all rungs the acceptance needs no flow evaluation: for chain a on rung k and c on rung k + 1

    A = min(1, exp((beta_k - beta_{k+1}) (C_c - C_a))),     C = sum cos P(F(x))

and C is row 1 of the beta-free state every trajectory already carries.  An exchange swaps the two chains' beta, rung and
chain_of entries on the device; fields never move, so a captured loop replays without a host copy.

The reference (nftqcd/fthmc) samples one beta per run and has no counterpart (Swendsen & Wang 1986; Hukushima & Nemoto 1996;
Earl & Deem 2005: PAPERS.md).

Random numbers: momenta and accept uniforms of trajectory t come from the stream (seed, GLOBAL chain id, t) as everywhere
(ops.chain_seeds / ops.random_momenta); the uniforms of swap round r of a ladder come from a stream of their own key domain,
(swap_seed(seed), GLOBAL ladder id, r) -> ops.chain_seeds -> ops.random_uniform(K - 1 values): a ladder's swaps do not depend
on how the ladders are sharded over ranks.
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

# key domains of the driver's own streams: a seed of another domain is the run's seed moved by a fixed odd offset, so the
# (seed, id, counter) triples of the swap uniforms and of the start fields never meet those of the trajectories
SWAP_DOMAIN = 0x53574150 << 20          # 'SWAP'
INIT_DOMAIN = 0x494E4954 << 20          # 'INIT'
_SEED_MASK = (1 << 62) - 1


def swap_seed(seed: int) -> int:
    """the seed of the swap-uniform stream of a run: key (swap_seed(seed), global ladder id, swap round)"""
    return (int(seed) + SWAP_DOMAIN + 1) & _SEED_MASK


def init_seed(seed: int) -> int:
    return (int(seed) + INIT_DOMAIN + 3) & _SEED_MASK


def round_trips(rung: np.ndarray, K: int) -> np.ndarray:
    """Completed round trips bottom -> top -> bottom of every chain from its rung trajectory [ntraj, B] -> [B]."""
    rung = np.asarray(rung)
    trips = np.zeros(rung.shape[1], dtype=np.int64)
    phase = np.zeros(rung.shape[1], dtype=np.int8)                       # 0: waiting for the bottom, 1: left the bottom, 2: reached the top
    for r in rung:
        phase = np.where((phase == 0) & (r == 0), 1, phase)
        phase = np.where((phase == 1) & (r == K - 1), 2, phase)
        done = (phase == 2) & (r == 0)
        trips += done
        phase = np.where(done, 1, phase)
    return trips


def run_tempered(param: Param, flow, betas: Sequence[float], n_ladders: int, ntraj: int, swap_every: int = 1,
                 integrator: str = 'leapfrog', seed: Optional[int] = None, x: Optional[torch.Tensor] = None, captured: bool = True,
                 shard=None, groups: int = 1):
    """Tempered HMC (flow None: the plain Wilson MD, the flowed sequence with zero layers) or tempered ftHMC (flow: an
    nn.ModuleList of coupling layers, or their per-layer weight tuples as ops.pack_weights takes them, shared by every rung) of
    `n_ladders` ladders over `betas` (strictly increasing) for `ntraj`
    trajectories of param.tau / param.nstep; param.beta is not read.  One iteration: momenta and uniforms -> one per-chain-beta
    trajectory of all chains -> every `swap_every`-th iteration one swap round, parities alternating.

    x: the start fields of THIS shard's chains [B_local, 2, L, L] (default: param's initializer per chain -- zeros, or U(-pi, pi)
    keyed by the global chain id with param.randinit).  shard: (rank, world_size), default the torchrun environment; ladders are
    whole on a rank (else ValueError) and keep their global ids; no collective is issued.  captured: the first period
    (2 swap_every iterations) runs eagerly and is then captured in a hipGraph (graph_loop.capture), every later period is a replay
    and what is left of the last one runs eagerly; False runs the same calls eagerly throughout -- the histories are bit-equal.

    -> history (read back lazily), every series sorted BY RUNG: 'plaq', 'Q', 'acc', 'dH' [ntraj, K, M_local]; 'swap_acc'
    [K - 1] acceptance per neighbouring pair and 'swap_tried' [K - 1]; 'rung' [ntraj, B_local] the rung each chain ran on;
    'round_trips' [B_local]; 'betas'; 'x' the final fields, 'beta_b' / 'rung_last' their ladder positions."""
    ops.integrator_code(integrator)
    bl = [float(b) for b in betas]
    K, M_all = len(bl), int(n_ladders)
    if K < 2 or any(not (bl[k] < bl[k + 1]) for k in range(K - 1)):
        raise ValueError(f'betas: at least two strictly increasing values expected, got {bl}')
    if M_all < 1 or ntraj < 1 or swap_every < 1:
        raise ValueError('n_ladders, ntraj and swap_every must be >= 1')
    rank, wsz = (world()[:2] if shard is None else (int(shard[0]), int(shard[1])))
    lo, hi = shard_range(M_all * K, rank, wsz)
    B = hi - lo
    if B < K or B % K != 0 or lo % K != 0:
        raise ValueError(f'rank {rank} of {wsz}: chains [{lo}, {hi}) do not form whole ladders of {K} rungs (ladders never span ranks)')
    M, ladder_lo = B // K, lo // K
    seed = int(param.seed if seed is None else seed)
    dev = device() if x is None else x.device
    L = param.L
    nl = 0 if flow is None else len(flow)
    if nl and isinstance(flow, torch.nn.Module):
        from .utils.layers import flow_activation, flow_weights
        w, act = flow_weights(flow, dev).detach(), flow_activation(flow)
    elif nl:                                                             # per-layer weight tuples (ops.pack_weights), silu
        w, act = ops.pack_weights(flow, device=dev), 'silu'
    else:
        w, act = None, 'silu'
    dt, nstep = param.tau / param.nstep, param.nstep

    if x is None:
        xs = torch.zeros(B, 2, L, L, dtype=DTYPE, device=dev)
        if param.randinit:
            ops.random_uniform(ops.chain_seeds(init_seed(seed), lo, B, 0, device=dev), (B, 2, L, L), -PI, PI, out=xs)
    else:
        if tuple(x.shape) != (B, 2, L, L):
            raise ValueError(f'x: expected this shard\'s fields [{B}, 2, {L}, {L}], got {tuple(x.shape)}')
        xs = x.detach().to(DTYPE).contiguous().clone()

    lad = ops.ladder_init(bl, M, device=dev)
    beta_b, rung, chain_of, dbetas = lad['beta_b'], lad['rung'], lad['chain_of'], lad['betas']
    P = 2 * int(swap_every)                                              # one period: both parities once
    layout = Row(None, acc=B, dH=B, plaq=B, Q=B, rung=B, swap_acc=(M, K - 1))     # swap_acc: of the round behind the trajectory
    rows = torch.empty(P, layout.width, dtype=torch.float64, device=dev)
    v = torch.empty_like(xs)
    u = torch.empty(B, dtype=torch.float64, device=dev)
    us = torch.empty(M, K - 1, dtype=torch.float64, device=dev)
    seeds = torch.empty(B, dtype=torch.int64, device=dev)
    sseeds = torch.empty(M, dtype=torch.int64, device=dev)
    t_cnt = torch.zeros(1, dtype=torch.int64, device=dev)                # trajectories done: the `t` of the chain streams
    r_cnt = torch.zeros(1, dtype=torch.int64, device=dev)                # swap rounds done
    state = torch.empty(3, B, dtype=torch.float64, device=dev)
    scratch = {k: torch.empty(B, dtype=torch.float64, device=dev) for k in ('H0', 'H1')}
    dscr = torch.empty(M, K - 1, dtype=torch.float64, device=dev)
    have_state = [False]

    def one(j: int):
        """trajectory j of a period (and the swap round behind it) -> rows[j]"""
        row = layout.over(rows[j])
        out = {'x_new': xs, 'acc': row['acc'], 'dH': row['dH'], 'plaq': row['plaq'], 'Q': row['Q'], 'state': state,
               'H0': scratch['H0'], 'H1': scratch['H1']}
        ops.chain_seeds(seed, lo, B, 0, counter=t_cnt, advance=True, out=seeds)
        ops.random_momenta(seeds, (B, 2, L, L), out_v=v, out_u=u)
        ops.ft_trajectory(xs, v, u, w, nl, beta_b, dt, nstep, act, mode='md', out=out, state_in=state if have_state[0] else None,
                          groups=groups, integrator=integrator)
        have_state[0] = True
        row['rung'].copy_(rung)                                          # the rung this trajectory ran on
        sw = row['swap_acc']
        if (j + 1) % swap_every == 0:
            parity = ((j + 1) // swap_every - 1) % 2
            ops.chain_seeds(swap_seed(seed), ladder_lo, M, 0, counter=r_cnt, advance=True, out=sseeds)
            ops.random_uniform(sseeds, (M, K - 1), 0.0, 1.0, out=us)
            ops.replica_swap(dbetas, state[1], us, beta_b, rung, chain_of, parity, out={'swap_acc': sw, 'd': dscr})
        else:
            sw.fill_(-1.0)

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
        x_out, bb_out, rung_out = xs.clone(), beta_b.clone(), rung.clone()
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
        for key in ('acc', 'dH', 'plaq', 'Q'):
            h[key] = np.take_along_axis(c[key], order.reshape(n, B), axis=1).reshape(n, M, K).transpose(0, 2, 1)   # [n, K, M]
        sw = c['swap_acc']
        tried = (sw >= 0).sum(axis=(0, 1))
        h['swap_tried'] = tried
        h['swap_acc'] = np.where(tried > 0, (sw > 0.5).sum(axis=(0, 1)) / np.maximum(tried, 1), np.nan)
        h['swap_rounds'] = sw
        h['rung'] = rg
        h['round_trips'] = round_trips(rg, K)
        h['betas'] = np.array(bl)
        h['x'], h['beta_b'], h['rung_last'] = x_out, bb_out, rung_out
        return h
    return LazyHistory(fill)
