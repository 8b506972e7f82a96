"""A device loop without the host in it: the enqueue-only sequence of one iteration is captured ONCE in a hipGraph and
replayed; what an iteration reports is one row of doubles that is copied into a device ring behind every replay and comes
to the host when somebody looks.

This is how the reference-shaped drivers run at the speed of the benchmark: `FieldTransformation.run` (fthmc/ft_hmc.py:272-346)
and `qed_helpers.ft_run` (ipynb/ft_hmc.py:437-487) are Python loops that synchronise with the device several times per
trajectory; here a trajectory costs the host one graph launch and one small copy.  (`train.GraphTrainer` is the same idea
for the training loop.)  What the drivers share on the host is here too: the row's named layout (`Row`), the ring (`RowRing`), the
argument checks, the start field of a batch and the run_hmc-keyed history of a chain loop (`chain_history`).
"""
from __future__ import annotations

import contextlib
import copy
import gc
import os
from math import prod
from typing import Callable, Optional

import numpy as np
import torch

from .config import DTYPE, device


def run_graph_default() -> bool:
    """whether the drivers capture their loop when the caller does not say: on, unless FTHMC_RUN_GRAPH is '' or '0'"""
    return os.environ.get('FTHMC_RUN_GRAPH', '1') not in ('', '0')


class Row:
    """What one iteration of a driver reports: named fields side by side in ONE flat contiguous float64 tensor (`flat`, zeros at
    first), which the loop copies.  `Row(dev, acc=B, dH=B, wloops=(Rmax, Tmax))`: the fields in order, each with its size or shape;
    a field of size 0 (or None: an option not asked for) takes no room.  `row[name]` is the device view of a field in its shape
    (what goes into the `out=` dictionaries of ops), `split` takes host rows apart by the same offsets.  dev = None: the layout
    alone, to be laid `over` tensors of the caller's."""

    def __init__(self, dev, **fields):
        self.fields, self.width = {}, 0                                   # name -> (offset, shape)
        for name, shape in fields.items():
            shape = tuple(int(s) for s in shape) if isinstance(shape, (tuple, list)) else (int(shape or 0),)
            if prod(shape):
                self.fields[name] = (self.width, shape)
                self.width += prod(shape)
        self.flat = None if dev is None else torch.zeros(self.width, dtype=torch.float64, device=dev)

    def __getitem__(self, name) -> torch.Tensor:
        o, shape = self.fields[name]
        return self.flat[o:o + prod(shape)].view(shape)

    def over(self, flat: torch.Tensor) -> "Row":
        """the same layout over another flat tensor of this width (one line of a [P, width] block)"""
        r = copy.copy(self)
        r.flat = flat
        return r

    def split(self, rows) -> dict:
        """rows [n, width] (or one row), numpy or torch -> {name: [n, *shape]} (views)"""
        rows = rows.reshape(-1, self.width)
        return {name: rows[:, o:o + prod(shape)].reshape((-1,) + shape) for name, (o, shape) in self.fields.items()}


class RowRing:
    """The rows of every iteration so far: `push` copies one on the device (current stream) into slot n % chunk of a [chunk, width]
    tensor, which goes to the host whenever it is full.  The owner synchronises its stream before it reads `rows()`."""

    def __init__(self, width: int, chunk: int, dev, dtype=torch.float64):
        self.chunk = max(1, int(chunk))
        self.buf = torch.empty(self.chunk, int(width), dtype=dtype, device=dev)
        self.reset()

    def reset(self):
        self.flushed, self.n = [], 0                                      # full chunks on the host (numpy), rows pushed

    def push(self, row: torch.Tensor):
        self.buf[self.n % self.chunk].copy_(row.reshape(-1))
        self.n += 1
        if self.n % self.chunk == 0:
            self.flushed.append(self.buf.to('cpu', copy=True).numpy())    # (copy: a ring on the host works too)

    def rows(self) -> np.ndarray:
        """[n, width] on the host"""
        return np.concatenate(self.flushed + [self.buf[:self.n % self.chunk].cpu().numpy()], axis=0)


@contextlib.contextmanager
def capture(graph: "torch.cuda.CUDAGraph", stream: "torch.cuda.Stream"):
    """`torch.cuda.graph(graph, stream=stream, capture_error_mode='thread_local')` with Python's cyclic garbage collector held
    off until the capture has ended.  An automatic collection that starts in the capturing thread may finalise an object left
    over from earlier work -- an older captured graph with its memory pool, a stream, an event -- whose destructor calls into the
    HIP runtime (hipGraphExecDestroy, hipFree, ...): not permitted while this thread captures, and an error inside a destructor
    ends the process (seen once: `Fatal Python error: Aborted`, `Garbage-collecting`, under the `enqueue` of a re-capture).
    torch.cuda.graph collects once on entry; what becomes garbage during the capture waits for its end.  thread_local: another
    thread (a process group's watchdog) may go on calling the runtime."""
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph, stream=stream, capture_error_mode='thread_local'):
            yield
    finally:
        if was_enabled:
            gc.enable()


class GraphLoop:
    """`enqueue()` must only enqueue device work on the current stream (no host synchronisation, no allocation that
    changes between iterations) and leave the iteration's results in `row` (a contiguous float64 device tensor).

    The first `step()` runs the sequence eagerly (allocator, workspaces), then captures it -- the capture does not execute,
    so n calls of `step()` are exactly n iterations, with the same random draws as n eager ones (torch's generator takes
    part in the capture).  `stream`: the stream the loop runs on (default: a new one); an owner that re-captures often hands
    in the same one every time.

    `extra` (optional): a second enqueue-only sequence that runs behind `enqueue` in every iteration whose number is a multiple of
    `extra_every` (a measurement that is not wanted after every trajectory), captured in a graph of its own; it writes into `row`
    too, whose entries keep their last values in the iterations between."""

    def __init__(self, enqueue: Callable[[], None], row: torch.Tensor, chunk: int = 256, use_graph: bool = True,
                 stream: Optional[torch.cuda.Stream] = None, extra: Optional[Callable[[], None]] = None, extra_every: int = 1):
        self.enqueue, self.row = enqueue, row
        self.extra, self.extra_every, self.extra_graph = extra, max(1, int(extra_every)), None
        self.dev = row.device
        self.ring = RowRing(row.numel(), chunk, self.dev, row.dtype)
        self.graph, self.use_graph = None, bool(use_graph)
        self.stream = stream if stream is not None else torch.cuda.Stream(device=self.dev)
        self.stream.wait_stream(torch.cuda.current_stream(self.dev))

    @property
    def captured(self) -> bool:
        return self.graph is not None

    def _capture(self, sequence):
        g = torch.cuda.CUDAGraph()
        with capture(g, self.stream):
            sequence()
        return g

    def step(self):
        measure = self.extra is not None and self.ring.n % self.extra_every == 0
        with torch.cuda.stream(self.stream):
            if self.graph is not None:
                self.graph.replay()
                if measure:
                    self.extra_graph.replay()
            else:
                self.enqueue()
                if measure:
                    self.extra()
                if self.use_graph:                # iteration 0 of a fresh loop (always a measured one) has run: capture the rest
                    self.stream.synchronize()
                    self.graph = self._capture(self.enqueue)
                    self.extra_graph = self._capture(self.extra) if self.extra is not None else None
            self.ring.push(self.row)

    def rows(self) -> np.ndarray:
        """[iterations, row] of every iteration so far, on the host (synchronises)"""
        self.stream.synchronize()
        return self.ring.rows()

    def reset_history(self):
        self.stream.synchronize()
        self.ring.reset()

    def join(self):
        """the caller's current stream waits for everything enqueued so far"""
        torch.cuda.current_stream(self.dev).wait_stream(self.stream)


def loops_arg(loops, L: int):
    """loops = None | n | (Rmax, Tmax) -> None | (Rmax, Tmax) with 1 <= Rmax, Tmax <= L"""
    if loops is None:
        return None
    Rmax, Tmax = (int(loops), int(loops)) if isinstance(loops, int) else (int(loops[0]), int(loops[1]))
    if not (1 <= Rmax <= L and 1 <= Tmax <= L):
        raise ValueError(f'loops: (Rmax, Tmax) with 1 <= Rmax, Tmax <= L = {L} expected, got {loops!r}')
    return Rmax, Tmax


def instanton_arg(k, who: str = '') -> int:
    """the number of instanton hits per trajectory, 0 .. 1024 (`who`: the driver the message names)"""
    k = int(k)
    if not 0 <= k <= 1024:
        raise ValueError((f'{who}: ' if who else '') + f'instanton: a number of hits in 0 .. 1024 expected, got {k}')
    return k


def batched_start(param, x) -> torch.Tensor:
    """the start field of every run, [B, 2, L, L] on the device: x ([2, L, L] or a batch), default param.initializer()"""
    x0 = param.initializer() if x is None else x
    return (x0 if x0.dim() == 4 else x0[None]).to(device=device(), dtype=DTYPE).contiguous()


def chain_history(first: int, dt: float, q0, cols: dict, wloops=None, loops_every: int = 1, late: dict = None) -> dict:
    """The history of one run of a chain loop in run_hmc's shape, {key: [one entry per trajectory]}: 'traj' (first, first + 1, ..),
    'dt', then `cols` in their order -- host series [ntraj, B] (an entry: a CPU tensor made from a copy) or plain lists (as they
    are) -- with 'dq' = sqrt((q - q_previous)^2) behind 'q' (q0 before the first); 'wloops' [ntraj, Rmax, Tmax] gives an entry for
    every `loops_every`-th trajectory; the keys of `late` (series as `cols`) exist once a trajectory has been recorded."""
    def entries(col):
        return [torch.from_numpy(r.copy()) for r in col] if isinstance(col, np.ndarray) else list(col)
    q = cols['q']
    history = {'traj': list(range(first, first + len(q))), 'dt': [dt] * len(q)}
    for key, col in cols.items():
        history[key] = entries(col)
        if key == 'q':
            history['dq'] = entries(np.sqrt((q - np.concatenate([q0[None], q[:-1]])) ** 2))
    if len(q):
        history.update({'wloops': entries(wloops[::loops_every])} if wloops is not None else {})
        history.update({key: entries(col) for key, col in (late or {}).items()})
    return history


class LazyHistory(dict):
    """The history dict of a captured run: {metric: [per-trajectory tensors]} as the eager loop builds it, filled from the
    device ring the first time anybody looks -- `run()` itself returns when everything is ENQUEUED."""

    def __init__(self, fill):
        super().__init__()
        self._fill_fn = fill

    def _fill(self):
        if self._fill_fn is not None:
            fn, self._fill_fn = self._fill_fn, None
            super().update(fn())

    # every way of looking at, copying or changing a dict fills first: a caller written against the reference's plain history dict
    # (ft_hmc.py:272-346) never sees (or overwrites) an empty one
    def __getitem__(self, k): self._fill(); return super().__getitem__(k)
    def __setitem__(self, k, v): self._fill(); return super().__setitem__(k, v)
    def __delitem__(self, k): self._fill(); return super().__delitem__(k)
    def __contains__(self, k): self._fill(); return super().__contains__(k)
    def __iter__(self): self._fill(); return super().__iter__()
    def __reversed__(self): self._fill(); return super().__reversed__()
    def __len__(self): self._fill(); return super().__len__()
    def __bool__(self): self._fill(); return super().__len__() > 0
    def __or__(self, other): self._fill(); return dict(super().items()) | dict(other)
    def __ror__(self, other): self._fill(); return dict(other) | dict(super().items())
    def __ior__(self, other): self._fill(); super().update(other); return self
    def get(self, k, d=None): self._fill(); return super().get(k, d)
    def keys(self): self._fill(); return super().keys()
    def values(self): self._fill(); return super().values()
    def items(self): self._fill(); return super().items()
    def setdefault(self, k, d=None): self._fill(); return super().setdefault(k, d)
    def pop(self, *a): self._fill(); return super().pop(*a)
    def popitem(self): self._fill(); return super().popitem()
    def update(self, *a, **kw): self._fill(); return super().update(*a, **kw)
    def clear(self): self._fill_fn = None; return super().clear()
    def copy(self): self._fill(); return dict(super().items())
    def __repr__(self): self._fill(); return super().__repr__()
    def __eq__(self, other): self._fill(); return super().__eq__(other)
    __hash__ = None
    def __reduce__(self): self._fill(); return (dict, (dict(super().items()),))     # pickles / copies as the plain dict it stands for
