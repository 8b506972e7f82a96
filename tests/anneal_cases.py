"""The numpy side of the annealing tests (tests/test_anneal.py, tests/test_z_anneal_gpu.py): a twin of fthmc_anneal
(include/fthmc_hip.h, fthmc_amd/csrc/local.hip) made of the twins that exist -- the class update of
tests/local_update_cases.py for the sweeps, the chain sum of tests/instanton_cases.py for C = sum cos P -- with the bound of the work
derived below, and the shapes, counts and schedules both test files use.

    step k = 0 .. n - 1:   C_k = sum cos P(x_k),   W <- W + (beta_k - beta_{k+1}) C_k,
                           x_{k+1} = x_k after nsweep compound sweeps (n_hb heatbath, n_or overrelaxation) at beta_{k+1}, the heatbath
                           sweeps at the indices sweep0 + k nsweep n_hb + ...
    trace[k] = C_k, k = 0 .. n (the last of the final field)

Not collected as a test (the name does not match test_*.py)."""
import numpy as np

import instanton_cases as IC
import local_update_cases as LC

LD = np.longdouble
U = LC.U
B = 3                                                  # chains of the deterministic device tests, distinct seeds
N_STEP = 3
# a rising step, a ZERO step and a FALLING step
BETAS = (0.5, 2.0, 2.0, 1.25)
COUNTS = ((1, 0, 1), (1, 2, 1), (2, 1, 2), (0, 1, 1))   # (n_hb, n_or, nsweep)
# L = 4: 8 links per class; 12: 72 per class, a ragged second wave; 64 = LU_MAXL: two links per thread; 68: the sequenced path only
SHAPES = (4, 8, 12, 64, 68)
LU_MAXL = 64
SWEEP0 = 5


def cases():
    """(L, (n_hb, n_or, nsweep)) of the device tests: every count triple on the small lattices, one on the two large ones"""
    return [(L, c) for L in SHAPES for c in (COUNTS if L < 64 else COUNTS[2:3])]


def fields(L, nb=B):
    x = LC.uniform_links(nb, L, 7000 + L)
    seeds = LC.chain_seeds(nb, 7100 + L)
    work = np.random.default_rng(7200 + L).normal(0.0, 30.0, nb)
    for a in (x, seeds, work):
        a.setflags(write=False)
    return x, seeds, work


def lu_threads(L):
    """csrc/local.hip: the workgroup of a chain in the annealing kernels"""
    return min(1024, (L * L // 2 + 63) // 64 * 64)


def cos_sum(x, dt=LD):
    """C = sum cos P per chain and the bound dC of the device's error of it (IC.sums: the same P, ft_sincos, a sum of V terms)
    -> (C [B] in dt, dC [B])"""
    C, _, dC, _ = IC.sums(np.asarray(x, dtype=np.float64), dt)
    return C, 1.01 * dC


def work_steps(betas, C, dC, w0):
    """The work of a ramp from the sums C[k] (k = 0 .. n - 1, each [B]) of its fields -> (W [B] in longdouble, bound [B]).
    The device forms d = fl(beta_k - beta_{k+1}), t = fl(d C~_k), W = fl(W + t) with |C~_k - C_k| <= dC_k: per step
        |d| dC_k                  the sum itself,
        u |d C_k| + u |d C_k|     the roundings of the difference (relative u, times C) and of the product,
        u |W_{k+1}|               the rounding of the sum;
    first order, 1 % on top for the second."""
    W = np.asarray(w0, dtype=LD).copy()
    bound = np.zeros(W.shape)
    for k in range(len(betas) - 1):
        d = LD(betas[k]) - LD(betas[k + 1])
        t = d * np.asarray(C[k], dtype=LD)
        W = W + t
        bound += abs(float(d)) * np.asarray(dC[k]) + 2 * U * np.abs(t.astype(np.float64)) + U * np.abs(W.astype(np.float64))
    return W, 1.01 * bound


def run(x, betas, seeds, n_hb=1, n_or=0, nsweep=1, sweep0=0, work_in=None):
    """The whole call in the twin's arithmetic, the fields rounded to float64 after every class as the device stores them
    -> dict(x [B, 2, L, L] float64, work [B] longdouble, work_bound [B], trace [B, n + 1] longdouble, dtrace [B, n + 1], fields:
    x_0 .. x_n).  (The work's bound holds for a device whose fields ARE the twin's: the device tests take the sums of the
    device's own fields instead.)"""
    x = np.asarray(x, dtype=np.float64)
    nb, n = x.shape[0], len(betas) - 1
    fields_, C, dC = [x], [], []
    sweep = int(sweep0)
    for k in range(n):
        c, d = cos_sum(x)
        C.append(c); dC.append(d)
        for _ in range(nsweep):
            for h in range(n_hb + n_or):
                kind = 'hb' if h < n_hb else 'or'
                for mu, p in LC.CLASSES:
                    x = LC.class_update(x, mu, p, kind, betas[k + 1], seeds, sweep)['x'].astype(np.float64)
                if kind == 'hb':
                    sweep += 1
        fields_.append(x)
    c, d = cos_sum(x)
    C.append(c); dC.append(d)
    w0 = np.zeros(nb) if work_in is None else work_in
    W, wb = work_steps(betas, C, dC, w0)
    return dict(x=x, work=W, work_bound=wb, trace=np.stack(C, axis=1), dtrace=np.stack(dC, axis=1), fields=fields_)
