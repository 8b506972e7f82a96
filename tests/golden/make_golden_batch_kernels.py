#!/usr/bin/env python3
"""Generate tests/golden/batch_kernels.npz: what the batch reductions, the Adam step and the per-chain sums must give on the seeded
inputs of tests/batch_kernel_cases.py, from mpmath at 60 digits with every input taken as the exact fp64 value it is, stored rounded
to fp64.  Needs mpmath and numpy only (no reference project, no GPU); the GPU tests read the file and never import mpmath.

  tm [case, 2]               (loss_dkl, ess) of every (B, family) of cases.tm_cases(), in that order
  st [B, round, 3]           the plaq, dH and exp(-dH) sums after each round, B in cases.B_LIST
  adam_idx [n]               the sampled element indices (cases.adam_sample())
  adam_p [mode, step, n], adam_m, adam_v [2, step, n]
                             the chain of fp64 states s_0 = inputs, s_{k+1} = round(exact step of s_k): entry k is the reference
                             of step k + 1 taken FROM THE fp64 STATE s_k (one step's error, nothing carried).  m and v do not see
                             the decoupled decay: mode 2 shares mode 0's
  kin [L, B]                 sum v^2
  act_S, act_plaq [L, set, B], act_Q [L, set, B] (integers), act_margin [L, set]: min distance of a plaquette angle from +-pi

    cd <repo> && python tests/golden/make_golden_batch_kernels.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import batch_kernel_cases as C  # noqa: E402

OUT = os.path.join(HERE, 'batch_kernels.npz')
DPS = 60


def _mp():
    import mpmath as mp
    mp.mp.dps = DPS
    return mp


def tm_reference(mp, logq, logp, f):
    """loss = f mean(logq - logp);  ess = (sum w)^2 / sum w^2 / B, w = exp(logw - max logw)"""
    B = len(logq)
    lw = [mp.mpf(float(a)) - mp.mpf(float(b)) for a, b in zip(logp, logq)]
    m = max(lw)
    w = [mp.exp(t - m) for t in lw]
    s1, s2 = mp.fsum(w), mp.fsum(t * t for t in w)
    return float(mp.mpf(float(f)) * (-mp.fsum(lw)) / B), float(s1 * s1 / s2 / B)


def st_reference(mp, inp):
    tot = [mp.mpf(0)] * 3
    out = []
    for r in range(C.ST_ROUNDS):
        tot[0] += mp.fsum(mp.mpf(float(t)) for t in inp['plaq'][r])
        tot[1] += mp.fsum(mp.mpf(float(t)) for t in inp['dH'][r])
        tot[2] += mp.fsum(mp.exp(-mp.mpf(float(t))) for t in inp['dH'][r])
        out.append([float(t) for t in tot])
    return np.array(out)


def adam_reference_step(mp, p, g, m, v, t0, lr, wd, decoupled):
    """the exact step on fp64 arrays -> (p, m, v) rounded to fp64"""
    b1, b2 = (mp.mpf(b) for b in C.AD_BETAS)
    eps, lr, wd = mp.mpf(C.AD_EPS), mp.mpf(lr), mp.mpf(wd)
    T = int(t0) + 1
    step, bc2s = lr / (1 - b1 ** T), mp.sqrt(1 - b2 ** T)
    po, mo, vo = np.empty_like(p), np.empty_like(p), np.empty_like(p)
    for i in range(p.size):
        pi, gi, mi, vi = mp.mpf(float(p[i])), mp.mpf(float(g[i])), mp.mpf(float(m[i])), mp.mpf(float(v[i]))
        if wd != 0:
            if decoupled:
                pi = pi * (1 - lr * wd)
            else:
                gi = gi + wd * pi
        mi = mi + (gi - mi) * (1 - b1)
        vi = vi * b2 + (1 - b2) * gi * gi
        po[i] = float(pi - step * mi / (mp.sqrt(vi) / bc2s + eps))
        mo[i], vo[i] = float(mi), float(vi)
    return po, mo, vo


def adam_reference(mp):
    A = C.adam_master()
    idx = C.adam_sample()
    g = A['g'][idx]
    P = np.zeros((len(C.AD_MODES), C.AD_STEPS, idx.size))
    M = np.zeros((2, C.AD_STEPS, idx.size))
    V = np.zeros_like(M)
    for mode, (wd, dec) in enumerate(C.AD_MODES):
        p, m, v = A['p'][idx], A['m'][idx], A['v'][idx]
        for k in range(C.AD_STEPS):
            p, m, v = adam_reference_step(mp, p, g, m, v, k, C.AD_LR[k], wd, dec)
            P[mode, k] = p
            if mode < 2:
                M[mode, k], V[mode, k] = m, v
            else:
                assert np.array_equal(m, M[0, k]) and np.array_equal(v, V[0, k])
    return idx, P, M, V


def kinetic_reference(mp, v):
    return np.array([float(mp.fsum(mp.mpf(float(t)) ** 2 for t in vb)) for vb in v.reshape(v.shape[0], -1)])


def action_reference(mp, x, beta):
    """-> (S, plaq, Q integer, margin): P = x0[i][j] - x1[i][j] - x0[i][j+1] + x1[i+1][j] exactly, C = sum cos P,
    S = -beta C, plaq = C / L^2, Q = sum wrap(P) / 2 pi (an integer: asserted to 1e-40), margin = min |pi - |wrap(P)||"""
    B, _, L, _ = x.shape
    pi, beta = mp.pi, mp.mpf(beta)
    S, pl, Q, margin = [], [], [], mp.mpf(10)
    for b in range(B):
        x0, x1 = x[b, 0], x[b, 1]
        c = q = mp.mpf(0)
        for i in range(L):
            for j in range(L):
                P = (mp.mpf(float(x0[i, j])) - mp.mpf(float(x1[i, j])) - mp.mpf(float(x0[i, (j + 1) % L])) +
                     mp.mpf(float(x1[(i + 1) % L, j])))
                w = P - 2 * pi * mp.floor((P + pi) / (2 * pi))
                margin = min(margin, pi - abs(w))
                c += mp.cos(P)
                q += w
        q = q / (2 * pi)
        assert abs(q - mp.nint(q)) < mp.mpf(10) ** -40
        S.append(float(-beta * c)); pl.append(float(c / (L * L))); Q.append(int(mp.nint(q)))
    return np.array(S), np.array(pl), np.array(Q, dtype=np.int64), float(margin)


def generate(verbose=False):
    mp = _mp()
    say = print if verbose else (lambda *a, **k: None)
    out = {}
    tm = []
    for B, fam in C.tm_cases():
        d = C.tm_inputs(B, fam)
        tm.append(tm_reference(mp, d['logq'], d['logp'], C.TM_F))
    out['tm'] = np.array(tm)
    say('train metrics:', out['tm'].shape)
    out['st'] = np.array([st_reference(mp, C.st_inputs(B)) for B in C.B_LIST])
    idx, P, M, V = adam_reference(mp)
    out['adam_idx'], out['adam_p'], out['adam_m'], out['adam_v'] = idx, P, M, V
    say('adam:', idx.size, 'elements')
    out['kin'] = np.array([kinetic_reference(mp, C.ka_momenta(L)) for L in C.KA_L])
    S, pl, Q, mg = [], [], [], []
    for L in C.KA_L:
        r = [action_reference(mp, C.ka_links(L, kind), C.KA_BETA) for kind in C.KA_SETS]
        S.append([t[0] for t in r]); pl.append([t[1] for t in r]); Q.append([t[2] for t in r]); mg.append([t[3] for t in r])
    out['act_S'], out['act_plaq'], out['act_Q'], out['act_margin'] = np.array(S), np.array(pl), np.array(Q), np.array(mg)
    say('charges:', out['act_Q'].reshape(len(C.KA_L), -1).tolist())
    return out


def main():
    out = generate(verbose=True)
    np.savez_compressed(OUT, **out)
    print(f'{os.path.basename(OUT)}: {os.path.getsize(OUT) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
