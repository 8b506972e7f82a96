#!/usr/bin/env python3
"""Generate tests/golden/steep_inverse.npz: the coupling layer's tan-mixture map and its inverse on STEEP flows, |s| of 2 .. 20,
from mpmath at 40 digits.  Needs mpmath and oracle/ref_cpu.py only (no reference project, no GPU).

    cd <repo> && python tests/golden/make_golden_steep.py

Weights: one default_flow draw; per case the last conv's bias is overwritten, b3[k] = sign_k * s0 for the s channels and
b3[K] = 0.7 for t, so that s_k = +-s0 + O(0.3) varies by site and t moves the targets across the wrap.
Cases: s0 in {2, 5, 10} x signs (+,+), (+,-), (-,-), and the sanity case s0 = 20, (+,-).

Plaquette fields P[B=2][L][L] are uniform in (-pi, pi), one draw per L, with planted values 0, +-1e-12, +-1e-6, +-(pi - d) on
sites that are active for both directions (i % 4 == j % 4); d is the smallest value that keeps the condition below at the planted
sites of every case with that s0 (s0 = 20: at least 1e-4).

Condition (asserted here, not measured on any kernel): e^{|s_k|} |tan(P/2)| <= 1e13 at every active site and component.  Above
that 2 atan(.) rounds to exactly pi in fp64 and wraps to -pi: the reference's own mixture mean is discontinuous there.

What is stored (fP, fp, logJ, labs, sens and y are computed at 40 digits on the oracle's fp64 s, t and rounded once):
  w0..w5, case_s0[C], case_sign[C, 2], P_L{L}[S, B, L, L] (S = the s0 values 2, 5, 10, 20)
  per L a table combo_L{L}[n, 3] = (case, mu, off) and, at the active sites in row-major order (b, i, j):
      fP    wrap(mean_k y_k + t)                         [n, B, na]
      fp    mean_k 1 / D_k (the map's slope dfP/dP)      [n, B, na]  (L = 32: float32 rounded UP, it only divides a tolerance)
      logJ  sum of log fp                                [n, B]
      labs  sum of |log fp|                              [n, B]
      sens  sum of |d log fp / dP| / fp                  [n, B]   sensitivity of log J to an error in y-space
      L = 16 also s[n, B, K, na], t[n, B, na] (oracle conv_net, fp64) and y[n, B, K, na]
  link-level cases (the kernels without a plaquette-level entry), link{c}_*: x [B, 2, L, L] with |P| < pi, P = R.plaq(x), meta =
      (case, L, mu, off), yl (the updated links on the active stripe), fp, logJ, labs, sens
  generic-net cases (n_mix 1 and 3, hidden [4]) at L = 16: their weights and the same quantities as the L = 16 table
  delta_ref[S]: max over active sites of |oracle fp64 forward - mpmath forward|, the reference's own noise floor per s0.

The file regenerates bit for bit (tests/test_steep_reference.py) wherever PyTorch's CPU kernels give the same bits for the oracle's
conv_net: independent of the number of threads, not of the instruction set its conv / cos / sin kernels are dispatched to (as the
fixtures of make_golden.py).
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, 'steep_inverse.npz')

S0 = (2.0, 5.0, 10.0, 20.0)
CASES = [(s0, sg) for s0 in S0[:3] for sg in ((1, 1), (1, -1), (-1, -1))] + [(20.0, (1, -1))]
MU_OFF = {32: [(mu, off) for mu in (0, 1) for off in range(4)], 20: [(0, 1), (1, 2)], 16: [(0, 3), (1, 0)]}
COND = 1e13
B = 2
# generic nets: (n_mix, s0, signs, (mu, off)); link-level cases: (case, L, (mu, off))
GENERIC = [(1, 5.0, (1,), (0, 2)), (1, 10.0, (-1,), (1, 1)), (3, 5.0, (1, -1, 1), (1, 3)), (3, 10.0, (-1, 1, -1), (0, 0))]
LINK_PLANTED = (0.0, 2.0 ** -40, -2.0 ** -40, 2.0 ** -20, -2.0 ** -20)        # on the links' 2^-40 grid
LINK = [(ci, (16, 20)[ci % 2], ((0, 1, 0, 1)[ci % 4], (ci * 3 + 1) % 4)) for ci in range(len(CASES))]


def planted_sites(L):
    """[(b, i, j)] x 4 per planted value m = 0..6: i % 4 == j % 4 == r, so that each value is active for (0, r) and (1, r)."""
    out = []
    for m in range(7):
        b, q = (0, m) if m < 4 else (1, m - 4)
        out.append([(b, (4 * q + r) % L, (4 * ((3 * q + 1) % (L // 4)) + r) % L) for r in range(4)])
    return out


def planted_values(d):
    return [0.0, 1e-12, -1e-12, 1e-6, -1e-6, math.pi - d, -(math.pi - d)]


def plant(P0, d):
    P = P0.clone()
    for sites, v in zip(planted_sites(P.shape[-1]), planted_values(d)):
        for (b, i, j) in sites:
            P[b, i, j] = v
    return P


def case_weights(base, s0, signs):
    w = [t.clone() for t in base]
    K = len(signs)
    for k in range(K):
        w[-1][k] = signs[k] * s0
    w[-1][K] = 0.7
    return tuple(w)


def net_st(R, P, w, mu, off):
    """s [B, K, na], t [B, na] of the oracle's fp64 conv_net at the active sites, and the active mask"""
    import torch
    L = P.shape[-1]
    mA, mF, _, _ = R.stripe_masks(L, mu, off)
    x2 = mF * P
    out = R.conv_net(torch.stack((torch.cos(x2), torch.sin(x2)), dim=1), w)
    act = mA.bool()
    return out[:, :-1][:, :, act].numpy(), out[:, -1][:, act].numpy(), act


def mp_forward(mp, Pa, s, t):
    """mpmath at the working precision on fp64 inputs Pa [B, na], s [B, K, na], t [B, na] ->
    dict of fp64 arrays y [B, K, na], fP, fp [B, na] and logJ, labs, sens [B]"""
    Bn, K, na = s.shape
    y = np.empty((Bn, K, na)); fP = np.empty((Bn, na)); fp = np.empty((Bn, na))
    logJ = np.empty(Bn); labs = np.empty(Bn); sens = np.empty(Bn)
    pi, two_pi = mp.pi, 2 * mp.pi
    for b in range(Bn):
        lj = la = se = mp.mpf(0)
        for a in range(na):
            c, sn = mp.cos_sin(mp.mpf(float(Pa[b, a])) / 2)
            tn, c2, s2, sinP = sn / c, c * c, sn * sn, 2 * sn * c
            ysum = f1 = f2 = mp.mpf(0)
            for k in range(K):
                es = mp.exp(mp.mpf(float(s[b, k, a])))
                ems = 1 / es
                yk = 2 * mp.atan(es * tn)
                D = ems * c2 + es * s2
                ysum += yk
                f1 += 1 / D
                f2 -= (es - ems) * sinP / (2 * D * D)          # d(1 / D_k)/dP
                y[b, k, a] = float(yk)
            f1 /= K; f2 /= K
            v = ysum / K + mp.mpf(float(t[b, a]))
            v -= two_pi * mp.floor((v + pi) / two_pi)          # [-pi, pi)
            fP[b, a] = float(v); fp[b, a] = float(f1)
            lg = mp.log(f1)
            lj += lg; la += abs(lg); se += abs(f2 / f1) / f1
        logJ[b], labs[b], sens[b] = float(lj), float(la), float(se)
    return {'y': y, 'fP': fP, 'fp': fp, 'logJ': logJ, 'labs': labs, 'sens': sens}


def wrapdiff(a, b):
    return (a - b + math.pi) % (2 * math.pi) - math.pi


def f32_up(a):
    """float32 not below the fp64 value (a tolerance divided by it never widens)"""
    r = a.astype(np.float32)
    low = r.astype(np.float64) < a
    r[low] = np.nextafter(r[low], np.float32(np.inf))
    return r


def generate(verbose=False):
    import mpmath as mp
    import torch
    from oracle import ref_cpu as R
    mp.mp.dps = 40
    say = print if verbose else (lambda *a, **k: None)
    gen = torch.Generator().manual_seed(20260417)
    base = R.default_flow(1, gen)[0]
    gen_nets = [case_weights(R.default_flow(1, gen, hidden=(4,), n_mix=K)[0], s0, sg) for (K, s0, sg, _) in GENERIC]
    out = {f'w{pi}': t.numpy().copy() for pi, t in enumerate(base)}
    out['case_s0'] = np.array([c[0] for c in CASES])
    out['case_sign'] = np.array([c[1] for c in CASES], dtype=np.int64)
    delta = np.zeros(len(S0))
    pmax = np.zeros(len(S0))                                        # largest e^{|s|} |tan(P/2)| met, per s0

    def check_cond(P_act, s, si):
        c = np.exp(np.abs(s)) * np.abs(np.tan(P_act / 2))[:, None, :]
        assert c.max() <= COND, (S0[si], c.max())
        pmax[si] = max(pmax[si], c.max())

    def noise(fx_act, fP, si):
        delta[si] = max(delta[si], float(np.abs(wrapdiff(fx_act, fP)).max()))

    # ---- plaquette-level cases
    for L in (32, 20, 16):
        P0 = (torch.rand(B, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi
        fields = []
        for si, s0 in enumerate(S0):
            mine = [c for c in CASES if c[0] == s0]
            # d: smallest value with e^{|s|} cot(d/2) <= COND at the sites planted near +-pi (s there does not depend on the
            # site's own value, and on the other planted sites only at the 1e-3 * d level: one pass at d = 1e-3, then the margin)
            Pt = plant(P0, 1e-3)
            smax = 0.0
            near_pi = [site for sites in planted_sites(L)[5:] for site in sites]
            nets = [(case_weights(base, s0, sg), mo) for (_, sg) in mine for mo in MU_OFF[L]]
            if L == 16:                                             # the generic nets run on this field too
                nets += [(w, g[3]) for w, g in zip(gen_nets, GENERIC) if g[1] == s0]
            for w, (mu, off) in nets:
                mA, mF, _, _ = R.stripe_masks(L, mu, off)
                x2 = mF * Pt
                s_all = R.conv_net(torch.stack((torch.cos(x2), torch.sin(x2)), dim=1), w)[:, :-1]
                if s0 == 20.0:                                      # sanity case: every active site counts, see below
                    smax = max(smax, float(s_all[:, :, mA.bool()].abs().max()))
                for (b, i, j) in near_pi:
                    if mA[i, j] > 0:
                        smax = max(smax, float(s_all[b, :, i, j].abs().max()))
            d = 2 * math.atan(math.exp(smax) / COND) * (1 + 1e-3)
            P = plant(P0, d)
            if s0 == 20.0:
                # pi - |P| >= 1e-4 at every site: the drawn values nearer to +-pi than that move to the planted distance
                d = max(d, 1e-4)
                P = plant(torch.where(P0.abs() > math.pi - d, torch.sign(P0) * (math.pi - d), P0), d)
                assert float((math.pi - P.abs()).min()) >= 1e-4
            fields.append(P)
            say(f'L={L} s0={s0:g}: max|s| at the near-pi sites {smax:.4f}, d = {d:.3e}')
        out[f'P_L{L}'] = torch.stack(fields).numpy()
        combos, rows = [], []
        for ci, (s0, sg) in enumerate(CASES):
            si = S0.index(s0)
            w = case_weights(base, s0, sg)
            for (mu, off) in MU_OFF[L]:
                P = fields[si]
                s, t, act = net_st(R, P, w, mu, off)
                Pa = P[:, act].numpy()
                check_cond(Pa, s, si)
                r = mp_forward(mp, Pa, s, t)
                noise(R.plaq_coupling_forward(P, w, mu, off)[0][:, act].numpy(), r['fP'], si)
                r['s'], r['t'] = s, t
                combos.append((ci, mu, off)); rows.append(r)
        out[f'combo_L{L}'] = np.array(combos, dtype=np.int64)
        keys = ['fP', 'fp', 'logJ', 'labs', 'sens'] + (['s', 't', 'y'] if L == 16 else [])
        for k in keys:
            a = np.stack([r[k] for r in rows])
            out[f'{k}_L{L}'] = f32_up(a) if (k == 'fp' and L == 32) else a

    # ---- link-level cases: x with |P| < pi (links within pi/4).  The links are multiples of 2^-40, so that a plaquette is an
    # exact sum in whatever order a kernel adds its four links (where the map is steep a rounding of P is magnified e^{|s|} times);
    # planted plaquettes 0, +-2^-40 (9.1e-13), +-2^-20 (9.5e-7): one link, its three partners zero
    xs = {}
    for L in (16, 20):
        x = (torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * (math.pi / 4)
        xs[L] = torch.round(x * 2.0 ** 40) / 2.0 ** 40
    for ci, L, (mu, off) in LINK:
        s0, sg = CASES[ci]
        si = S0.index(s0)
        w = case_weights(base, s0, sg)
        x = xs[L].clone()
        for sites, v in zip(planted_sites(L)[:5], LINK_PLANTED):
            for (b, i, j) in sites:
                x[b, 0, i, j] = v; x[b, 1, i, j] = 0.0; x[b, 0, i, (j + 1) % L] = 0.0; x[b, 1, (i + 1) % L, j] = 0.0
        P = R.plaq(x)
        assert float(P.abs().max()) < math.pi - 1e-2 and torch.equal(P, R._plaq_action_order(x))     # exact in either order
        assert all(float(P[b, i, j]) == v for sites, v in zip(planted_sites(L)[:5], LINK_PLANTED)
                   for (b, i, j) in sites)
        s, t, act = net_st(R, P, w, mu, off)
        Pa = P[:, act].numpy()
        check_cond(Pa, s, si)
        r = mp_forward(mp, Pa, s, t)
        noise(R.plaq_coupling_forward(P, w, mu, off)[0][:, act].numpy(), r['fP'], si)
        # the layer's link update in fp64 from the high-precision fP (layers.py:196-202): y = wrap(x +- (fP - P)) on the stripe
        dlt = torch.from_numpy(r['fP']) - P[:, act]
        xl = x[:, mu][:, act]
        yl = R.wrap(dlt + xl) if mu == 0 else R.wrap(-dlt + xl)
        out[f'link{ci}_x'] = x.numpy(); out[f'link{ci}_yl'] = yl.numpy()
        out[f'link{ci}_meta'] = np.array([ci, L, mu, off], dtype=np.int64)
        for k in ('fp', 'logJ', 'labs', 'sens'):
            out[f'link{ci}_{k}'] = r[k]

    # ---- generic nets at L = 16 on the plaquette fields of their s0
    for gi, (K, s0, sg, (mu, off)) in enumerate(GENERIC):
        si = S0.index(s0)
        w = gen_nets[gi]
        P = torch.from_numpy(out['P_L16'][si])
        s, t, act = net_st(R, P, w, mu, off)
        Pa = P[:, act].numpy()
        check_cond(Pa, s, si)
        r = mp_forward(mp, Pa, s, t)
        noise(R.plaq_coupling_forward(P, w, mu, off)[0][:, act].numpy(), r['fP'], si)
        out[f'gen{gi}_meta'] = np.array([K, si, mu, off], dtype=np.int64)
        for pi, tw in enumerate(w):
            out[f'gen{gi}_w{pi}'] = tw.numpy()
        for k in ('fP', 'fp', 'logJ', 'labs', 'sens'):
            out[f'gen{gi}_{k}'] = r[k]

    out['delta_ref'] = delta
    out['cond_max'] = pmax
    for si, s0 in enumerate(S0):
        say(f's0={s0:g}: delta_ref = {delta[si]:.3e}, max e^|s| |tan(P/2)| = {pmax[si]:.3e}')
    return out


def main():
    sys.dont_write_bytecode = True
    d = generate(verbose=True)
    np.savez_compressed(OUT, **d)
    print(f'steep_inverse: {os.path.getsize(OUT) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
