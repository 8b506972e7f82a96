// The coupling layer on DUAL numbers (dual.h) as fused tile kernels: the second-order sweep of the force-norm training step
// (fthmc_train_force_grad, api.hip; ipynb/ft_hmc.py:253-299).  The gradient of sum_b |F_b|^2 with respect to the weights is
// twice the tangent part of the first-order weight gradient taken on the dual field x + eps F (forward over reverse), so a
// training step needs one forward sweep and one backward sweep of every layer on (value, tangent) pairs.  flow_generic.hip runs
// them as a dozen plain launches per layer with every activation plane in HBM; here a workgroup owns a tile of one chain and
// everything between the dual link field and the layer's results stays in LDS, as in flow.hip (whose structure this file has:
// k_flow_layer<0> and k_flow_layer<2> on Dual, with a tile small enough for 16-byte planes).
//
//   k_flow_dual<.., false>  forward: plaquette window (tile + 3), (cos, sin) input, conv1 + act on tile + 2, conv2 + act on
//                           tile + 1, conv3 and the tan-mixture transform (flow_transform.h) at the tile's active sites, link
//                           update.  No log J: its tangent is never needed (the backward takes d/d logJ = -1 as a constant).
//                           HBM traffic: the dual links in and out, 32 B per link each way.
//   k_flow_dual<.., true>   backward: recomputes the layer from its input X[l - 1] on tile + halo, then walks the adjoint in
//                           SCATTER form (only the tile's own active sites seed it, so no forward halo is widened): transform
//                           adjoint, conv3^T, conv2^T, conv1^T, the (cos, sin) adjoint.  The tile's partial plaquette-gradient
//                           window goes to gp_part and k_gather_gp_dual sums the windows onto the upstream field in a fixed order.
//                           Weight gradients: only their TANGENT parts, sum_s (gz' h + gz h'), are formed; the threads keep
//                           register tiles of these sums while their workgroup walks (chain, tile) items, and the workgroup
//                           writes ONE 955-entry partial row (k_reduce_gw sums the rows in fixed order: no atomics).
//
// Convolutions run on the fp64 VALU with the weights of the value convolutions (k_pack_weights' layout, wave-uniform addresses ->
// scalar loads): a dual FMA with a constant weight is two v_fma_f64.  Tiles: 8 x 8 and 8 x 16; the backward's register
// count leaves one resident workgroup per CU with either.
#include "common.h"
#include "kernels.h"
#include "flow_common.h"
#include "dual.h"
#include "flow_transform.h"

namespace {

using namespace fthmc;
using namespace fthmc_flow;

template <int TR, int TC> struct DG {
    static_assert(TR % 4 == 0 && TC % 4 == 0 && TR * TC <= 256, "tile origins keep the stripe phase; one thread per tile site");
    static constexpr int C0 = TC + 6, C1 = TC + 4, C2 = TC + 2;                  // window widths
    static constexpr int M0 = (TR + 6) * C0, M1 = (TR + 4) * C1, M2 = (TR + 2) * C2, M3 = TR * TC, NA = M3 / 4;
    // channel-plane strides of the activation windows, in dual numbers: ODD, so that lanes which read the same site of different
    // channels (the weight-gradient stages) fall on different LDS banks -- 144, 240 and 100, 180 are multiples of 4 (x 16 B: 64 B)
    static constexpr int S1 = M1 | 1, S2 = M2 | 1;
    // active site a of the tile: mu = 0 columns off + 4 m, mu = 1 rows off + 4 m (tile origins are multiples of 4)
    __device__ static __forceinline__ void active(int a, int mu, int off, int& r, int& c) {
        if (mu == 0) { r = a / (TC / 4); c = off + 4 * (a - r * (TC / 4)); } else { const int m = a / TC; c = a - m * TC; r = off + 4 * m; }
    }
    __device__ static __forceinline__ int active_index(int r, int c, int mu, int off) {
        return mu == 0 ? r * (TC / 4) + ((c - off) >> 2) : ((r - off) >> 2) * TC + c;
    }
};

// LDS plan (dual numbers)
template <int TR, int TC, bool BWD> struct DSmem {
    using G = DG<TR, TC>;
    static constexpr int P = 0;                              // [M0] plaquette window
    static constexpr int IN = P + G::M0;                     // [2][M0] cos, sin
    static constexpr int H1 = IN + 2 * G::M0;                // [8][M1]
    static constexpr int H2 = H1 + 8 * G::S1;                // [8][M2]
    static constexpr int ST = H2 + 8 * G::S2;                // [3][NA] s_0, s_1, t at the active sites
    static constexpr int DL = ST + 3 * G::NA;                // [NA] P' - P                   (fwd)
    static constexpr int D1 = DL + (BWD ? 0 : G::NA);        // [8][M1] act' -> gz1           (bwd)
    static constexpr int D2 = D1 + (BWD ? 8 * G::S1 : 0);    // [8][M2] act' -> gz2
    static constexpr int GO = D2 + (BWD ? 8 * G::S2 : 0);    // [3][M3] g(s_0, s_1, t)
    static constexpr int GP = GO + (BWD ? 3 * G::M3 : 0);    // [M0] partial plaquette gradient
    static constexpr int SIZE = GP + (BWD ? G::M0 : 0);
    static_assert((size_t)SIZE * sizeof(Dual) <= 160 * 1024, "LDS of one CU");
};

// One convolution stage on a window in LDS.  A thread owns NS output sites (slot, slot + 128, ...) and the four output channels of
// its wave's half, and runs the input channels in a ROLLED loop with the nine taps unrolled: a weight is loaded once (wave-uniform
// address: a scalar load) and serves all of the thread's sites -- with the site loop outside, the compiler hoisted every weight of
// the stage out of it and spilled them.
template <int CIN, int MOUT, int COUTW, int OUTP, int MINP, int CINW, bool KEEP_D>
__device__ __forceinline__ void conv_act(const Dual* __restrict__ in, const double* __restrict__ wf, const double* __restrict__ bias,
                                         Dual* __restrict__ sH, Dual* __restrict__ sD, int half, int lane128, int act) {
    constexpr int NS = (MOUT + 127) / 128;
    Dual acc[NS][4];
    int base[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) {
        const int s = min(lane128 + 128 * q, MOUT - 1);                  // a slot past the window recomputes the last site and stores nothing
        const int r = s / COUTW;
        base[q] = r * CINW + (s - r * COUTW);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[q][k] = Dual(bias[half * 4 + k]);
    }
#pragma unroll 1
    for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const double* wp = wf + ((ci * 9 + ky * 3 + kx) * 8 + half * 4);
#pragma unroll
                for (int q = 0; q < NS; ++q) {
                    const Dual v = in[ci * MINP + base[q] + ky * CINW + kx];
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[q][k] = fma(wp[k], v, acc[q][k]);
                }
            }
#pragma unroll
    for (int q = 0; q < NS; ++q) {
        const int s = lane128 + 128 * q;
        if (s < MOUT) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                Dual h, d; act_eval(acc[q][k], act, h, d);
                sH[(half * 4 + k) * OUTP + s] = h;
                if (KEEP_D) sD[(half * 4 + k) * OUTP + s] = d;
            }
        }
    }
}

// The transposed convolution of a gradient window g [COUT][RIN x CINW] onto the window one site wider on every side, times the
// act' already in sD (in place): sD[ci][s] *= sum_{co, tap} w[co][tap][ci] g[co][s - tap].  Same blocking as conv_act.
template <int COUT, int MOUT, int COUTW, int OUTP, int RIN, int CINW, int GSTR>
__device__ __forceinline__ void convT_mul(const Dual* __restrict__ g, const double* __restrict__ wb, Dual* __restrict__ sD, int half,
                                          int lane128) {
    constexpr int NS = (MOUT + 127) / 128;
    Dual acc[NS][4];
    int rq[NS], cq[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) {
        const int s = min(lane128 + 128 * q, MOUT - 1);
        rq[q] = s / COUTW; cq[q] = s - rq[q] * COUTW;
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[q][k] = Dual(0.0);
    }
#pragma unroll 1
    for (int co = 0; co < COUT; ++co)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const double* wp = wb + ((co * 9 + ky * 3 + kx) * 8 + half * 4);
#pragma unroll
                for (int q = 0; q < NS; ++q) {
                    const int rr = rq[q] - ky, cc = cq[q] - kx;
                    const bool ok = (rr >= 0) && (rr < RIN) && (cc >= 0) && (cc < CINW);
                    const Dual v = g[co * GSTR + (ok ? rr * CINW + cc : 0)];
                    const Dual gv = ok ? v : Dual(0.0);
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[q][k] = fma(wp[k], gv, acc[q][k]);
                }
            }
#pragma unroll
    for (int q = 0; q < NS; ++q) {
        const int s = lane128 + 128 * q;
        if (s < MOUT) {
#pragma unroll
            for (int k = 0; k < 4; ++k) sD[(half * 4 + k) * OUTP + s] *= acc[q][k];
        }
    }
}

template <int TR, int TC, bool BWD>
__global__ __launch_bounds__(256) void k_flow_dual(FlowDualArgs A) {
    using G = DG<TR, TC>;
    using S = DSmem<TR, TC, BWD>;
    constexpr int C0 = G::C0, C1 = G::C1, C2 = G::C2, M0 = G::M0, M1 = G::M1, M2 = G::M2, M3 = G::M3, NA = G::NA, S1 = G::S1, S2 = G::S2;
    __shared__ __attribute__((aligned(16))) Dual sm[S::SIZE];
    Dual* sP = sm + S::P;   Dual* sIn = sm + S::IN;
    Dual* sH1 = sm + S::H1; Dual* sH2 = sm + S::H2;
    Dual* sST = sm + S::ST; Dual* sDL = sm + S::DL;
    Dual* sD1 = sm + S::D1; Dual* sD2 = sm + S::D2;
    Dual* sGO = sm + S::GO; Dual* sGP = sm + S::GP;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = wave & 1;                       // which 4 output channels this wave owns
    const int lane128 = lane | ((wave >> 1) << 6);   // site slot among the 2 waves of a half
    const int L = A.L, mu = A.mu, off = A.off, act = A.act;
    const int n = L * L;
    const double* __restrict__ w = A.wint;
    // Tangent parts of the weight gradients, kept in registers while the workgroup walks its items.  conv3: one weight per thread
    // (216 + 3).  conv2 and conv1 are register-tiled, a thread summing over every NCH-th site of the window:
    //   conv2: task (ci, ky) x 8 output channels x 3 taps kx = 24 sums (the 25th task is the bias: h = 1), 10 site chunks;
    //   conv1: task (ci, tap) x 8 output channels = 8 sums (the 19th task is the bias), 13 site chunks;
    // a site then costs 11 (9) LDS reads for 48 (16) FMAs instead of two reads per pair.  The chunks are added up once, behind the walk.
    constexpr int NT2 = 25, NCH2 = 10, NT1 = 19, NCH1 = 13;
    static_assert(NT2 * NCH2 <= 256 && NT1 * NCH1 <= 256, "one thread per (task, chunk)");
    double a3 = 0.0, a2[24], a1[8];
#pragma unroll
    for (int k = 0; k < 24; ++k) a2[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) a1[k] = 0.0;

    for (int item = blockIdx.x; item < A.items; item += gridDim.x) {
        const int b = item / A.ntiles, tile = item - b * A.ntiles;
        const int ti = tile / A.ntj, tj = tile - ti * A.ntj;
        const int i0 = ti * TR, j0 = tj * TC;
        const Dual* __restrict__ x0 = A.x + (size_t)b * 2 * n;
        const Dual* __restrict__ x1 = x0 + n;

        // ---- plaquette window + net input ------------------------------------
        for (int t = tid; t < M0; t += 256) {
            const int r = t / C0, c = t - r * C0;
            const int i = ft_modL(i0 - 3 + r, L), j = ft_modL(j0 - 3 + c, L);
            const int ip = i + 1 == L ? 0 : i + 1, jp = j + 1 == L ? 0 : j + 1;
            const Dual p = x0[i * L + j] - x1[i * L + j] - x0[i * L + jp] + x1[ip * L + j];
            const int sel = ft_stripe(i, j, mu, off);
            Dual sn = 0.0, cs = 1.0;
            if (sel == 1 || sel == 2) ft_sincos(p, &sn, &cs);
            sP[t] = p;
            sIn[t] = cs;
            sIn[M0 + t] = sn;
            if (BWD) sGP[t] = Dual(0.0);
        }
        if (BWD) { for (int t = tid; t < 3 * M3; t += 256) sGO[t] = Dual(0.0); }
        __syncthreads();

        // ---- conv1 (2 -> 8) + act on the tile+2 window, conv2 (8 -> 8) + act on the tile+1 window
        conv_act<2, M1, C1, S1, M0, C0, BWD>(sIn, w + W1F, w + B1, sH1, sD1, half, lane128, act);
        __syncthreads();
        conv_act<8, M2, C2, S2, S1, C1, BWD>(sH1, w + W2F, w + B2, sH2, sD2, half, lane128, act);
        __syncthreads();

        // ---- conv3 (8 -> 3) at the active sites: wave co computes output channel co ---
        static_assert(NA <= 64, "one lane per active site");
        if (wave < 3 && lane < NA) {
            int ar, ac; G::active(lane, mu, off, ar, ac);
            Dual acc = Dual(w[B3 + wave]);
#pragma unroll 1
            for (int ci = 0; ci < 8; ++ci)
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx)
                        acc = fma(w[W3F + (ci * 9 + ky * 3 + kx) * 4 + wave], sH2[ci * S2 + (ar + ky) * C2 + ac + kx], acc);
            sST[wave * NA + lane] = acc;
        }
        __syncthreads();

        if (!BWD) {
            // ---- tan-mixture transform and the link update x' = wrap(x +- delta) on the active stripe
            for (int a = tid; a < NA; a += 256) {
                int ar, ac; G::active(a, mu, off, ar, ac);
                const Dual Pa = sP[(ar + 3) * C0 + ac + 3];
                Dual sn, cs;
                ft_sincos(0.5 * Pa, &sn, &cs);
                Dual ysum = 0.0;
#pragma unroll
                for (int k = 0; k < NMIX; ++k) { const MixComp<Dual> m(sST[k * NA + a], cs, sn); ysum += m.y(); }
                sDL[a] = mix_new_plaq(ysum, NMIX, sST[NMIX * NA + a]) - Pa;
            }
            __syncthreads();
            for (int t = tid; t < M3; t += 256) {
                const int r = t / TC, c = t - r * TC;
                const int i = i0 + r, j = j0 + c;
                Dual v0 = x0[i * L + j], v1 = x1[i * L + j];
                if (ft_stripe(i, j, mu, off) == 0) {
                    const Dual d = sDL[G::active_index(r, c, mu, off)];
                    if (mu == 0) v0 = ft_wrap(d + v0); else v1 = ft_wrap(-d + v1);
                }
                Dual* y0 = A.y + (size_t)b * 2 * n;
                y0[i * L + j] = v0; y0[n + i * L + j] = v1;
            }
        } else {
            // ---- adjoint of the transform at the tile's own active sites (k_gen_transform_bwd's statement) -------
            for (int a = tid; a < NA; a += 256) {
                int ar, ac; G::active(a, mu, off, ar, ac);
                const int ai = i0 + ar, aj = j0 + ac;
                const Dual* __restrict__ gp = A.up_gp + (size_t)b * n;
                const int sp = mu == 0 ? ai * L + (aj == 0 ? L - 1 : aj - 1) : (ai == 0 ? L - 1 : ai - 1) * L + aj;   // the passive neighbour
                const Dual gdelta = gp[ai * L + aj] - gp[sp];
                const Dual Pa = sP[(ar + 3) * C0 + ac + 3];
                Dual sn, cs;
                ft_sincos(0.5 * Pa, &sn, &cs);
                const Dual sinP = 2.0 * sn * cs;
                Dual csum = 0.0, esum = 0.0;
#pragma unroll
                for (int k = 0; k < NMIX; ++k) {
                    const MixComp<Dual> m(sST[k * NA + a], cs, sn);
                    csum += m.C(NMIX);
                    esum += m.En(sinP) * m.invD * m.invD;
                }
                const MixAdjoint<Dual> adj(gdelta, A.glogj_const / (NMIX * csum), csum, esum);
#pragma unroll
                for (int k = 0; k < NMIX; ++k) {
                    const MixComp<Dual> m(sST[k * NA + a], cs, sn);
                    sGO[k * M3 + ar * TC + ac] = adj.gs(m.A(sinP, NMIX), m.Bn() * m.invD * m.invD);     // dL/ds_k
                }
                sGO[NMIX * M3 + ar * TC + ac] = gdelta;                                                  // dL/dt
                sGP[(ar + 3) * C0 + ac + 3] = adj.dir();
            }
            __syncthreads();

            // ---- weight gradient of conv3 (g_out and h2), tangent part ------------
            if (tid < 216 + 3) {
                double acc = 0.0;
                if (tid < 216) {
                    const int co = tid / 72, ci = (tid / 9) % 8, tap = tid % 9, ky = tap / 3, kx = tap % 3;
                    for (int a = 0; a < NA; ++a) {
                        int r, c; G::active(a, mu, off, r, c);
                        const Dual g = sGO[co * M3 + r * TC + c], h = sH2[ci * S2 + (r + ky) * C2 + c + kx];
                        acc = ::fma(g.t, h.v, ::fma(g.v, h.t, acc));
                    }
                } else {
                    const int co = tid - 216;
                    for (int a = 0; a < NA; ++a) { int r, c; G::active(a, mu, off, r, c); acc += sGO[co * M3 + r * TC + c].t; }
                }
                a3 += acc;
            }

            // ---- conv3^T, times act'(z2)  -> gz2 (in place over D2) -------------
            convT_mul<3, M2, C2, S2, TR, TC, M3>(sGO, w + W3B, sD2, half, lane128);
            __syncthreads();

            // ---- weight gradient of conv2 (gz2 and h1) -----------------------------
            if (tid < NT2 * NCH2) {
                const int task = tid % NT2, chunk = tid / NT2;
                const bool bias = task == NT2 - 1;
                const int ci = bias ? 0 : task / 3, ky = bias ? 0 : task - 3 * (task / 3);
                for (int s = chunk; s < M2; s += NCH2) {
                    const int r = s / C2, c = s - r * C2;
                    const Dual* hp = sH1 + ci * S1 + (r + ky) * C1 + c;
                    const Dual h0 = bias ? Dual(1.0) : hp[0], h1 = bias ? Dual(0.0) : hp[1], h2 = bias ? Dual(0.0) : hp[2];
#pragma unroll
                    for (int co = 0; co < 8; ++co) {
                        const Dual g = sD2[co * S2 + s];
                        a2[co * 3 + 0] = ::fma(g.t, h0.v, ::fma(g.v, h0.t, a2[co * 3 + 0]));
                        a2[co * 3 + 1] = ::fma(g.t, h1.v, ::fma(g.v, h1.t, a2[co * 3 + 1]));
                        a2[co * 3 + 2] = ::fma(g.t, h2.v, ::fma(g.v, h2.t, a2[co * 3 + 2]));
                    }
                }
            }

            // ---- conv2^T, times act'(z1) -> gz1 (in place over D1) --------------
            convT_mul<8, M1, C1, S1, TR + 2, C2, S2>(sD2, w + W2B, sD1, half, lane128);
            __syncthreads();

            // ---- weight gradient of conv1 (gz1 and the net input) -------------------
            if (tid < NT1 * NCH1) {
                const int task = tid % NT1, chunk = tid / NT1;
                const bool bias = task == NT1 - 1;
                const int ci = bias ? 0 : task / 9, tap = bias ? 0 : task - 9 * (task / 9), ky = tap / 3, kx = tap - 3 * ky;
                for (int s = chunk; s < M1; s += NCH1) {
                    const int r = s / C1, c = s - r * C1;
                    const Dual h = bias ? Dual(1.0) : sIn[ci * M0 + (r + ky) * C0 + c + kx];
#pragma unroll
                    for (int co = 0; co < 8; ++co) {
                        const Dual g = sD1[co * S1 + s];
                        a1[co] = ::fma(g.t, h.v, ::fma(g.v, h.t, a1[co]));
                    }
                }
            }

            // ---- conv1^T and the (cos, sin) adjoint at frozen plaquettes --------
            {
                constexpr int NS0 = (M0 + 255) / 256;
                Dual gc[NS0], gs[NS0];
                int rq[NS0], cq[NS0];
#pragma unroll
                for (int q = 0; q < NS0; ++q) {
                    const int t = min(tid + 256 * q, M0 - 1);
                    rq[q] = t / C0; cq[q] = t - rq[q] * C0;
                    gc[q] = Dual(0.0); gs[q] = Dual(0.0);
                }
#pragma unroll 1
                for (int co = 0; co < 8; ++co)
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                        for (int kx = 0; kx < 3; ++kx) {
                            const double* wp = w + W1B + (co * 9 + ky * 3 + kx) * 2;
#pragma unroll
                            for (int q = 0; q < NS0; ++q) {
                                const int rr = rq[q] - ky, cc = cq[q] - kx;
                                const bool ok = (rr >= 0) && (rr < TR + 4) && (cc >= 0) && (cc < C1);
                                const Dual v = sD1[co * S1 + (ok ? rr * C1 + cc : 0)];
                                const Dual g = ok ? v : Dual(0.0);
                                gc[q] = fma(wp[0], g, gc[q]); gs[q] = fma(wp[1], g, gs[q]);
                            }
                        }
#pragma unroll
                for (int q = 0; q < NS0; ++q) {
                    const int t = tid + 256 * q;
                    if (t < M0) {
                        const int i = ft_modL(i0 - 3 + rq[q], L), j = ft_modL(j0 - 3 + cq[q], L);
                        const int sel = ft_stripe(i, j, mu, off);
                        if (sel == 1 || sel == 2) sGP[t] = -sIn[M0 + t] * gc[q] + sIn[t] * gs[q];
                    }
                }
            }
            __syncthreads();
            Dual* out = A.gp_part + (size_t)item * M0;
            for (int t = tid; t < M0; t += 256) out[t] = sGP[t];
        }
        __syncthreads();                                   // the next item rewrites the planes
    }

    if constexpr (BWD) {
        // one partial row per workgroup: the chunks' sums of conv2 and conv1 added in chunk order through LDS (the planes are done)
        double* gwp = A.gw_part + (size_t)blockIdx.x * FLOW_GW_STRIDE;
        double* red = reinterpret_cast<double*>(sm);
        static_assert(NT2 * NCH2 * 24 * sizeof(double) <= (size_t)S::SIZE * sizeof(Dual), "the reduction fits the planes");
        if (tid < 216) gwp[CW2 + tid] = a3; else if (tid < 219) gwp[CB2 + tid - 216] = a3;
        if (tid < NT2 * NCH2) {
#pragma unroll
            for (int k = 0; k < 24; ++k) red[tid * 24 + k] = a2[k];
        }
        __syncthreads();
        for (int t = tid; t < 576 + 8; t += 256) {
            int task, k, o;
            if (t < 576) { const int co = t / 72, ci = (t / 9) % 8, tap = t % 9; task = ci * 3 + tap / 3; k = co * 3 + tap % 3; o = CW1 + t; }
            else { task = NT2 - 1; k = (t - 576) * 3; o = CB1 + t - 576; }
            double acc = 0.0;
            for (int ch = 0; ch < NCH2; ++ch) acc += red[(ch * NT2 + task) * 24 + k];
            gwp[o] = acc;
        }
        __syncthreads();
        if (tid < NT1 * NCH1) {
#pragma unroll
            for (int k = 0; k < 8; ++k) red[tid * 8 + k] = a1[k];
        }
        __syncthreads();
        if (tid < 144 + 8) {
            int task, k, o;
            if (tid < 144) { k = tid / 18; task = tid - 18 * k; o = CW0 + tid; }       // [co][ci][tap]: task = ci * 9 + tap
            else { task = NT1 - 1; k = tid - 144; o = CB0 + k; }
            double acc = 0.0;
            for (int ch = 0; ch < NCH1; ++ch) acc += red[(ch * NT1 + task) * 8 + k];
            gwp[o] = acc;
        }
    }
}

// gp[b][i][j] += sum over tiles and over every window position that wraps onto (i, j): k_gather_gp's general path (flow.hip) on
// dual numbers, fixed summation order
__global__ void k_gather_gp_dual(const Dual* __restrict__ part, int L, int tr, int tc, int nti, int ntj, Dual* __restrict__ gp) {
    const int b = blockIdx.y;
    const int n = L * L;
    const int ntiles = nti * ntj;
    const int wr = tr + 6, wc = tc + 6, n0 = wr * wc;
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
        const int i = s / L, j = s - i * L;
        Dual acc = 0.0;
        // candidate tiles per dimension: all of them when there are <= 3, else own and both neighbours
        const int ni = nti <= 3 ? nti : 3, bi = nti <= 3 ? 0 : i / tr - 1;
        const int nj = ntj <= 3 ? ntj : 3, bj = ntj <= 3 ? 0 : j / tc - 1;
        for (int di = 0; di < ni; ++di) {
            const int ti = (bi + di + nti) % nti;
            const int r0 = ft_modL(i - ti * tr + 3, L);
            for (int r = r0; r < wr; r += L)
                for (int dj = 0; dj < nj; ++dj) {
                    const int tj = (bj + dj + ntj) % ntj;
                    const int c0 = ft_modL(j - tj * tc + 3, L);
                    const Dual* p = part + ((size_t)b * ntiles + ti * ntj + tj) * n0 + r * wc;
                    for (int c = c0; c < wc; c += L) acc += p[c];
                }
        }
        const size_t o = (size_t)b * n + s;
        gp[o] = gp[o] + acc;
    }
}

template <bool BWD>
int launch_dual(FlowDualArgs a, int tile, hipStream_t s) {
    if (!flow_dual_shape(a.B, a.L, tile)) return FTHMC_ERR_UNSUPPORTED;
    const FlowGeom g = flow_dual_geom(tile);
    a.ntj = g.ntj(a.L); a.ntiles = g.ntiles(a.L); a.items = a.B * a.ntiles;
    // forward: one workgroup per item up to eight rounds of the chip; backward: flow_dual_nparts workgroups, one partial row each
    const int grid = BWD ? flow_dual_nparts(a.B, a.L, tile) : (a.items < 4096 ? a.items : 4096);
    if (tile == 0) hipLaunchKernelGGL((k_flow_dual<8, 8, BWD>), dim3(grid), dim3(256), 0, s, a);
    else           hipLaunchKernelGGL((k_flow_dual<8, 16, BWD>), dim3(grid), dim3(256), 0, s, a);
    FT_LAUNCH_CHECK(); return FTHMC_OK;
}

}  // namespace

namespace fthmc {

int launch_flow_dual_fwd(const FlowDualArgs& a, int tile, hipStream_t s) { return launch_dual<false>(a, tile, s); }
int launch_flow_dual_bwd(const FlowDualArgs& a, int tile, hipStream_t s) { return launch_dual<true>(a, tile, s); }
int launch_gather_gp_dual(const Dual* gp_part, int B, int L, int tile, Dual* gp, hipStream_t s) {
    const FlowGeom g = flow_dual_geom(tile);
    int gx = (L * L + 255) / 256; if (gx > 64) gx = 64;
    hipLaunchKernelGGL(k_gather_gp_dual, dim3(gx, B), dim3(256), 0, s, gp_part, L, g.tr, g.tc, g.nti(L), g.ntj(L), gp);
    FT_LAUNCH_CHECK(); return FTHMC_OK;
}

}  // namespace fthmc
