// What the kernels that walk a coupling layer BACKWARDS state once: k_flow_bwd_gather (flow_bwd_gather.hip), k_flow_bwd_train
// (flow_bwd_train.hip), k_flow_wgrad (flow_wgrad.hip) and the backward half of k_ft_small (flow_small.hip).
//   * every kernel of the adjoint walk: the conv2^T dispatch over the dead window line, conv1^T's wave-uniform weights, frozen_site;
//   * the two 16 x 16-tile adjoint walks (gather, train): window geometry, the transform-task map and its coefficient loads, the
//     conv2^T tile map with the act'(z1) loads of its epilogue lanes;
//   * the two kernels that WALK (chain, tile) items and sum weight gradients (wgrad, train): the walk itself, the h-window and
//     net-input window maps, the B-operand lane map, conv3's weight-gradient task, the group's partial.
// A function here is the text its callers used to carry, moved: `mu` and `off` are plain arguments that fold where the caller's
// are compile-time constants.  DESIGN.md 4.4 says which kernel takes which piece, what stayed written out twice and what was measured.
#pragma once
#include "flow_mfma_common.h"

namespace fthmc_flow {

// ---- every kernel of the adjoint walk ---------------------------------------------------------------------------------------

// conv2^T of one MFMA tile whose dead window line is kd (wave-uniform): pairs = columns for mu = 0 (3 x 4 window), rows for
// mu = 1 (4 x 3); straight-line code per (K order, kd) (flow_mfma_common.h conv2t_tile)
template <int RSA, int PSA>
__device__ __forceinline__ double4_t conv2t_dead_line(int mu, int kd, const double* wp, const double* a0) {
    double4_t acc;
    if (mu == 0) {
        switch (kd) {
            case 0: acc = conv2t_tile<KConv2Col, 4, 0, RSA, PSA>(wp, a0); break;
            case 1: acc = conv2t_tile<KConv2Col, 4, 1, RSA, PSA>(wp, a0); break;
            case 2: acc = conv2t_tile<KConv2Col, 4, 2, RSA, PSA>(wp, a0); break;
            default: acc = conv2t_tile<KConv2Col, 4, 3, RSA, PSA>(wp, a0); break;
        }
    } else {
        switch (kd) {
            case 0: acc = conv2t_tile<KConv2Row, 3, 0, RSA, PSA>(wp, a0); break;
            case 1: acc = conv2t_tile<KConv2Row, 3, 1, RSA, PSA>(wp, a0); break;
            case 2: acc = conv2t_tile<KConv2Row, 3, 2, RSA, PSA>(wp, a0); break;
            default: acc = conv2t_tile<KConv2Row, 3, 3, RSA, PSA>(wp, a0); break;
        }
    }
    return acc;
}

// conv1^T's 18 weights of one hidden channel (wq: the channel's line of the backward weight block, LB_W0 + 18 co; wave-uniform):
// scalar loads from the constant address space, written out wide (8 + 8 + 2 doubles): the merging pass is off for these
// kernels (FT_LDS_B64)
__device__ __forceinline__ void conv1t_weights(const double* wq_, double (&w0s)[18]) {
    typedef const double __attribute__((address_space(4))) * cdptr;
    cdptr wq = (cdptr)(size_t)wq_;
    typedef double double8c_t __attribute__((ext_vector_type(8)));
    typedef const double8c_t __attribute__((address_space(4))) * cd8ptr;
    const double8c_t va = *(cd8ptr)(wq), vb = *(cd8ptr)(wq + 8);
#pragma unroll
    for (int k = 0; k < 8; ++k) { w0s[k] = va[k]; w0s[8 + k] = vb[k]; }
    w0s[16] = wq[16]; w0s[17] = wq[17];
}

// frozen site f of a region with NL positions along the stripe lines: line position q = f % NL along the stripes, h-th frozen
// line across them (stripe classes 1, 2 of every four lines) -> (r, c).  NL = 16: f = position + 16 h -- a 32-lane group then
// holds an odd and an even line of 16 positions: 32 different banks at row stride 18
template <int NL> __device__ __forceinline__ void frozen_site(int f, int mu, int off, int& r, int& c) {
    const int h = fdiv<NL>(f), q = f - h * NL, x = 4 * (h >> 1) + ((off + 1 + (h & 1)) & 3);
    if (mu == 0) { r = q; c = x; } else { c = q; r = x; }
}

// ---- the 16 x 16-tile adjoint walks (SmemG, SmemT) ----------------------------------------------------------------------------

template <int TR, int TC> struct BwdWindows {
    static constexpr int W3R = TR + 6, W3C = TC + 6, N3W = W3R * W3C;   // g_out window (active sites only)
    static constexpr int W2R = TR + 4, W2C = TC + 4, N2W = W2R * W2C;   // act'(z2) -> gz2
    static constexpr int W1R = TR + 2, W1C = TC + 2, N1W = W1R * W1C;   // act'(z1) -> gz1; cos/sin; h1, h2
    static constexpr int N3 = TR * TC;
    // gz2 rows are RS2 apart in LDS: odd, so that the 16 lanes of a conv2^T operand read (one per window row) fall into 16
    // different banks
    static constexpr int RS2 = W2C + 1;
    static constexpr int PS2 = ps_round16(W2R * RS2), PS1 = ps_round(N1W);   // gz2: MFMA operand; gz1: read by four channel lanes per site
    // active lines of the g_out window: every 4th column (mu = 0) or row (mu = 1)
    static constexpr int NLC = (W3C + 3) / 4, NLR = (W3R + 3) / 4;
    static constexpr int NSLOT = cmax_(W3R * NLC, NLR * W3C);           // transform tasks
    static constexpr int NTT = (NSLOT + 63) / 64 * 64;                  // threads that run them (last waves)
};

// transform task `ta` (ta < 0: none) -> active site (tr3, tc3) of the tile+3 window whose first active column / row is c0 / r0;
// threads without a task get a valid site to load from
template <class S> __device__ __forceinline__ bool transform_task(int ta, int mu, int c0, int r0, int& tr3, int& tc3) {
    bool ttask = false;
    tr3 = 0; tc3 = 0;
    if (ta >= 0) {
        if (mu == 0) { tr3 = fdiv<S::NLC>(ta); tc3 = c0 + 4 * (ta - tr3 * S::NLC); ttask = tr3 < S::W3R && tc3 < S::W3C; }
        else { const int m = fdiv<S::W3C>(ta); tc3 = ta - m * S::W3C; tr3 = r0 + 4 * m; ttask = tr3 < S::W3R; }
        if (!ttask) { tr3 = 3; tc3 = 3; }                                // any valid site
    } else { tr3 = 3; tc3 = 3; }
    return ttask;
}
// the task's mixture coefficients, [k][n/4][A B C E] (struct Stash) at compact active index ia: 16 bytes per load
__device__ __forceinline__ void transform_coeffs(const double* stc, int n, unsigned ia, double (&tcv)[4 * NMIX]) {
#pragma unroll
    for (int q = 0; q < 4 * NMIX; q += 2) {
        const double2_t t2 = ldu2(stc + (size_t)(q >> 2) * n, ia * 4u + (q & 3));
        tcv[q] = t2.x; tcv[q + 1] = t2.y;
    }
}

// conv2^T pairs its output sites ACROSS the stripe lines -- columns (c, c + 1) of one row for mu = 0, rows (r, r + 1)
// of one column for mu = 1 -- so the pair's input window is four consecutive lines of gz2, exactly one of which is
// dead (conv3^T wrote zeros there): its six K steps are skipped, 18 of 24 remain.  Which of the four it is depends on
// the parity of the pair's position u across the lines only, so an MFMA tile holds pairs of ONE parity:
//     tiles 0 .. NU-1:  u = tile, positions v = 0 .. 15 along the lines        (NU = 9 pairs across, NV = 18 along)
//     tiles NU, NU+1:   the remaining v = 16, 17 of the even / of the odd u
// The epilogue's lane (g = lane >> 4, i = lane & 15) of tile T = wave + 8 it owns pair i of the tile, channels
// 2 g and 2 g + 1, both sites of the pair.
template <int W1C> struct Conv2TMap {
    static constexpr int NU = W1C / 2, NTILE1 = NU + 2, NIT1 = (NTILE1 + NW - 1) / NW;
    static_assert(W1C == 18 && NIT1 == 2, "conv2^T tile map: 16 positions along the lines + 2, two rounds of tiles");
    // pair position (across, along) of round `it`; rows / columns of site 0: mu = 0: (pv, 2 pu), mu = 1: (2 pu, pv) in tile+1 coordinates
    static __device__ __forceinline__ void pair(int wave, int lane, int it, int& pu, int& pv, bool& pok) {
        const int T = wave + NW * it, i = lane & 15;
        if (T < NU) { pu = T; pv = i; pok = true; }
        else { pu = 2 * (i >> 1) + (T - NU); pv = 16 + (i & 1); pok = T < NTILE1 && pu < NU; if (!pok) { pu = 0; pv = 0; } }
    }
    // dead window line of tile T, kd0 = that of the even pairs (odd: + 2); wave-uniform
    static __device__ __forceinline__ int dead_line(int kd0, int T) { return (kd0 + 2 * (T < NU ? T & 1 : T - NU)) & 3; }
};
// act'(z1) of the epilogue lane's two sites (records ga, gb of the stashed plane), channels 2 g, 2 g + 1: one 16-byte load per site
__device__ __forceinline__ void conv2t_d1_load(const double* st1, int ga, int gb, int lane, double (&d1v)[4]) {
    const unsigned og = 2u * (unsigned)(lane >> 4);
    const double2_t va = ldu2(st1, (unsigned)ga * 8u + og), vb = ldu2(st1, (unsigned)gb * 8u + og);
    d1v[0] = va.x; d1v[1] = va.y; d1v[2] = vb.x; d1v[3] = vb.y;
}

// ---- the kernels that WALK (chain, tile) items and sum weight gradients (k_flow_wgrad, k_flow_bwd_train) ------------------------

// The walk is STRIDED: the ns workgroups that are resident together on an XCD (slot s of a round) stand on ns consecutive
// items at every step and move on by ns items -- at L = 256 four whole tile rows of a chain per step, so that the halo lines a
// tile shares with its neighbours are fetched once into the XCD's L2 (walking CONSECUTIVE tiles, every halo came from HBM
// again: 781 MB per launch at the config-5 shard against 573 MB for one tile per workgroup).
// grid: x = 8 XCDs (blockIdx.x % 8) x rounds x ns; round kr = xcd * R + r covers items [kr * tpw * ns, (kr + 1) * tpw * ns)
struct Walk { int first, grp, nwalk, ns; };              // items first, first + ns, ... (nwalk of them); row grp of the partials
__device__ __forceinline__ bool walk_of_block(const fthmc::FlowLayerArgs& A, int ntiles, Walk& w) {
    const int items = A.B * ntiles, tpw = A.tpw, ns = A.wg_ns;
    const int KR = (items + tpw * ns - 1) / (tpw * ns), R = (KR + 7) >> 3;
    const int idx = (int)blockIdx.x >> 3, r_ = idx / ns, s_ = idx - r_ * ns, kr = ((int)blockIdx.x & 7) * R + r_;
    const int first = kr * tpw * ns + s_;
    if (r_ >= R || first >= items) return false;
    const int grp = kr * ns + s_;                                         // valid groups are a prefix of this numbering
    const int nwalk = min(tpw, (items - first + ns - 1) / ns);
    w.first = first; w.grp = grp; w.nwalk = nwalk; w.ns = ns;
    return true;
}
// item -> (chain, tile row, tile column); uniform: scalar divisions, once per item
__device__ __forceinline__ void item_coords(int item, int ntiles, int ntj_, int& b, int& ti, int& tj) {
    b = item / ntiles;
    const int t = item - b * ntiles;
    ti = t / ntj_; tj = t - ti * ntj_;
}

// h1 / h2 / net-input planes on tile+1 (+ one row of slack).  Plane stride = 12 (mod 32): the B operand reads of every N tile
// (lanes = (ci, kx + g, kyb): 18 ci + 4 kyb + kx + g with the stride 18 of ps_round put ci = 2 on the banks of ci = 0, kyb = 1)
// and the fill's writes (channel quads 4 planes apart) are both free of bank conflicts
constexpr int psh_round(int nh, int w1c) { return ((nh + w1c - 12 + 31) / 32) * 32 + 12; }
// after the walk, over the planes: the waves' accumulators [8][4 tiles][4][64], bias lane sums [8][2][8], conv3 sums [432]
struct WalkRed { static constexpr int RED = 0, RBS = RED + 8 * 4 * 4 * 64, RC3 = RBS + 8 * 2 * 8, RSIZE = RC3 + 432; };

// tile+1 window of h1 / h2: tasks (window site, channel quad) in NRH rounds of the workgroup; hls: LDS slot or -1
template <int W1C, int NH, int PSH> struct HWindow {
    static constexpr int NIT = 2 * NH, NRH = (NIT + NT - 1) / NT;
    int hwr[NRH], hwc[NRH], hwq[NRH], hls[NRH];
    __device__ __forceinline__ explicit HWindow(int t0) {
#pragma unroll
        for (int k = 0; k < NRH; ++k) {
            const int t = min(t0 + k * NT, NIT - 1), ws = t >> 1;
            hwq[k] = t & 1; hwr[k] = fdiv<W1C>(ws); hwc[k] = ws - hwr[k] * W1C;
            hls[k] = t0 + k * NT < NIT ? (4 * hwq[k]) * PSH + hwr[k] * W1C + hwc[k] : -1;
        }
    }
};
// an h record's channel quad (two 16-byte loads) into its four LDS planes
template <int PSH> __device__ __forceinline__ void h_quad_store(double* p, const double2_t (&hv)[2]) {
    p[0] = hv[0].x; p[PSH] = hv[0].y; p[2 * PSH] = hv[1].x; p[3 * PSH] = hv[1].y;
}
// net input on the tile+1 window, thread = window site (fwr, fwc): frozen = stripe classes 1, 2 (tile origins are multiples of 4)
template <int W1C, int NH> __device__ __forceinline__ void netin_task(int t0, int mu, int off, int& fwr, int& fwc, bool& ftask, bool& ffrozen) {
    fwr = fdiv<W1C>(min(t0, NH - 1)); fwc = min(t0, NH - 1) - fwr * W1C;
    const int fl = ((mu == 0 ? fwc : fwr) - 1 - off) & 3;
    ftask = t0 < NH; ffrozen = ftask && (fl == 1 || fl == 2);
}

// weight-gradient GEMM, B operand of lane group g: column ncol = (ci, kx, kyb) of an N tile with ncols live columns, ky = 2 kyb + dy
template <int W1C, int PSH> __device__ __forceinline__ int wgrad_bcol(int ncol, int ncols, int g) {
    const int nc = ncol < ncols ? ncol : 0, ci = nc / 6, kx = (nc % 6) >> 1, kyb = nc & 1;
    return ci * PSH + 2 * kyb * W1C + kx + g;
}

// conv3 (8 -> 3, active sites only) weight gradient: thread = (output (co, ci, tap), half of the active sites); the 32 sites of
// the half at compile-time offsets from the thread's base (the stripe offset `off` and the half are folded into `ph`).  Two
// loop forms side by side: the plain one (k_flow_wgrad) ...
template <int MU, int TC, int W1C>
__device__ __forceinline__ void conv3_acc(const double* __restrict__ pg, const double* __restrict__ ph, double (&acc)[4]) {
#pragma unroll
    for (int a = 0; a < 32; a += 2) {
        const double2_t g2 = *reinterpret_cast<const double2_t*>(pg + a);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int aa = a + e;
            const int o = MU == 0 ? (aa / (TC / 4)) * W1C + 4 * (aa % (TC / 4)) : 4 * (aa / TC) * W1C + aa % TC;
            acc[aa & 3] = fma(e ? g2.y : g2.x, ph[o], acc[aa & 3]);
        }
    }
}
// ... and in batches of eight sites (k_flow_bwd_train): the eight h2 reads and the four 16-byte g_out reads of a batch are issued
// together, then its eight FMAs (left to itself the scheduler of the mu = 0 instance put a full LDS wait behind every single read:
// 2.2 k cycles for this loop against 1.0 k in the mu = 1 instance with the same instructions)
template <int MU, int TC, int W1C>
__device__ __forceinline__ void conv3_acc_batched(const double* __restrict__ pg, const double* __restrict__ ph, double (&acc)[4]) {
#pragma unroll
    for (int a0 = 0; a0 < 32; a0 += 8) {
        double2_t g2[4];
        double hv[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) g2[e] = *reinterpret_cast<const double2_t*>(pg + a0 + 2 * e);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int aa = a0 + e;
            hv[e] = ph[MU == 0 ? (aa / (TC / 4)) * W1C + 4 * (aa % (TC / 4)) : 4 * (aa / TC) * W1C + aa % TC];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e & 3] = fma((e & 1) ? g2[e >> 1].y : g2[e >> 1].x, hv[e], acc[e & 3]);
        __builtin_amdgcn_sched_barrier(0);
    }
}
// one item's conv3 task: gw2[co][ci][tap] += sum over the own active sites of g_out[co] h2[ci][site + tap] on threads 0 .. 431
// (sGO: [3][NA] g_out at the own active sites, task order; sH2: the h2 window, [8][PSH]); b3: the eighth wave sums the three
// g_out planes
template <int TC, int W1C, int PSH, int NA, bool BATCHED>
__device__ __forceinline__ void conv3_wgrad_task(const double* __restrict__ sGO, const double* __restrict__ sH2, int tid, int lane,
                                                 int mu, int off, double (&acc3)[3]) {
    if (tid < 432) {
        const int hf = tid >= 216 ? 1 : 0, t = tid - 216 * hf;
        const int co = fdiv<9>(fdiv<8>(t)), ci = fdiv<9>(t) & 7, tap = t - fdiv<9>(t) * 9, ky = fdiv<3>(tap), kx = tap - 3 * ky;
        const double* pg = sGO + co * NA + hf * (NA / 2);
        const double* ph = sH2 + ci * PSH + ky * W1C + kx;           // h2 at own (r, c) + (ky - 1, kx - 1): window index (r + ky) W1C + c + kx
        double c3[4] = {0.0, 0.0, 0.0, 0.0};
        const double* ph0 = ph + hf * (NA / 2 / (TC / 4)) * W1C + off, * ph1 = ph + (off + 4 * hf * (NA / 2 / TC)) * W1C;
        if (BATCHED) { if (mu == 0) conv3_acc_batched<0, TC, W1C>(pg, ph0, c3); else conv3_acc_batched<1, TC, W1C>(pg, ph1, c3); }
        else         { if (mu == 0) conv3_acc<0, TC, W1C>(pg, ph0, c3);         else conv3_acc<1, TC, W1C>(pg, ph1, c3); }
        acc3[0] += (c3[0] + c3[1]) + (c3[2] + c3[3]);
    } else if (tid >= 448) {
#pragma unroll
        for (int k = 0; k < 3; ++k) acc3[k] += sGO[k * NA + lane];
    }
}

// The group's partial: the waves' K slices (acc: four N tiles, 0..2 conv2, 3 conv1; bsum: bias lane sums b2, b1; acc3: conv3)
// summed through LDS (S::RED, RBS, RC3 over the planes) in a fixed order and scattered into canonical order at gw0.  TR2: conv2
// was accumulated transposed (k_flow_bwd_train, mu = 1: columns (ci, ky, kxb), kx = 2 kxb + d).  Starts with a barrier.
template <class S, bool TR2>
__device__ __forceinline__ void walk_partial(double* sm, double* gw0, const double4_t (&acc)[4], const double (&bsum)[2],
                                             const double (&acc3)[3], int tid, int wave) {
    const int lane = tid & 63;
    lds_barrier();
    double* R = sm + S::RED; double* BS = sm + S::RBS; double* C3 = sm + S::RC3;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int q = 0; q < 4; ++q) R[((wave * 4 + nt) * 4 + q) * 64 + lane] = acc[nt][q];
#pragma unroll
    for (int k = 0; k < 2; ++k) {                                    // A rows (co, dy = 0): lanes co + 16 g
        double v = bsum[k];
        v += __shfl_xor(v, 16); v += __shfl_xor(v, 32);
        if (lane < 8) BS[(wave * 2 + k) * 8 + lane] = v;
    }
    if (tid < 432) C3[tid] = acc3[0];
    else if (tid >= 448) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double v = ft_wave_sum(acc3[k]);
            if (lane == 0) gw0[CB2 + k] = v;
        }
    }
    lds_barrier();
#pragma unroll
    for (int h = 0; h < 2; ++h) {                                    // element e = (nt, q, lane) = D_nt[row g + 4 q][col i]
        const int e = tid + NT * h, nt = e >> 8, q = (e >> 6) & 3, ln = e & 63;
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < 8; ++w) v += R[w * 1024 + e];
        const int g = ln >> 4, i = ln & 15, m = g + 4 * q, co = m & 7, dy = m >> 3;
        const int ncol = (nt < 3 ? nt * 16 : 0) + i;
        if (ncol < (nt < 3 ? 48 : 12)) {
            // conv1 (nt = 3) and conv2 as accumulated plainly: columns (ci, kx, kyb), ky = 2 kyb + d; conv2 transposed: (ci, ky, kxb), kx = 2 kxb + d
            const bool tr = TR2 && nt < 3;
            const int ci = ncol / 6, ka = (ncol % 6) >> 1, kb2 = 2 * (ncol & 1) + dy;
            const int ky = tr ? ka : kb2, kx = tr ? kb2 : ka;
            if (kb2 <= 2) gw0[(nt < 3 ? CW1 + (co * 8 + ci) * 9 : CW0 + (co * 2 + ci) * 9) + ky * 3 + kx] = v;
        }
    }
    if (tid < 16) {
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < 8; ++w) v += BS[w * 16 + tid];
        gw0[(tid < 8 ? CB1 : CB0) + (tid & 7)] = v;
    }
    if (tid < 216) gw0[CW2 + tid] = C3[tid] + C3[216 + tid];
}

}  // namespace fthmc_flow
