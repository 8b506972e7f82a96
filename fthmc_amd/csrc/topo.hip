// Instanton hits of 2D U(1) with the plaquette action: a Metropolis update across topological sectors (fthmc_instanton_hit,
// DESIGN 4.14).  With A the constant-field-strength configuration of charge 1,
//   A1[i][j] = (2 pi / L^2) i,      A0[L-1][j] = -(2 pi / L) j,      A0[i][j] = 0 for i < L - 1,
// x -> x + k A moves every plaquette by k w, w = 2 pi / L^2 (the one at (L-1, L-1) by k w - 2 pi k), so the action difference of a
// step k -> k + s, s = +-1, is a closed form in the two sums C = sum cos P, Sn = sum sin P of the field the call received:
//   dS = 2 beta s sin(w / 2) [C sin theta + Sn cos theta],      theta = (2 k + s) pi / L^2
// (the product form of beta [(cos k w - cos (k + s) w) C + (sin (k + s) w - sin k w) Sn]: nothing cancels).  A call reduces C and Sn
// once, runs its n_hit Metropolis steps as a scalar Markov chain in k on one lane, and applies the net k in one pass over the x1
// plane and the last row of x0.  Every angle is formed from an integer reduced first (topo_int.h): the shifts lie in [0, 2 pi)
// whatever k, and a link whose reduced integer is 0 is copied bit for bit.
// Draws: Philox4x32-10 under the chain's key at counter (hit0 + h, 0, 4, 0): u from words (0, 1), s from bit 0 of word 2.
// Two launch shapes -- one workgroup per chain, or one wave per workgroup + a decision kernel + an apply kernel for a few chains of a
// large lattice -- add the same numbers in the same order and run the same it_* functions on them: the same bits.
#include "common.h"
#include "kernels.h"
#include "rng_common.h"
#include "topo_int.h"

namespace {

using namespace fthmc_rng;
using fthmc::it_shift_num_seam;
using fthmc::it_shift_num_x1;
using fthmc::it_theta_num;

// (fp contract off in the functions that hold the update's arithmetic, as in local.hip: which products and sums become one FMA must
// not be left to the optimiser's view of different kernels -- the two launch shapes promise the same bits)

// the sums of cos P and sin P over the sites tid, tid + nthr, ... of one chain (tid of nthr: the thread's place in the chain's
// workgroup -- k_instanton_waves runs the workgroup's waves as workgroups of their own)
__device__ __forceinline__ void it_chain_sums(const double* x0, int L, int tid, int nthr, double& csum, double& ssum) {
#pragma clang fp contract(off)
    const int n = L * L;
    const double* x1 = x0 + n;
    double c = 0.0, q = 0.0;
    for (int s = tid; s < n; s += nthr) {
        const int i = s / L, j = s - i * L;
        const int ip = i + 1 == L ? 0 : i + 1, jp = j + 1 == L ? 0 : j + 1;
        const double P = ((x0[s] + x1[ip * L + j]) - x0[i * L + jp]) - x1[s];
        double sn, cs;
        ft_sincos_wide(P, &sn, &cs);
        c += cs;
        q += sn;
    }
    csum = c; ssum = q;
}

// dS of the step k -> k + s; sh = sin(pi / L^2)
__device__ __forceinline__ double it_delta_s(double C, double Sn, double beta, double sh, int k, int s, int L) {
#pragma clang fp contract(off)
    const double th = ((double)it_theta_num(k, s, L) * FT_PI) / (double)((int64_t)L * L);
    double st, ct;
    ft_sincos(th, &st, &ct);
    const double d = ((2.0 * beta) * sh) * (C * st + Sn * ct);
    return s > 0 ? d : -d;
}

// the n_hit Metropolis steps of one chain from k = 0 -> k; *nacc: the accepted ones.  seeds is read with n_hit > 0 only
__device__ __forceinline__ int it_hits(double C, double Sn, double beta, int L, const int64_t* seeds, int b, int n_hit, uint32_t hit0,
                                       int* nacc) {
#pragma clang fp contract(off)
    int k = 0, na = 0;
    if (n_hit > 0) {
        const uint64_t sd = (uint64_t)seeds[b];
        const uint32_t k0 = (uint32_t)sd, k1 = (uint32_t)(sd >> 32);
        double sh, ch;
        ft_sincos(FT_PI / (double)((int64_t)L * L), &sh, &ch);
        for (int h = 0; h < n_hit; ++h) {
            const u4 w = philox4x32_10(u4{hit0 + (uint32_t)h, 0u, 4u, 0u}, k0, k1);
            const double u = accept_uniform(w.x, w.y);
            const int s = (w.z & 1u) ? 1 : -1;
            const double dS = it_delta_s(C, Sn, beta, sh, k, s, L);
            if (u < exp(-dS)) { k += s; ++na; }
        }
    }
    *nacc = na;
    return k;
}

// link t of the x1 plane (row i = t / L) and link j of the last row of x0 under the net charge k; *moved: the value is a new one
__device__ __forceinline__ double it_shift_x1(double x, int k, int i, int L, bool* moved) {
#pragma clang fp contract(off)
    const int64_t r = it_shift_num_x1(k, i, L);
    *moved = r != 0;
    if (r == 0) return x;
    return ft_regularize(x + (FT_TWO_PI * (double)r) / (double)((int64_t)L * L));
}
__device__ __forceinline__ double it_shift_seam(double x, int k, int j, int L, bool* moved) {
#pragma clang fp contract(off)
    const int64_t r = it_shift_num_seam(k, j, L);
    *moved = r != 0;
    if (r == 0) return x;
    return ft_regularize(x - (FT_TWO_PI * (double)r) / (double)L);
}

// the links tid, tid + nthr, ... of one chain under the net charge k.  In place (xo == xb) only the links that move are written, and
// the walk starts at the last row of x0: all of x0 above it stays.  xb and xo may be the same: a link is read and written by one thread
__device__ __forceinline__ void it_apply(const double* xb, double* xo, int L, int k, int tid, int nthr) {
    const int n = L * L;
    const bool inplace = xo == xb;
    if (inplace && k == 0) return;
    for (int s = (inplace ? n - L : 0) + tid; s < 2 * n; s += nthr) {
        const double v = xb[s];
        bool moved = false;
        double o = v;
        if (s >= n) o = it_shift_x1(v, k, (s - n) / L, L, &moved);
        else if (s >= n - L) o = it_shift_seam(v, k, s - (n - L), L, &moved);
        if (moved || !inplace) xo[s] = o;
    }
}

__device__ __forceinline__ void it_store(int b, int k, int nacc, double C, double Sn, int32_t* k_out, int32_t* nacc_out, double* cs_out) {
    if (k_out) k_out[b] = k;
    if (nacc_out) nacc_out[b] = nacc;
    if (cs_out) { cs_out[2 * (size_t)b] = C; cs_out[2 * (size_t)b + 1] = Sn; }
}

// ---------------------------------------------------------------- one workgroup per chain, the whole call in one launch
template <bool PB>
__global__ __launch_bounds__(1024) void k_instanton(const double* x, int L, typename BetaArg<PB>::type beta_, const int64_t* __restrict__ seeds,
                                                    int n_hit, uint32_t hit0, double* x_out, int32_t* __restrict__ k_out,
                                                    int32_t* __restrict__ nacc_out, double* __restrict__ cs_out) {     // x_out may be x
    __shared__ double red[16];
    __shared__ int kk;
    const int b = blockIdx.x, n = L * L;
    const double* xb = x + (size_t)b * 2 * n;
    double c, q;
    it_chain_sums(xb, L, (int)threadIdx.x, (int)blockDim.x, c, q);
    c = ft_block_sum(c, red);
    q = ft_block_sum(q, red);
    if (threadIdx.x == 0) {
        int nacc;
        const int k = it_hits(c, q, beta_at(beta_, b), L, seeds, b, n_hit, hit0, &nacc);
        it_store(b, k, nacc, c, q, k_out, nacc_out, cs_out);
        kk = k;
    }
    __syncthreads();                               // also: every read of the sums is behind it before a link is written in place
    it_apply(xb, x_out + (size_t)b * 2 * n, L, kk, (int)threadIdx.x, (int)blockDim.x);
}

// ---------------------------------------------------------------- a few chains of a large lattice: the same sums by the same threads
// wave w of chain b's workgroup as a workgroup of its own (grid B x nw), its two wave sums in part[b][w][2]
__global__ __launch_bounds__(FT_WAVE) void k_instanton_waves(const double* __restrict__ x, int L, double* __restrict__ part) {
    const int b = blockIdx.x, w = blockIdx.y, nw = gridDim.y;
    double c, q;
    it_chain_sums(x + (size_t)b * 2 * L * L, L, w * FT_WAVE + (int)threadIdx.x, nw * FT_WAVE, c, q);
    c = ft_wave_sum(c);
    q = ft_wave_sum(q);
    if (threadIdx.x == 0) { part[((size_t)b * nw + w) * 2] = c; part[((size_t)b * nw + w) * 2 + 1] = q; }
}
// a thread per chain: the partials added as ft_block_sum does (0.0 + wave 0 + wave 1 + ...), the hit chain, k for k_instanton_apply
template <bool PB>
__global__ __launch_bounds__(FT_WAVE) void k_instanton_decide(const double* __restrict__ part, int nw, int B, int L,
                                                              typename BetaArg<PB>::type beta_, const int64_t* __restrict__ seeds, int n_hit,
                                                              uint32_t hit0, int32_t* __restrict__ kbuf, int32_t* __restrict__ k_out,
                                                              int32_t* __restrict__ nacc_out, double* __restrict__ cs_out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double c = 0.0, q = 0.0;
    for (int w = 0; w < nw; ++w) { c += part[((size_t)b * nw + w) * 2]; q += part[((size_t)b * nw + w) * 2 + 1]; }
    int nacc;
    const int k = it_hits(c, q, beta_at(beta_, b), L, seeds, b, n_hit, hit0, &nacc);
    it_store(b, k, nacc, c, q, k_out, nacc_out, cs_out);
    kbuf[b] = k;
}
// grid-stride over a chain's links: the chain on grid x, up to 64 workgroups of 256 threads per chain on grid y
__global__ __launch_bounds__(256) void k_instanton_apply(const double* x, int L, const int32_t* __restrict__ kbuf, double* x_out) {
    const int b = blockIdx.x;
    const size_t off = (size_t)b * 2 * L * L;
    it_apply(x + off, x_out + off, L, kbuf[b], (int)(blockIdx.y * 256 + threadIdx.x), (int)(gridDim.y * 256));
}

}  // namespace

namespace fthmc {

int launch_instanton(const double* x, int B, int L, double beta, const double* beta_b, const int64_t* seeds, int n_hit, uint32_t hit0,
                     bool split, double* x_out, int32_t* k_out, int32_t* nacc_out, double* cs_out, double* part, int32_t* kbuf, hipStream_t s) {
    const int nt = chain_threads(L);
    if (!split) {
        if (beta_b) hipLaunchKernelGGL(k_instanton<true>, dim3(B), dim3(nt), 0, s, x, L, beta_b, seeds, n_hit, hit0, x_out, k_out, nacc_out, cs_out);
        else hipLaunchKernelGGL(k_instanton<false>, dim3(B), dim3(nt), 0, s, x, L, beta, seeds, n_hit, hit0, x_out, k_out, nacc_out, cs_out);
        FT_LAUNCH_CHECK();
        return FTHMC_OK;
    }
    const int nw = nt / FT_WAVE;
    hipLaunchKernelGGL(k_instanton_waves, dim3(B, nw), dim3(FT_WAVE), 0, s, x, L, part);
    FT_LAUNCH_CHECK();
    const dim3 gd((B + FT_WAVE - 1) / FT_WAVE);
    if (beta_b) hipLaunchKernelGGL(k_instanton_decide<true>, gd, dim3(FT_WAVE), 0, s, part, nw, B, L, beta_b, seeds, n_hit, hit0, kbuf, k_out, nacc_out, cs_out);
    else hipLaunchKernelGGL(k_instanton_decide<false>, gd, dim3(FT_WAVE), 0, s, part, nw, B, L, beta, seeds, n_hit, hit0, kbuf, k_out, nacc_out, cs_out);
    FT_LAUNCH_CHECK();
    const long long blocks = (2LL * L * L + 255) / 256;
    hipLaunchKernelGGL(k_instanton_apply, dim3(B, (unsigned)(blocks > 64 ? 64 : blocks)), dim3(256), 0, s, x, L, kbuf, x_out);
    FT_LAUNCH_CHECK();
    return FTHMC_OK;
}

}  // namespace fthmc
