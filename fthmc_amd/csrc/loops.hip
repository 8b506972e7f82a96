// Rectangular Wilson loops W(R, T) of 2D U(1), the whole table of one configuration batch in three launches:
//   W[b][R-1][T-1] = (1 / L^2) sum_{i,j} cos theta,
//   theta = sum_{a<R} x0[i+a][j] + sum_{c<T} x1[i+R][j+c] - sum_{a<R} x0[i+a][j+T] - sum_{c<T} x1[i][j+c]      (indices mod L)
// (R = T = 1: the plaquette of k_plaq; T = L: the Polyakov-loop correlator at distance R).  With
//   E(i,j) = exp(i sum_{a<R} x0[i+a][j]),   d(i,j) = exp(i (x1[i+R][j] - x1[i][j]))
// everything a site needs lies in its own row i:  cos theta = Re[ E(i,j) conj(E(i,j+T)) prod_{c<T} d(i,j+c) ], so a thread keeps
// G_T = E(i,j) prod_{c<T} d(i,j+c) of its sites in registers and walks T = 1 .. Tmax with
//   W_T += Re[G_T conj(E(i,j+T))] (2 FMAs),   G_{T+1} = G_T d(i,j+T) (4 FMAs)
// and two 16-byte LDS reads per site and step: one sincos per link and extent R, no transcendental inside the walk.
// No atomics: every sum has a fixed order, two calls give the same bits.
#include "common.h"
#include "kernels.h"

namespace {

using fthmc::LP_THREADS;
using fthmc::LP_SITES;

// ---------------------------------------------------------------- prefix sums of x0 along i
// S[b][i][j] = sum_{a<i} x0[a][j], i = 0 .. L (row L: the column totals), one thread per column (coalesced in j), the running sum
// as an unevaluated pair hi + lo (two-sum), so that a stored prefix carries ONE rounding, 2^-53 |S|, instead of the i roundings of
// a plain recursive sum: the error of a segment sum is O(L) ulps of pi, not O(L^2) (tests/wilson_loop_cases.py derived_bound)
__global__ __launch_bounds__(FT_WAVE) void k_link_prefix(const double* __restrict__ x, int L, double* __restrict__ S) {
    const int b = blockIdx.x, j = blockIdx.y * FT_WAVE + threadIdx.x;
    if (j >= L) return;
    const double* x0 = x + (size_t)b * 2 * L * L + j;
    double* Sb = S + (size_t)b * (L + 1) * L + j;
    double hi = 0.0, lo = 0.0;
    Sb[0] = 0.0;
#pragma unroll 8
    for (int i = 0; i < L; ++i) {
        const double v = x0[(size_t)i * L];
        const double t = hi + v, bv = t - hi;
        lo += (hi - (t - bv)) + (v - bv);
        hi = t;
        Sb[(size_t)(i + 1) * L] = hi + lo;
    }
}

// sum_{a<R} x0[i+a][j] from the prefix sums: two loads, three where the segment wraps
__device__ __forceinline__ double lp_segment(const double* __restrict__ Sb, int L, int i, int R, int j) {
    const int e = i + R;
    if (e <= L) return Sb[(size_t)e * L + j] - Sb[(size_t)i * L + j];
    return (Sb[(size_t)L * L + j] - Sb[(size_t)i * L + j]) + Sb[(size_t)(e - L) * L + j];
}

// the planes E and d of rows i0 .. i0 + nrows - 1, [row][j] with row stride L
__device__ __forceinline__ void lp_build(const double* __restrict__ Sb, const double* __restrict__ x1, int L, int R, int i0, int nrows,
                                         double2* E, double2* d) {
    for (int s = threadIdx.x; s < nrows * L; s += LP_THREADS) {
        const int r = s / L, j = s - r * L, i = i0 + r;
        const int ir = i + R >= L ? i + R - L : i + R;
        double sn, cs;
        ft_sincos_wide(lp_segment(Sb, L, i, R, j), &sn, &cs);
        E[s] = make_double2(cs, sn);
        ft_sincos_wide(x1[(size_t)ir * L + j] - x1[(size_t)i * L + j], &sn, &cs);
        d[s] = make_double2(cs, sn);
    }
}

// The T walk of sites s0 <= s < s1 (site s = row s / L, column s % L of the planes), up to NS sites per thread, consecutive
// threads on consecutive sites; red[wave][T] receives the wave's sum.  No barrier inside.
// LDS banks (planes in LDS): a 16-byte read is served in four groups of 16 lanes, conflict-free when the 16 slots (16-byte units)
// of a group differ mod 16.  The lanes of a group hold 16 sites whose numbers differ mod 16 (a group is three runs of consecutive
// lanes that tile 0 .. 15 mod 16), and with row stride L the slot of site s at step T is s + T, or s + T - L where the column
// wrapped: for L % 16 == 0 both are s + T mod 16 -- every step of every group is conflict-free, whatever rows the wave spans.  A
// ragged L (12, 20: L % 16 != 0) pays a two-way conflict in the one group per row end that holds wrapped and unwrapped lanes.
template <int NS>
__device__ __forceinline__ void lp_walk(const double2* E, const double2* d, int L, int s0, int s1, int Tmax, double* red) {
    double gr[NS], gi[NS];
    int rb[NS], jt[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const int s = s0 + (int)threadIdx.x + k * LP_THREADS;
        const bool ok = s < s1;
        const int ss = ok ? s : s0;
        const int r = ss / L;
        rb[k] = r * L; jt[k] = ss - r * L;
        const double2 e = E[ss], dd = d[ss];
        gr[k] = ok ? e.x * dd.x - e.y * dd.y : 0.0;      // G_1 = E d; a slot without a site adds zeros
        gi[k] = ok ? e.x * dd.y + e.y * dd.x : 0.0;
    }
    const int lane = threadIdx.x & (FT_WAVE - 1), wave = threadIdx.x / FT_WAVE;
    for (int T = 0; T < Tmax; ++T) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            jt[k] = jt[k] + 1 == L ? 0 : jt[k] + 1;
            const double2 e2 = E[rb[k] + jt[k]], dn = d[rb[k] + jt[k]];
            acc += gr[k] * e2.x + gi[k] * e2.y;
            const double nr = gr[k] * dn.x - gi[k] * dn.y;
            gi[k] = gr[k] * dn.y + gi[k] * dn.x;
            gr[k] = nr;
        }
        acc = ft_wave_sum(acc);
        if (lane == 0) red[wave * Tmax + T] = acc;
    }
}

__device__ __forceinline__ void lp_store_partials(const double* red, int Tmax, double* __restrict__ out) {
    for (int T = threadIdx.x; T < Tmax; T += LP_THREADS)
        out[T] = ((red[T] + red[Tmax + T]) + red[2 * Tmax + T]) + red[3 * Tmax + T];
}

// ---------------------------------------------------------------- L <= LP_LDS_MAXL: one workgroup per (chain, R, block of rows)
// grid (B, Rmax, nblk); dynamic LDS: E and d of `rows` rows (32 B per site) + the four waves' partials red[4][Tmax]: at most
// 32 LP_SITES + 32 LP_LDS_MAXL bytes (L = Tmax = LP_LDS_MAXL), which must stay within the 64 KB a launch gets without opting in
static_assert(32 * LP_SITES + 32 * fthmc::LP_LDS_MAXL <= 65536, "k_wilson_loops: planes + red beyond the default dynamic LDS limit");
static_assert(LP_SITES % LP_THREADS == 0 && LP_SITES / LP_THREADS == 4 && LP_THREADS == 4 * FT_WAVE, "lp_walk<4>, red[4][Tmax]");
template <int NS>
__global__ __launch_bounds__(LP_THREADS) void k_wilson_loops(const double* __restrict__ x, const double* __restrict__ S, int L, int rows,
                                                             int Tmax, double* __restrict__ part) {
    extern __shared__ double2 lp_lds[];
    const int b = blockIdx.x, R = blockIdx.y + 1, blk = blockIdx.z, Rmax = gridDim.y, nblk = gridDim.z;
    const int i0 = blk * rows, nrows = L - i0 < rows ? L - i0 : rows;
    double2* E = lp_lds;
    double2* d = E + rows * L;
    double* red = reinterpret_cast<double*>(d + rows * L);
    lp_build(S + (size_t)b * (L + 1) * L, x + ((size_t)b * 2 + 1) * L * L, L, R, i0, nrows, E, d);
    __syncthreads();
    lp_walk<NS>(E, d, L, 0, nrows * L, Tmax, red);
    __syncthreads();
    lp_store_partials(red, Tmax, part + (((size_t)b * Rmax + (R - 1)) * nblk + blk) * Tmax);
}

// ---------------------------------------------------------------- L > LP_LDS_MAXL: a row no longer fits a workgroup's LDS share
// A fixed number of workgroups, each with a slot of global scratch (E and d of ONE row, red[4][Tmax]), walks the items
// (chain, R, row) in order; a row is walked in chunks of LP_SITES columns, each chunk one partial of the row: nblk = L nchunk
__global__ __launch_bounds__(LP_THREADS) void k_wilson_loops_big(const double* __restrict__ x, const double* __restrict__ S, int B, int L,
                                                                 int Rmax, int Tmax, int nchunk, double* scratch, double* __restrict__ part) {
    double* slot = scratch + (size_t)blockIdx.x * (4 * (size_t)L + 4 * (size_t)Tmax);
    double2* E = reinterpret_cast<double2*>(slot);
    double2* d = E + L;
    double* red = slot + 4 * (size_t)L;
    const long long nitem = (long long)B * Rmax * L;
    for (long long item = blockIdx.x; item < nitem; item += gridDim.x) {
        const int i = (int)(item % L);
        const long long br = item / L;
        const int R = (int)(br % Rmax) + 1;
        const size_t b = (size_t)(br / Rmax);
        lp_build(S + b * (L + 1) * L, x + (b * 2 + 1) * L * L, L, R, i, 1, E, d);
        __syncthreads();
        for (int c = 0; c < nchunk; ++c) {
            const int s0 = c * LP_SITES, s1 = s0 + LP_SITES < L ? s0 + LP_SITES : L;
            lp_walk<LP_SITES / LP_THREADS>(E, d, L, s0, s1, Tmax, red);
            __syncthreads();
            lp_store_partials(red, Tmax, part + ((size_t)item * nchunk + c) * Tmax);
            __syncthreads();
        }
    }
}

// W[b][R-1][T-1] = (sum of the nblk partials, in order) / L^2: a division, so that x = 0 gives exactly 1
__global__ void k_wilson_loops_fin(const double* __restrict__ part, long long n, int nblk, int Tmax, double vol, double* __restrict__ W) {
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const long long br = e / Tmax;
        const double* p = part + (size_t)br * nblk * Tmax + (size_t)(e - br * Tmax);
        double sum = 0.0;
        for (int k = 0; k < nblk; ++k) sum += p[(size_t)k * Tmax];
        W[e] = sum / vol;
    }
}
// Wmean[R-1][T-1] = (W[0] + W[1] + ... + W[B-1]) / B, the chains in index order
__global__ void k_wilson_loops_mean(const double* __restrict__ W, int B, long long nt, double* __restrict__ Wmean) {
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < nt; e += (long long)gridDim.x * blockDim.x) {
        double sum = 0.0;
#pragma unroll 8
        for (int b = 0; b < B; ++b) sum += W[(size_t)b * nt + e];
        Wmean[e] = sum / (double)B;
    }
}

inline unsigned lp_grid(long long n, int block) {
    const long long g = (n + block - 1) / block;
    return (unsigned)(g < 1 ? 1 : (g > (1 << 20) ? (1 << 20) : g));
}

}  // namespace

namespace fthmc {

int launch_wilson_loops(const double* x, int B, int L, int Rmax, int Tmax, double* W, double* Wmean, double* prefix, double* part,
                        double* scratch, hipStream_t s) {
    const LoopsGeom g = loops_geom(B, L, Rmax, Tmax);
    if (!g.ok) return FTHMC_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_link_prefix, dim3(B, (L + FT_WAVE - 1) / FT_WAVE), dim3(FT_WAVE), 0, s, x, L, prefix);
    FT_LAUNCH_CHECK();
    if (g.lds) {
        const dim3 grid(B, Rmax, g.nblk);
        const size_t lds = (size_t)g.rows * L * 32 + (size_t)4 * Tmax * sizeof(double);
        const int sites = g.rows * L;
        if (sites <= LP_THREADS)
            hipLaunchKernelGGL(k_wilson_loops<1>, grid, dim3(LP_THREADS), lds, s, x, prefix, L, g.rows, Tmax, part);
        else if (sites <= 2 * LP_THREADS)
            hipLaunchKernelGGL(k_wilson_loops<2>, grid, dim3(LP_THREADS), lds, s, x, prefix, L, g.rows, Tmax, part);
        else
            hipLaunchKernelGGL(k_wilson_loops<4>, grid, dim3(LP_THREADS), lds, s, x, prefix, L, g.rows, Tmax, part);
    } else {
        hipLaunchKernelGGL(k_wilson_loops_big, dim3(g.nwg), dim3(LP_THREADS), 0, s, x, prefix, B, L, Rmax, Tmax, g.nblk / L, scratch, part);
    }
    FT_LAUNCH_CHECK();
    const long long nt = (long long)Rmax * Tmax, n = nt * B;
    hipLaunchKernelGGL(k_wilson_loops_fin, dim3(lp_grid(n, 256)), dim3(256), 0, s, part, n, g.nblk, Tmax, (double)L * (double)L, W);
    FT_LAUNCH_CHECK();
    if (Wmean) {
        hipLaunchKernelGGL(k_wilson_loops_mean, dim3(lp_grid(nt, 64)), dim3(64), 0, s, W, B, nt, Wmean);
        FT_LAUNCH_CHECK();
    }
    return FTHMC_OK;
}

}  // namespace fthmc
