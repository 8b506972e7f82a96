// Local updates of 2D U(1) with the plaquette action: heatbath and overrelaxation sweeps (fthmc_local_update).
// A link sits in two plaquettes, so its conditional weight is exp(kappa cos(x - phi)) with A = exp(i a) + exp(-i b) = |A| e^{-i phi},
//   x0[i][j]:  a = x1[i+1][j] - x0[i][j+1] - x1[i][j],       b = x0[i][j-1] + x1[i+1][j-1] - x1[i][j-1]
//   x1[i][j]:  a = -(x0[i][j] + x1[i+1][j] - x0[i][j+1]),    b = -(x0[i-1][j] - x0[i-1][j+1] - x1[i-1][j])
// and A = 2 cos((a + b) / 2) exp(i (a - b) / 2) in closed form: kappa = 2 beta |cos h|, h = (a + b) / 2, phi = (b - a) / 2 (+ pi where
// cos h < 0) -- one cosine, no atan2, no square root, and phi is as well conditioned as a and b themselves wherever cos h is away from 0.
//   overrelaxation: x <- regularize(2 phi - x) = regularize((b - a) - x): no transcendental at all, the two plaquettes exchange angles
//   heatbath: Best-Fisher rejection for von Mises(kappa), x <- regularize(phi +- acos f), at most LU_MAX_ATTEMPTS attempts
// x0 links of one parity of j (x1 links of one parity of i) read only links of the other three classes: a class is updated in place.
// Draws: Philox4x32-10 under the chain's key at counter (site i L + j, heatbath sweep, 3, mu << 8 | attempt) -- nothing of the batch,
// the launch geometry or the path enters, and both paths run lu_update on the same loaded values: they give the same bits.
#include "common.h"
#include "kernels.h"
#include "rng_common.h"

namespace {

using namespace fthmc_rng;
using fthmc::LU_MAXL;
using fthmc::LU_MAX_ATTEMPTS;

// below it 1 + 4 kappa^2 and every other place kappa enters round to their kappa = 0 values long since: the draw is the algorithm's
// own limit r -> inf, f = z, c = 1 (accepted at once): uniform on the circle.  Above it nothing of the setup cancels (rho below)
constexpr double LU_KAPPA_MIN = 8.673617379884035e-19;      // 2^-60

// the staple angles from the six neighbours in the order the callers load them (lu_neighbours)
// (fp contract off in the three functions that hold the update's arithmetic: which products and sums become one FMA must not be left
// to the optimiser's view of two different kernels -- the two paths promise the same bits)
__device__ __forceinline__ void lu_staples(int mu, const double* v, double* a, double* b) {
#pragma clang fp contract(off)
    if (mu == 0) { *a = (v[0] - v[1]) - v[2]; *b = (v[3] + v[4]) - v[5]; }
    else { *a = -((v[0] + v[1]) - v[2]); *b = -((v[3] - v[4]) - v[5]); }
}

__device__ __forceinline__ double lu_overrelax(double x, double a, double b) {
#pragma clang fp contract(off)
    return ft_regularize((b - a) - x);
}

// One heatbath draw.  Best & Fisher (1979): tau = 1 + sqrt(1 + 4 kappa^2), rho = (tau - sqrt(2 tau)) / 2 kappa, r = (1 + rho^2) / 2 rho;
// rho is formed as 2 kappa / (tau + sqrt(2 tau)) -- the same number ((tau - sqrt(2 tau))(tau + sqrt(2 tau)) = tau (tau - 2) = 4 kappa^2)
// without the cancellation that costs the textbook form its digits below kappa ~ 1e-6 and makes it 0 / 0 at kappa = 0.
// The loop is bounded: a link that is never accepted (probability < 0.34^64) keeps xold.
__device__ __forceinline__ double lu_heatbath(double xold, double a, double b, double beta, uint32_t k0, uint32_t k1, uint32_t site,
                                              uint32_t mu, uint32_t sweep) {
#pragma clang fp contract(off)
    double sn, ch;
    ft_sincos_wide(0.5 * (a + b), &sn, &ch);
    const double kappa = 2.0 * beta * fabs(ch);
    double phi = 0.5 * (b - a);
    if (ch < 0.0) phi += FT_PI;
    const bool flat = !(kappa >= LU_KAPPA_MIN);
    double r = 1.0;
    if (!flat) {
        const double tau = 1.0 + sqrt(1.0 + 4.0 * kappa * kappa);
        const double rho = 2.0 * kappa / (tau + sqrt(2.0 * tau));
        r = (1.0 + rho * rho) / (2.0 * rho);
    }
    double out = xold;
    for (int t = 0; t < LU_MAX_ATTEMPTS; ++t) {
        const u4 w = philox4x32_10(u4{site, sweep, 3u, (mu << 8) | (uint32_t)t}, k0, k1);
        const double u1 = u53(w.x, w.y), u2 = u53(w.z, w.w);
        double sz, z;
        ft_sincos(FT_PI * u1, &sz, &z);
        double f = z;
        bool take = true;
        if (!flat) {
            f = (1.0 + r * z) / (r + z);
            f = fmin(fmax(f, -1.0), 1.0);                         // r + z = 0 (kappa beyond 1e7, z = -1): 0 / 0 becomes -1
            const double c = kappa * (r - f);
            take = c * (2.0 - c) - u2 > 0.0 || log(c / u2) + 1.0 - c >= 0.0;
        }
        if (take) {
            const double th = acos(f);
            out = ft_regularize((w.y & 1u) ? phi - th : phi + th);
            break;
        }
    }
    return out;
}

template <bool HEAT>
__device__ __forceinline__ double lu_update(double x, int mu, const double* v, double beta, uint32_t k0, uint32_t k1, uint32_t site,
                                            uint32_t sweep) {
    double a, b;
    lu_staples(mu, v, &a, &b);
    if (HEAT) return lu_heatbath(x, a, b, beta, k0, k1, site, (uint32_t)mu, sweep);
    return lu_overrelax(x, a, b);
}

// the six neighbours of link (mu, i, j) as (plane, row, column), in lu_staples' order
struct LuNb { int pl[6], r[6], c[6]; };
__device__ __forceinline__ LuNb lu_neighbours(int mu, int i, int j, int L) {
    const int ip = i + 1 == L ? 0 : i + 1, im = i == 0 ? L - 1 : i - 1, jp = j + 1 == L ? 0 : j + 1, jm = j == 0 ? L - 1 : j - 1;
    if (mu == 0) return LuNb{{1, 0, 1, 0, 1, 1}, {ip, i, i, i, ip, i}, {j, jp, j, jm, jm, jm}};
    return LuNb{{0, 1, 0, 0, 0, 1}, {i, ip, i, im, im, im}, {j, j, jp, j, jp, j}};
}

// link e of class (mu, p): the x0 links of column parity p row by row, the x1 links of row parity p row by row
__device__ __forceinline__ void lu_link(int mu, int p, int e, int L, int* i, int* j) {
    if (mu == 0) { const int hl = L >> 1, r = e / hl; *i = r; *j = 2 * (e - r * hl) + p; }
    else { const int r = e / L; *i = 2 * r + p; *j = e - r * L; }
}

// ---------------------------------------------------------------- any L: one launch per class, in place, the chain on grid x
// the links of class (mu, p) of chain b that this workgroup of the launch owns (k_local_class, k_anneal_class)
template <bool HEAT>
__device__ __forceinline__ void lu_class_links(double* __restrict__ x, int L, double beta, const int64_t* __restrict__ seeds, int mu, int p,
                                               uint32_t sweep) {
    const int b = blockIdx.x, n = L * L;
    uint32_t k0 = 0u, k1 = 0u;
    if (HEAT) { const uint64_t sd = (uint64_t)seeds[b]; k0 = (uint32_t)sd; k1 = (uint32_t)(sd >> 32); }
    double* xb = x + (size_t)b * 2 * n;
    for (int e = blockIdx.y * 256 + threadIdx.x; e < n / 2; e += gridDim.y * 256) {
        int i, j;
        lu_link(mu, p, e, L, &i, &j);
        const LuNb nb = lu_neighbours(mu, i, j, L);
        double v[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) v[q] = xb[(size_t)nb.pl[q] * n + (size_t)nb.r[q] * L + nb.c[q]];
        double* own = xb + (size_t)mu * n + (size_t)i * L + j;
        *own = lu_update<HEAT>(*own, mu, v, beta, k0, k1, (uint32_t)(i * L + j), sweep);
    }
}

template <bool HEAT, bool PB>
__global__ __launch_bounds__(256) void k_local_class(double* __restrict__ x, int L, typename BetaArg<PB>::type beta_,
                                                     const int64_t* __restrict__ seeds, int mu, int p, uint32_t sweep) {
    lu_class_links<HEAT>(x, L, beta_at(beta_, (int)blockIdx.x), seeds, mu, p, sweep);
}

// ---------------------------------------------------------------- L <= LU_MAXL: the whole call in one launch, one workgroup per chain
// Both planes live in LDS, each split by the PARITY OF THE COLUMN: slot(mu, i, j) = mu 2 H + (j & 1) H + i L / 2 + (j >> 1),
// H = L^2 / 2 + 16.  Then
//   * an x0 class owns one half of plane 0, consecutive threads on consecutive slots (reads and writes of the own link), its x0
//     neighbours (columns j +- 1) are consecutive slots of the other half and its x1 neighbours (columns j, j - 1) consecutive slots
//     of the two halves of plane 1: every access of a wave is a run of consecutive 8-byte slots, conflict-free, where the row-major
//     plane would give stride-2 (two-way) reads and writes;
//   * an x1 class owns whole rows: consecutive threads alternate between the halves, 16 slots each per 32 lanes, and the 16 doubles
//     of padding in H put the two runs on the two halves of the 64 banks (L >= 32; a smaller lattice has several rows per 32 lanes and
//     pays a two-way conflict on some of them: its call is launch latency, not LDS).
// A thread keeps the coordinates of its links (formed once, two divisions per link) and owns the same links of a class throughout.
// The six neighbour slots are re-formed from them at every update (wrap selects and adds, ~30 integer instructions against ~700 of a
// heatbath draw): kept, they would be 7 indices x 4 classes x LU_PER links = 56 registers on top of the 123 the kernel holds (126 with the
// annealing step loop around it), beyond the 128 a lane of a 1024-thread workgroup may have.
constexpr int LU_NT = 1024, LU_PER = LU_MAXL * LU_MAXL / 2 / LU_NT, LU_PAD = 16;
static_assert(LU_PER * LU_NT * 2 == LU_MAXL * LU_MAXL, "k_local_resident: LU_PER links per thread and class cover L = LU_MAXL");
constexpr int LU_LDS = 2 * (LU_MAXL * LU_MAXL + 2 * LU_PAD);       // doubles of a chain in LDS

// a thread per link of a class, whole waves, at most LU_NT: the workgroup of the one-launch kernels (and of the annealing work kernel)
inline int lu_threads(int L) {
    const int nt = (L * L / 2 + FT_WAVE - 1) / FT_WAVE * FT_WAVE;
    return nt > LU_NT ? LU_NT : nt;
}

struct LuLds {                                                      // the slot layout above
    int L, n, hl, H;
    __device__ __forceinline__ explicit LuLds(int L_) : L(L_), n(L_ * L_), hl(L_ >> 1), H(L_ * L_ / 2 + LU_PAD) {}
    __device__ __forceinline__ int slot(int mu, int i, int j) const { return mu * 2 * H + (j & 1) * H + i * hl + (j >> 1); }
};
// a chain between global memory (row-major planes) and LDS
__device__ __forceinline__ void lu_lds_load(double* sx, const LuLds& g, const double* xb, int tid, int nt) {
    const int n = g.n;
    for (int s = tid; s < 2 * n; s += nt) {
        const int mu = s >= n ? 1 : 0, t = s - mu * n, i = t / g.L, j = t - i * g.L;
        sx[g.slot(mu, i, j)] = xb[s];
    }
}
__device__ __forceinline__ void lu_lds_store(const double* sx, const LuLds& g, double* xo, int tid, int nt) {
    const int n = g.n;
    for (int s = tid; s < 2 * n; s += nt) {
        const int mu = s >= n ? 1 : 0, t = s - mu * n, i = t / g.L, j = t - i * g.L;
        xo[s] = sx[g.slot(mu, i, j)];
    }
}
// the links a thread owns: link e = tid + k nt of every class, as (row, half column) of x0 and (half row, column) of x1
struct LuOwn {
    int r0[LU_PER], q0[LU_PER], r1[LU_PER], c1[LU_PER];
    bool have[LU_PER];
    __device__ __forceinline__ LuOwn(const LuLds& g, int tid, int nt) {
#pragma unroll
        for (int k = 0; k < LU_PER; ++k) {
            const int e = tid + k * nt;
            have[k] = e < g.n / 2;
            const int ee = have[k] ? e : 0;
            r0[k] = ee / g.hl; q0[k] = ee - r0[k] * g.hl;
            r1[k] = ee / g.L; c1[k] = ee - r1[k] * g.L;
        }
    }
};
// nsweep compound sweeps of the chain in LDS at one beta, from heatbath sweep `sweep` on -> the next heatbath sweep's index.
// Behind a barrier, and every class ends in one
__device__ __forceinline__ uint32_t lu_lds_sweeps(double* sx, const LuLds& g, const LuOwn& o, double beta, uint32_t k0, uint32_t k1, int n_hb,
                                                  int n_or, int nsweep, uint32_t sweep, int classes) {
    for (int sw = 0; sw < nsweep; ++sw)
        for (int h = 0; h < n_hb + n_or; ++h) {
            const bool heat = h < n_hb;
            for (int cl = 0; cl < 4; ++cl) {
                if (!((classes >> cl) & 1)) continue;               // uniform over the workgroup, as is every loop bound here
                const int mu = cl >> 1, p = cl & 1;
#pragma unroll
                for (int k = 0; k < LU_PER; ++k)
                    if (o.have[k]) {
                        const int i = mu == 0 ? o.r0[k] : 2 * o.r1[k] + p, j = mu == 0 ? 2 * o.q0[k] + p : o.c1[k];
                        const LuNb nb = lu_neighbours(mu, i, j, g.L);
                        double v[6];
#pragma unroll
                        for (int q = 0; q < 6; ++q) v[q] = sx[g.slot(nb.pl[q], nb.r[q], nb.c[q])];
                        const int own = g.slot(mu, i, j);
                        const uint32_t site = (uint32_t)(i * g.L + j);
                        sx[own] = heat ? lu_update<true>(sx[own], mu, v, beta, k0, k1, site, sweep)
                                       : lu_update<false>(sx[own], mu, v, beta, k0, k1, site, sweep);
                    }
                __syncthreads();
            }
            if (heat) ++sweep;
        }
    return sweep;
}

template <bool PB>
__global__ __launch_bounds__(LU_NT) void k_local_resident(const double* x, int L, typename BetaArg<PB>::type beta_,
                                                          const int64_t* __restrict__ seeds, int n_hb, int n_or, int nsweep,
                                                          uint32_t sweep0, int classes, double* x_out) {     // x_out may be x
    __shared__ double sx[LU_LDS];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, n = L * L;
    const double beta = beta_at(beta_, b);
    uint32_t k0 = 0u, k1 = 0u;
    if (n_hb > 0) { const uint64_t sd = (uint64_t)seeds[b]; k0 = (uint32_t)sd; k1 = (uint32_t)(sd >> 32); }
    const LuLds g(L);
    lu_lds_load(sx, g, x + (size_t)b * 2 * n, tid, nt);
    const LuOwn own(g, tid, nt);
    __syncthreads();
    lu_lds_sweeps(sx, g, own, beta, k0, k1, n_hb, n_or, nsweep, sweep0, classes);
    lu_lds_store(sx, g, x_out + (size_t)b * 2 * n, tid, nt);
}

// ---------------------------------------------------------------- annealing: a ramp of beta with the work it costs (fthmc_anneal, 4.17)
// Step k of a chain: C_k = sum cos P(x_k), W += (beta_k - beta_{k+1}) C_k, then the compound sweeps at beta_{k+1}.  The sum is stated
// once, over a reader of the links: thread tid of nt adds the sites tid, tid + nt, ... from 0.0, ft_block_sum adds the threads.  The
// one-launch kernel reads LDS and the work kernel of the sequenced path global memory, with the same nt (lu_threads): the same
// numbers in the same order, the same bits -- the rule of topo.hip's two shapes.
template <class At>
__device__ __forceinline__ double an_cos_sum(At at, int L, int tid, int nt) {
#pragma clang fp contract(off)
    const int n = L * L;
    double c = 0.0;
    for (int s = tid; s < n; s += nt) {
        const int i = s / L, j = s - i * L;
        const int ip = i + 1 == L ? 0 : i + 1, jp = j + 1 == L ? 0 : j + 1;
        const double P = ((at(0, i, j) + at(1, ip, j)) - at(0, i, jp)) - at(1, i, j);
        double sn, cs;
        ft_sincos_wide(P, &sn, &cs);
        c += cs;
    }
    return c;
}
// the work of one step: the difference, the product and the sum each rounded
__device__ __forceinline__ double an_work(double W, double beta_k, double beta_next, double C) {
#pragma clang fp contract(off)
    const double d = beta_k - beta_next;
    const double t = d * C;
    return W + t;
}
// a value every lane holds alike, moved to scalar registers: beta of a step is read from memory inside the step loop, where the
// compiler cannot prove the load uniform AND unclobbered, and as a vector value it would cost the heatbath two registers
__device__ __forceinline__ double an_uniform(double v) {
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)u);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(u >> 32));
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// The whole ramp in one launch: k_local_resident's walk inside a step loop.  The sum runs between two barriers out of LDS with
// nothing of a link alive but the owner's coordinates.  ft_block_sum leaves C_k in every lane, so every lane forms the same W: it is
// kept as a scalar pair (an_uniform) from work_in to the one store of work_out -- as a vector value it is the two registers that
// push the heatbath's 123 beyond what the allocator can hold without scratch (measured: 128 + 12 bytes of scratch, against 126 and
// none).  betas[k + 1] is one address for the workgroup: every lane reads it and an_uniform makes it the scalar the walk takes, so no
// lane has to broadcast it through LDS
__global__ __launch_bounds__(LU_NT) void k_anneal_resident(const double* x, int L, const double* betas, int n_step,
                                                           const int64_t* __restrict__ seeds, int n_hb, int n_or, int nsweep, uint32_t sweep0,
                                                           const double* work_in, double* x_out, double* work_out,
                                                           double* c_trace) {     // x_out may be x, work_out may be work_in
    __shared__ double sx[LU_LDS];
    __shared__ double red[16];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, n = L * L;
    uint32_t k0 = 0u, k1 = 0u;
    if (n_hb > 0) { const uint64_t sd = (uint64_t)seeds[b]; k0 = (uint32_t)sd; k1 = (uint32_t)(sd >> 32); }
    const LuLds g(L);
    lu_lds_load(sx, g, x + (size_t)b * 2 * n, tid, nt);
    const LuOwn own(g, tid, nt);
    double W = an_uniform(work_in ? work_in[b] : 0.0);
    double beta = an_uniform(betas[0]);
    uint32_t sweep = sweep0;
    __syncthreads();
    for (int k = 0;; ++k) {
        double C = an_cos_sum([&](int mu, int i, int j) { return sx[g.slot(mu, i, j)]; }, L, tid, nt);
        C = ft_block_sum(C, red);
        if (tid == 0 && c_trace) c_trace[(size_t)b * ((size_t)n_step + 1) + k] = C;
        if (k == n_step) break;
        const double beta_next = an_uniform(betas[k + 1]);
        W = an_uniform(an_work(W, beta, beta_next, C));
        beta = beta_next;
        sweep = lu_lds_sweeps(sx, g, own, beta, k0, k1, n_hb, n_or, nsweep, sweep, 15);
    }
    if (tid == 0) work_out[b] = W;
    lu_lds_store(sx, g, x_out + (size_t)b * 2 * n, tid, nt);
}

// The sequenced path, any L.  Its work kernel: one workgroup of lu_threads(L) per chain, step k's C out of global memory;
// update: W = win[b] (null: 0) + (betas[0] - betas[1]) C, else W is copied (the last entry of the trace, n_step = 0)
__global__ __launch_bounds__(LU_NT) void k_anneal_work(const double* __restrict__ x, int L, const double* __restrict__ betas, int update,
                                                       const double* win, double* wout, double* c_out, size_t c_stride) {
    __shared__ double red[16];
    const int b = blockIdx.x, n = L * L;
    const double* x0 = x + (size_t)b * 2 * n;
    double C = an_cos_sum([&](int mu, int i, int j) { return x0[(size_t)mu * n + (size_t)i * L + j]; }, L, (int)threadIdx.x, (int)blockDim.x);
    C = ft_block_sum(C, red);
    if (threadIdx.x == 0) {
        double W = win ? win[b] : 0.0;
        if (update) W = an_work(W, betas[0], betas[1], C);
        wout[b] = W;
        if (c_out) c_out[(size_t)b * c_stride] = C;
    }
}
// ... and its class kernels: k_local_class' links at the beta the step's entry of the schedule holds
template <bool HEAT>
__global__ __launch_bounds__(256) void k_anneal_class(double* __restrict__ x, int L, const double* __restrict__ beta_dev,
                                                      const int64_t* __restrict__ seeds, int mu, int p, uint32_t sweep) {
    lu_class_links<HEAT>(x, L, *beta_dev, seeds, mu, p, sweep);
}

template <bool HEAT>
int lu_launch_class(double* x, int B, int L, double beta, const double* beta_b, const int64_t* seeds, int cl, uint32_t sweep, hipStream_t s) {
    const long long blocks = ((long long)L * L / 2 + 255) / 256;
    const dim3 grid((unsigned)B, (unsigned)(blocks > 65535 ? 65535 : blocks));
    if (beta_b) hipLaunchKernelGGL((k_local_class<HEAT, true>), grid, dim3(256), 0, s, x, L, beta_b, seeds, cl >> 1, cl & 1, sweep);
    else hipLaunchKernelGGL((k_local_class<HEAT, false>), grid, dim3(256), 0, s, x, L, beta, seeds, cl >> 1, cl & 1, sweep);
    FT_LAUNCH_CHECK();
    return FTHMC_OK;
}

}  // namespace

namespace fthmc {

int launch_local_update(const double* x, int B, int L, double beta, const double* beta_b, const int64_t* seeds, int n_hb, int n_or,
                        int nsweep, uint32_t sweep0, int classes, double* x_out, bool resident, hipStream_t s) {
    if (resident) {
        if (L > LU_MAXL) return FTHMC_ERR_UNSUPPORTED;
        const int nt = lu_threads(L);
        if (beta_b) hipLaunchKernelGGL(k_local_resident<true>, dim3(B), dim3(nt), 0, s, x, L, beta_b, seeds, n_hb, n_or, nsweep, sweep0, classes, x_out);
        else hipLaunchKernelGGL(k_local_resident<false>, dim3(B), dim3(nt), 0, s, x, L, beta, seeds, n_hb, n_or, nsweep, sweep0, classes, x_out);
        FT_LAUNCH_CHECK();
        return FTHMC_OK;
    }
    if (x_out != x && hipMemcpyAsync(x_out, x, (size_t)B * 2 * L * L * sizeof(double), hipMemcpyDeviceToDevice, s) != hipSuccess)
        return FTHMC_ERR_LAUNCH;
    uint32_t sweep = sweep0;
    for (int sw = 0; sw < nsweep; ++sw)
        for (int h = 0; h < n_hb + n_or; ++h) {
            const bool heat = h < n_hb;
            for (int cl = 0; cl < 4; ++cl) {
                if (!((classes >> cl) & 1)) continue;
                const int rc = heat ? lu_launch_class<true>(x_out, B, L, beta, beta_b, seeds, cl, sweep, s)
                                    : lu_launch_class<false>(x_out, B, L, beta, beta_b, seeds, cl, sweep, s);
                if (rc != FTHMC_OK) return rc;
            }
            if (heat) ++sweep;
        }
    return FTHMC_OK;
}

int launch_anneal(const double* x, int B, int L, const double* betas, int n_step, const int64_t* seeds, int n_hb, int n_or, int nsweep,
                  uint32_t sweep0, const double* work_in, double* x_out, double* work_out, double* c_trace, bool resident, hipStream_t s) {
    const int nt = lu_threads(L);
    if (resident) {
        if (L > LU_MAXL) return FTHMC_ERR_UNSUPPORTED;
        hipLaunchKernelGGL(k_anneal_resident, dim3(B), dim3(nt), 0, s, x, L, betas, n_step, seeds, n_hb, n_or, nsweep, sweep0, work_in, x_out,
                           work_out, c_trace);
        FT_LAUNCH_CHECK();
        return FTHMC_OK;
    }
    if (x_out != x && hipMemcpyAsync(x_out, x, (size_t)B * 2 * L * L * sizeof(double), hipMemcpyDeviceToDevice, s) != hipSuccess)
        return FTHMC_ERR_LAUNCH;
    const size_t stride = (size_t)n_step + 1;
    const long long blocks = ((long long)L * L / 2 + 255) / 256;
    const dim3 grid((unsigned)B, (unsigned)(blocks > 65535 ? 65535 : blocks));
    uint32_t sweep = sweep0;
    for (int k = 0; k < n_step; ++k) {
        hipLaunchKernelGGL(k_anneal_work, dim3(B), dim3(nt), 0, s, x_out, L, betas + k, 1, k == 0 ? work_in : work_out, work_out,
                           c_trace ? c_trace + k : nullptr, stride);
        FT_LAUNCH_CHECK();
        for (int sw = 0; sw < nsweep; ++sw)
            for (int h = 0; h < n_hb + n_or; ++h) {
                const bool heat = h < n_hb;
                for (int cl = 0; cl < 4; ++cl) {
                    if (heat) hipLaunchKernelGGL(k_anneal_class<true>, grid, dim3(256), 0, s, x_out, L, betas + k + 1, seeds, cl >> 1, cl & 1, sweep);
                    else hipLaunchKernelGGL(k_anneal_class<false>, grid, dim3(256), 0, s, x_out, L, betas + k + 1, seeds, cl >> 1, cl & 1, sweep);
                    FT_LAUNCH_CHECK();
                }
                if (heat) ++sweep;
            }
    }
    if (n_step == 0 || c_trace) {                                   // the final field's entry of the trace; n_step = 0: the work is copied
        hipLaunchKernelGGL(k_anneal_work, dim3(B), dim3(nt), 0, s, x_out, L, betas + n_step, 0, n_step == 0 ? work_in : work_out, work_out,
                           c_trace ? c_trace + n_step : nullptr, stride);
        FT_LAUNCH_CHECK();
    }
    return FTHMC_OK;
}

}  // namespace fthmc
