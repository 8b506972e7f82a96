// Boundary-condition tempering of 2D U(1) (fthmc_defect_*): plain HMC whose action carries a per-chain coupling on a
// short line of plaquettes, the defect
//   D = {((i0 + a) mod L, j0) : 0 <= a < Ld},      g_b = beta c_b, c_b in [0, 1]  (0: the line is open, 1: the periodic lattice).
// With C = sum over all plaquettes of cos P (BatchAction's order) and Dsum = sum over D of the same cosines
//   S_d = (-beta) C + (beta - g_b) Dsum,      H = S_d + sum v^2 / 2,
//   gP(p) = w(p) sin P(p),  w = g_b on D, beta elsewhere,      F0 = gP(i,j) - gP(i,j-1),  F1 = gP(i-1,j) - gP(i,j).
// With g_b = beta the second term of S_d is an exact zero and every weight is beta: each kernel here then does the arithmetic of
// its per-chain-beta twin in wilson.hip.  Two trajectory shapes: k_defect_trajectory (L <= 64: one launch, one workgroup per chain,
// the resident plan of traj_resident.h with one weight per owned site) and the sequenced one for any L (api.hip: k_defect_sums,
// k_defect_gp, k_defect_energy and the plain kick / shift / kinetic / Metropolis kernels).  No atomics anywhere.
#include "common.h"
#include "kernels.h"
#include "traj_resident.h"

namespace {

using fthmc::DefectLine;

// is the plaquette at site (i, j) on the defect?  (0 <= i0 < L, 0 <= Ld <= L: i - i0 + L lies in [1, 2 L))
__device__ __forceinline__ bool df_on(const DefectLine& d, int L, int i, int j) {
    int a = i - d.i0;
    a = a < 0 ? a + L : a;
    return j == d.j0 && a < d.Ld;
}

// the integer charge of a chain from its sum of wrapped plaquettes (a zero comes out as +0 whatever the sign of the sum)
__device__ __forceinline__ double df_charge(double q) {
    const double r = rint(q / FT_TWO_PI);
    return r == 0.0 ? 0.0 : r;
}

// sin and cos of the plaquette at site (i, j), the force kernels' order of the four links
__device__ __forceinline__ void df_sincos_site(const double* __restrict__ x0, const double* __restrict__ x1, int L, int i, int j,
                                               double* sn, double* cs) {
    const int ip = i + 1 == L ? 0 : i + 1, jp = j + 1 == L ? 0 : j + 1;
    ft_sincos(x0[i * L + j] - x1[i * L + j] - x0[i * L + jp] + x1[ip * L + j], sn, cs);
}

// The three sums of one chain over the sites tid, tid + nthr, ...: c = sum cos P and q = sum wrap(P) exactly as k_action_charge forms
// them (wilson.hip chain_action_charge: the same expressions in the same order), d = the cosines of the defect among them
__device__ __forceinline__ void df_chain_sums(const double* __restrict__ x0, int L, const DefectLine& df, int tid, int nthr, double& csum,
                                              double& dsum, double& qsum) {
    const int n = L * L;
    const double* x1 = x0 + n;
    double c = 0.0, d = 0.0, q = 0.0;
    for (int s = tid; s < n; s += nthr) {
        const int i = s / L, j = s - i * L;
        const int ip = i + 1 == L ? 0 : i + 1, jp = j + 1 == L ? 0 : j + 1;
        const double a = x0[s], bb = x1[s], cc = x0[i * L + jp], dd = x1[ip * L + j];
        const double cs = cos(a + dd - cc - bb);     // summation order of BatchAction._u1_plaq
        c += cs;
        d += df_on(df, L, i, j) ? cs : 0.0;
        q += ft_wrap(a - bb - cc + dd);              // summation order of batch_plaqs
    }
    csum = c; dsum = d; qsum = q;
}

// ---------------------------------------------------------------- the sequenced path's kernels
// S[b] = (-beta) C (k_action_charge's S: the product rounded on its own), sums[0 .. 2][b] = (C, Dsum, Q); one workgroup of
// chain_threads(L) per chain.  S may be null.
__global__ void k_defect_sums(const double* __restrict__ x, int L, int B, double beta, DefectLine df, double* __restrict__ S,
                              double* __restrict__ sums) {
    __shared__ double red[16];
    const int b = blockIdx.x;
    double c, d, q;
    df_chain_sums(x + (size_t)b * 2 * L * L, L, df, (int)threadIdx.x, (int)blockDim.x, c, d, q);
    c = ft_block_sum(c, red);
    d = ft_block_sum(d, red);
    q = ft_block_sum(q, red);
    if (threadIdx.x == 0) {
        if (S) S[b] = (-beta) * c;
        sums[b] = c; sums[(size_t)B + b] = d; sums[2 * (size_t)B + b] = df_charge(q);
    }
}

// gP[b][L][L] = w sin P, w = g_b[b] on the defect and beta elsewhere; grid-stride over a chain's sites (the chain on grid y)
__global__ __launch_bounds__(256) void k_defect_gp(const double* __restrict__ x, int L, double beta, const double* __restrict__ g_b,
                                                   DefectLine df, double* __restrict__ gp) {
    const int b = blockIdx.y, n = L * L;
    const double* x0 = x + (size_t)b * 2 * n;
    const double g = g_b[b];
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
        const int i = s / L, j = s - i * L;
        double sn, cs;
        df_sincos_site(x0, x0 + n, L, i, j, &sn, &cs);
        gp[(size_t)b * n + s] = (df_on(df, L, i, j) ? g : beta) * sn;
    }
}

// a thread per chain: H[b] += (beta - g_b[b]) Dsum[b]
__global__ void k_defect_energy(const double* __restrict__ sums, int B, double beta, const double* __restrict__ g_b, double* __restrict__ H) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    H[b] = H[b] + (beta - g_b[b]) * sums[(size_t)B + b];
}

// ---------------------------------------------------------------- the pieces on their own: force and action of one field
// F = dS_d / dx: the stencil's two differences of gP, every gP recomputed where it is needed (three sincos per site: a test and
// measurement kernel, not the MD's).  Grid-stride over a chain's sites, the chain on grid y.
__global__ __launch_bounds__(256) void k_defect_force(const double* __restrict__ x, int L, double beta, const double* __restrict__ g_b,
                                                      DefectLine df, double* __restrict__ F) {
    const int b = blockIdx.y, n = L * L;
    const double* x0 = x + (size_t)b * 2 * n;
    const double* x1 = x0 + n;
    const double g = g_b[b];
    double* Fb = F + (size_t)b * 2 * n;
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
        const int i = s / L, j = s - i * L;
        const int im = i == 0 ? L - 1 : i - 1, jm = j == 0 ? L - 1 : j - 1;
        double sn, cs;
        df_sincos_site(x0, x1, L, i, j, &sn, &cs);
        const double gc = (df_on(df, L, i, j) ? g : beta) * sn;
        df_sincos_site(x0, x1, L, i, jm, &sn, &cs);
        const double gl = (df_on(df, L, i, jm) ? g : beta) * sn;
        df_sincos_site(x0, x1, L, im, j, &sn, &cs);
        const double gu = (df_on(df, L, im, j) ? g : beta) * sn;
        Fb[s] = gc - gl;
        Fb[n + s] = gu - gc;
    }
}

// S[b] = (-beta) C + (beta - g_b) Dsum, csum[b] = C, dsum[b] = Dsum, Q[b] = the integer charge; each output optional
__global__ void k_defect_action(const double* __restrict__ x, int L, double beta, const double* __restrict__ g_b, DefectLine df,
                                double* __restrict__ S, double* __restrict__ csum, double* __restrict__ dsum, double* __restrict__ Q) {
    __shared__ double red[16];
    const int b = blockIdx.x;
    double c, d, q;
    df_chain_sums(x + (size_t)b * 2 * L * L, L, df, (int)threadIdx.x, (int)blockDim.x, c, d, q);
    c = ft_block_sum(c, red);
    d = ft_block_sum(d, red);
    q = ft_block_sum(q, red);
    if (threadIdx.x == 0) {
        if (S) S[b] = (-beta) * c + (beta - g_b[b]) * d;
        if (csum) csum[b] = c;
        if (dsum) dsum[b] = d;
        if (Q) Q[b] = df_charge(q);
    }
}

// x_out[b][mu][(i + s0) mod L][(j + s1) mod L] = x[b][mu][i][j] for the chains on rung `top`, a plain copy for every other chain.  A
// thread walks OUTPUT sites (coalesced stores; the loads are rows cut once).  shift[b] = (s0, s1), any integers.
__global__ __launch_bounds__(256) void k_defect_translate(const double* __restrict__ x, int L, const int32_t* __restrict__ rung, int top,
                                                          const int32_t* __restrict__ shift, double* __restrict__ x_out) {
    const int b = blockIdx.y, n = L * L;
    int s0 = 0, s1 = 0;
    if (rung[b] == top) {
        s0 = shift[2 * (size_t)b] % L; s1 = shift[2 * (size_t)b + 1] % L;
        s0 = s0 < 0 ? s0 + L : s0; s1 = s1 < 0 ? s1 + L : s1;
    }
    const double* xb = x + (size_t)b * 2 * n;
    double* ob = x_out + (size_t)b * 2 * n;
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
        const int i = s / L, j = s - i * L;
        int fi = i - s0, fj = j - s1;                    // the site that lands on (i, j)
        fi = fi < 0 ? fi + L : fi; fj = fj < 0 ? fj + L : fj;
        const int f = fi * L + fj;
        ob[s] = xb[f]; ob[n + s] = xb[n + f];
    }
}

// ---------------------------------------------------------------- whole trajectory with a defect, one launch (L <= 64)
// k_hmc_trajectory_sched<true>'s thread-to-site map, LDS plan (links 64 KB, w sin P 32 KB, one reduction row) and stage loop; per owned
// site one weight, decided once at load.  Each energy takes the parent's two block sums (cos P, v^2) in the parent's order and two
// more, Dsum and the charge: H = ((-beta) C + K / 2) + (beta - g) Dsum, the bracket as the parent forms it.
__global__ __launch_bounds__(TJ_NT) void k_defect_trajectory(const double* __restrict__ x, const double* __restrict__ v,
                                                             const double* __restrict__ u, int L, double beta, const double* __restrict__ g_b,
                                                             DefectLine df, fthmc::Sched sched, double* __restrict__ x_new,
                                                             double* __restrict__ dH, double* __restrict__ acc, double* __restrict__ H0o,
                                                             double* __restrict__ H1o, double* __restrict__ csum_out,
                                                             double* __restrict__ dsum_out, double* __restrict__ q_out) {
    __shared__ double sx[2 * TJ_MAXL * TJ_MAXL];        // links
    __shared__ double sp[TJ_MAXL * TJ_MAXL];            // w sin P
    __shared__ double red[16];
    const int b = blockIdx.x, tid = threadIdx.x, n = L * L;
    const double g = g_b[b];
    const double* xb = x + (size_t)b * 2 * n;
    const double* vb = v + (size_t)b * 2 * n;
    double v0[TJ_NSITE], v1[TJ_NSITE], k0[TJ_NSITE], k1[TJ_NSITE], wt[TJ_NSITE];
    int st[TJ_NSITE], sjm[TJ_NSITE], sim[TJ_NSITE], sjp[TJ_NSITE], sip[TJ_NSITE];
    bool on[TJ_NSITE];
    double kin = 0.0;
#pragma unroll
    for (int k = 0; k < TJ_NSITE; ++k) {
        const int s = tid + k * TJ_NT;
        st[k] = s < n ? s : -1;
        v0[k] = v1[k] = k0[k] = k1[k] = 0.0; sjm[k] = sim[k] = sjp[k] = sip[k] = 0;
        wt[k] = beta; on[k] = false;
        if (s < n) {
            const int i = s / L, j = s - i * L;
            sjp[k] = i * L + (j + 1 == L ? 0 : j + 1);  sip[k] = (i + 1 == L ? 0 : i + 1) * L + j;
            sjm[k] = i * L + (j == 0 ? L - 1 : j - 1);  sim[k] = (i == 0 ? L - 1 : i - 1) * L + j;
            on[k] = df_on(df, L, i, j);
            wt[k] = on[k] ? g : beta;
            sx[s] = xb[s]; sx[n + s] = xb[n + s];
            v0[k] = vb[s]; v1[k] = vb[n + s];
            kin += v0[k] * v0[k] + v1[k] * v1[k];
        }
    }
    __syncthreads();
    // H of the links in sx and the momenta behind ksum; C, Dsum and the charge of the same links beside it
    auto energy = [&](double ksum, double* C, double* D, double* Q) {
        double c = 0.0, d = 0.0, q = 0.0;
#pragma unroll
        for (int k = 0; k < TJ_NSITE; ++k)
            if (st[k] >= 0) {
                double sn_, cs_;
                ft_sincos(tj_plaq_energy(sx, n, st[k], sjp[k], sip[k]), &sn_, &cs_);
                c += cs_;
                d += on[k] ? cs_ : 0.0;
                q += ft_wrap(tj_plaq_force(sx, n, st[k], sjp[k], sip[k]));
            }
        c = ft_block_sum(c, red);
        // the parent's H = -beta C + K / 2 as its pinned code rounds it: K / 2 exact, then ONE fused multiply-add (stated, not left to
        // the contraction pass: it follows the code around it, meta.hip mt_block_sums)
        const double hp = fma(-beta, c, 0.5 * ft_block_sum(ksum, red));
        d = ft_block_sum(d, red);
        q = ft_block_sum(q, red);
        *C = c; *D = d; *Q = df_charge(q);
        return hp + (beta - g) * d;
    };
    double c0, d0, q0, c1, d1, q1;
    const double h0 = energy(kin, &c0, &d0, &q0);
#pragma unroll
    for (int k = 0; k < TJ_NSITE; ++k)
        if (st[k] >= 0) { sx[st[k]] += sched.b0 * v0[k]; sx[n + st[k]] += sched.b0 * v1[k]; }
    bool shifted = false;                                // sx holds the shifted links of the own sites, k0 / k1 the links themselves
    for (int it = 0; it < sched.n; ++it) {
        const fthmc::SchedStage sg = sched.stage(it);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < TJ_NSITE; ++k)
            if (st[k] >= 0) {
                double sn_, cs_;
                ft_sincos(tj_plaq_force(sx, n, st[k], sjp[k], sip[k]), &sn_, &cs_);
                sp[st[k]] = wt[k] * sn_;
            }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < TJ_NSITE; ++k)
            if (st[k] >= 0) {
                const double sc = sp[st[k]];
                tj_stage(sg, shifted, sc - sp[sjm[k]], sp[sim[k]] - sc, sx, n, st[k], v0[k], v1[k], k0[k], k1[k]);
            }
        shifted = sg.kind == fthmc::FT_STAGE_SHIFT;
    }
    kin = 0.0;
#pragma unroll
    for (int k = 0; k < TJ_NSITE; ++k)
        if (st[k] >= 0) {
            sx[st[k]] = ft_regularize(sx[st[k]]); sx[n + st[k]] = ft_regularize(sx[n + st[k]]);
            kin += v0[k] * v0[k] + v1[k] * v1[k];
        }
    __syncthreads();
    const double h1 = energy(kin, &c1, &d1, &q1);
    const double d = h1 - h0;
    const bool ok = u[b] < exp(-d);
    if (tid == 0) {
        if (dH) dH[b] = d;
        if (acc) acc[b] = ok ? 1.0 : 0.0;
        if (H0o) H0o[b] = h0;
        if (H1o) H1o[b] = h1;
        if (csum_out) csum_out[b] = ok ? c1 : c0;
        if (dsum_out) dsum_out[b] = ok ? d1 : d0;
        if (q_out) q_out[b] = ok ? q1 : q0;
    }
    double* xo = x_new + (size_t)b * 2 * n;
#pragma unroll
    for (int k = 0; k < TJ_NSITE; ++k)
        if (st[k] >= 0) {
            xo[st[k]] = ok ? sx[st[k]] : xb[st[k]];
            xo[n + st[k]] = ok ? sx[n + st[k]] : xb[n + st[k]];
        }
}

// grid-stride over a chain's sites, 256 threads a workgroup, at most 64 workgroups per chain (the chain on grid y: B <= 65535)
inline dim3 df_stride_grid(int B, int L) { const int gx = (L * L + 255) / 256; return dim3(gx > 64 ? 64 : gx, B); }

}  // namespace

namespace fthmc {

int launch_defect_trajectory(const double* x, const double* v, const double* u, int B, int L, double beta, const double* g_b,
                             const DefectLine& df, const Sched& sched, double* x_new, double* dH, double* acc, double* H0, double* H1,
                             double* csum_out, double* dsum_out, double* q_out, hipStream_t s) {
    if (L > TJ_MAXL) return FTHMC_ERR_UNSUPPORTED;
    if (sched.n < 1 || sched.nper < 1 || sched.nper > 3) return FTHMC_ERR_ARG;
    hipLaunchKernelGGL(k_defect_trajectory, dim3(B), dim3(TJ_NT), 0, s, x, v, u, L, beta, g_b, df, sched, x_new, dH, acc, H0, H1, csum_out,
                       dsum_out, q_out);
    FT_LAUNCH_CHECK(); return FTHMC_OK;
}
int launch_defect_sums(const double* x, int B, int L, double beta, const DefectLine& df, double* S, double* sums, hipStream_t s) {
    hipLaunchKernelGGL(k_defect_sums, dim3(B), dim3(chain_threads(L)), 0, s, x, L, B, beta, df, S, sums);
    FT_LAUNCH_CHECK(); return FTHMC_OK;
}
int launch_defect_gp(const double* x, int B, int L, double beta, const double* g_b, const DefectLine& df, double* gp, hipStream_t s) {
    hipLaunchKernelGGL(k_defect_gp, df_stride_grid(B, L), dim3(256), 0, s, x, L, beta, g_b, df, gp);
    FT_LAUNCH_CHECK(); return FTHMC_OK;
}
int launch_defect_energy(const double* sums, int B, double beta, const double* g_b, double* H, hipStream_t s) {
    hipLaunchKernelGGL(k_defect_energy, dim3((B + 255) / 256), dim3(256), 0, s, sums, B, beta, g_b, H);
    FT_LAUNCH_CHECK(); return FTHMC_OK;
}
// the force and the translation walk the chains of grid y in slices of 65535: they take B up to FTHMC_MAX_B
int launch_defect_force(const double* x, int B, int L, double beta, const double* g_b, const DefectLine& df, double* F, hipStream_t s) {
    const size_t n2 = (size_t)2 * L * L;
    for (int b0 = 0; b0 < B; b0 += 65535) {
        const int nb = B - b0 < 65535 ? B - b0 : 65535;
        hipLaunchKernelGGL(k_defect_force, df_stride_grid(nb, L), dim3(256), 0, s, x + b0 * n2, L, beta, g_b + b0, df, F + b0 * n2);
        FT_LAUNCH_CHECK();
    }
    return FTHMC_OK;
}
int launch_defect_action(const double* x, int B, int L, double beta, const double* g_b, const DefectLine& df, double* S, double* csum,
                         double* dsum, double* Q, hipStream_t s) {
    hipLaunchKernelGGL(k_defect_action, dim3(B), dim3(chain_threads(L)), 0, s, x, L, beta, g_b, df, S, csum, dsum, Q);
    FT_LAUNCH_CHECK(); return FTHMC_OK;
}
int launch_defect_translate(const double* x, int B, int L, const int32_t* rung, int top, const int32_t* shift, double* x_out, hipStream_t s) {
    const size_t n2 = (size_t)2 * L * L;
    for (int b0 = 0; b0 < B; b0 += 65535) {
        const int nb = B - b0 < 65535 ? B - b0 : 65535;
        hipLaunchKernelGGL(k_defect_translate, df_stride_grid(nb, L), dim3(256), 0, s, x + b0 * n2, L, rung + b0, top, shift + 2 * (size_t)b0,
                           x_out + b0 * n2);
        FT_LAUNCH_CHECK();
    }
    return FTHMC_OK;
}

}  // namespace fthmc
