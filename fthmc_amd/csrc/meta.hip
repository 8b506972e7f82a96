// Metadynamics HMC of 2D U(1) (fthmc_meta_*): plain HMC under a bias potential V(Q_m) in the continuous charge
//   Q_m(x) = (1 / 2 pi) sum sin P,      S_b = -beta sum cos P + V(Q_m),      H = S_b + sum v^2 / 2.
// Action and Q_m are both functions of the plaquettes, so the biased force is the plain stencil applied to
//   gP(site) = beta sin P + c_b cos P,      c_b = V'(Q_m(chain b)) / 2 pi:
// the sincos the plain kernels evaluate anyway, one chain-wide sum and one FMA per site; no new pass over memory.
// V is a table V[G][nb] on the nodes q_i = -qmax + i delta, delta = 2 qmax / (nb - 1), piecewise linear between them and a
// quadratic wall outside; chain b reads row b / (B / G).  With an all-zero table (and no wall in reach) every kernel here does
// the arithmetic of its plain twin in wilson.hip: beta sn + 0 cs, h + 0.
// Two trajectory shapes: k_meta_trajectory (L <= 64: one launch, one workgroup per chain, links in LDS, momenta in registers --
// the resident plan of traj_resident.h with a sin P and a cos P plane) and the sequenced one for any L (api.hip: k_meta_sums, k_meta_gp and the plain kick / shift /
// energy / Metropolis kernels).  k_meta_deposit adds the walkers' hills to the table in chain order, without atomics.
#include "common.h"
#include "kernels.h"
#include "meta_tab.h"
#include "traj_resident.h"

namespace {

// (the table's lookup mt_locate / mt_lookup / mt_bias_row / mt_bias: meta_tab.h, shared with flow_small.hip)

// sin and cos of the plaquette at site (i, j), the force kernels' order of the four links
__device__ __forceinline__ void mt_sincos_site(const double* __restrict__ x0, const double* __restrict__ x1, int L, int i, int j,
                                               double* sn, double* cs) {
    const int ip = i + 1 == L ? 0 : i + 1, jp = j + 1 == L ? 0 : j + 1;
    ft_sincos(x0[i * L + j] - x1[i * L + j] - x0[i * L + jp] + x1[ip * L + j], sn, cs);
}

// the sums of sin P and cos P over the sites tid, tid + nthr, ... of one chain
__device__ __forceinline__ void mt_chain_sums(const double* __restrict__ x0, int L, int tid, int nthr, double& ssum, double& csum) {
    const int n = L * L;
    const double* x1 = x0 + n;
    double q = 0.0, c = 0.0;
    for (int s = tid; s < n; s += nthr) {
        const int i = s / L, j = s - i * L;
        double sn, cs;
        mt_sincos_site(x0, x1, L, i, j, &sn, &cs);
        q += sn; c += cs;
    }
    ssum = q; csum = c;
}

// ---------------------------------------------------------------- the sequenced path's two kernels and the energy lookup
// sums[b][2] = (sum sin P, sum cos P); one workgroup of chain_threads(L) per chain
__global__ void k_meta_sums(const double* __restrict__ x, int L, double* __restrict__ sums) {
    __shared__ double red[16];
    const int b = blockIdx.x;
    double q, c;
    mt_chain_sums(x + (size_t)b * 2 * L * L, L, (int)threadIdx.x, (int)blockDim.x, q, c);
    q = ft_block_sum(q, red);
    c = ft_block_sum(c, red);
    if (threadIdx.x == 0) { sums[2 * (size_t)b] = q; sums[2 * (size_t)b + 1] = c; }
}

// gP[b][L][L] = beta sin P + c_b cos P, c_b from the chain's sin sum; grid-stride over a chain's sites (the chain on grid y)
__global__ __launch_bounds__(256) void k_meta_gp(const double* __restrict__ x, int L, double beta, const double* __restrict__ sums,
                                                 MetaTab T, double* __restrict__ gp) {
    const int b = blockIdx.y, n = L * L;
    const double* x0 = x + (size_t)b * 2 * n;
    double qm, V, c;
    mt_bias(T, b, sums[2 * (size_t)b], &qm, &V, &c);
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
        const int i = s / L, j = s - i * L;
        double sn, cs;
        mt_sincos_site(x0, x0 + n, L, i, j, &sn, &cs);
        gp[(size_t)b * n + s] = beta * sn + c * cs;
    }
}

// a thread per chain: H[b] += V(Q_m) (H null: no energy), qv[0][b] = Q_m, qv[1][b] = V
__global__ void k_meta_energy(const double* __restrict__ sums, int B, MetaTab T, double* __restrict__ H, double* __restrict__ qv) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double qm, V, c;
    mt_bias(T, b, sums[2 * (size_t)b], &qm, &V, &c);
    if (H) H[b] = H[b] + V;
    if (qv) { qv[b] = qm; qv[(size_t)B + b] = V; }
}

// the same from a carried Q_m (the flowed trajectory's table-free state): H[b] += V(qm[b]), vb[b] = V(qm[b]); each optional
__global__ void k_meta_energy_qm(const double* __restrict__ qm, int B, MetaTab T, double* __restrict__ H, double* __restrict__ vb) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double q = qm[b];
    double V, c;
    mt_lookup(mt_row(T, b), T.nb, T.qmax, T.wall, q, &V, &c);
    if (H) H[b] = H[b] + V;
    if (vb) vb[b] = V;
}

// ---------------------------------------------------------------- the bias on its own: force and action of one field
// F = dS_b / dx: the stencil's two differences of gP, every gP recomputed where it is needed (three sincos per site: a test and
// measurement kernel, not the MD's).  One workgroup of chain_threads(L) per chain: the sums are k_meta_sums'.
__global__ void k_meta_force(const double* __restrict__ x, int L, double beta, MetaTab T, double* __restrict__ F) {
    __shared__ double red[16];
    const int b = blockIdx.x, n = L * L;
    const double* x0 = x + (size_t)b * 2 * n;
    const double* x1 = x0 + n;
    double q, cc;
    mt_chain_sums(x0, L, (int)threadIdx.x, (int)blockDim.x, q, cc);
    q = ft_block_sum(q, red);
    double qm, V, c;
    mt_bias(T, b, q, &qm, &V, &c);
    double* Fb = F + (size_t)b * 2 * n;
    for (int s = threadIdx.x; s < n; s += blockDim.x) {
        const int i = s / L, j = s - i * L;
        const int im = i == 0 ? L - 1 : i - 1, jm = j == 0 ? L - 1 : j - 1;
        double sn, cs;
        mt_sincos_site(x0, x1, L, i, j, &sn, &cs);
        const double g = beta * sn + c * cs;
        mt_sincos_site(x0, x1, L, i, jm, &sn, &cs);
        const double gl = beta * sn + c * cs;
        mt_sincos_site(x0, x1, L, im, j, &sn, &cs);
        const double gu = beta * sn + c * cs;
        Fb[s] = g - gl;
        Fb[n + s] = gu - g;
    }
}

// S[b] = -beta sum cos P + V(Q_m), qm[b] = Q_m, vb[b] = V(Q_m); each output optional
__global__ void k_meta_action(const double* __restrict__ x, int L, double beta, MetaTab T, double* __restrict__ S, double* __restrict__ qmo,
                              double* __restrict__ vbo) {
    __shared__ double red[16];
    const int b = blockIdx.x;
    double q, c;
    mt_chain_sums(x + (size_t)b * 2 * L * L, L, (int)threadIdx.x, (int)blockDim.x, q, c);
    q = ft_block_sum(q, red);
    c = ft_block_sum(c, red);
    if (threadIdx.x == 0) {
        double qm, V, cb;
        mt_bias(T, b, q, &qm, &V, &cb);
        if (S) S[b] = (-beta) * c + V;
        if (qmo) qmo[b] = qm;
        if (vbo) vbo[b] = V;
    }
}

// ---------------------------------------------------------------- deposit
// One hill per walker at its Q_m: inside the table node i gains w (1 - f) and node i + 1 gains w f, outside nothing.  A thread per
// node walks its row's chains IN ORDER and adds what falls on its node: no atomics, the sum of a node is that of the chains in
// order whatever the launch shape.  In place: a node is read and written by its own thread only.  The workgroup locates 256 chains
// at a time together (the two divisions of a lookup and the two hills, once per chain and workgroup) and leaves them in LDS; the walk
// itself is three LDS reads, an add and two selects per chain.
__global__ __launch_bounds__(256) void k_meta_deposit(const double* __restrict__ qm, int cpr, int nb, double qmax, double w,
                                                      double* __restrict__ vtab) {
#pragma clang fp contract(off)
    __shared__ int si[256];
    __shared__ double slo[256], shi[256];
    const int node = blockIdx.y * blockDim.x + threadIdx.x, g = blockIdx.x;            // the row on grid x: G may be B
    const bool mine = node < nb;
    double acc = mine ? vtab[(size_t)g * nb + node] : 0.0;
    const double* q = qm + (size_t)g * cpr;
    for (int k0 = 0; k0 < cpr; k0 += 256) {
        const int k = k0 + (int)threadIdx.x, m = cpr - k0 < 256 ? cpr - k0 : 256;
        __syncthreads();                                                                // the walk over the chunk before is over
        if (k < cpr) {
            int i = -2; double f = 0.0, delta;
            if (!mt_locate(q[k], nb, qmax, &i, &f, &delta)) i = -2;                     // outside: meets no node
            si[threadIdx.x] = i; slo[threadIdx.x] = w * (1.0 - f); shi[threadIdx.x] = w * f;
        }
        __syncthreads();
        for (int j = 0; j < m; ++j) {                                                   // no branch: the sum moves on where the chain meets the node
            const int i = si[j];
            const double t = acc + (i == node ? slo[j] : shi[j]);
            acc = (i == node || i + 1 == node) ? t : acc;
        }
    }
    if (mine) vtab[(size_t)g * nb + node] = acc;
}

// ---------------------------------------------------------------- whole biased trajectory, one launch (L <= 64)
// ft_block_sum's sums of N values at once behind ONE barrier: wave sums, lane 0 of every wave leaves them in red[n][wave], every thread
// adds them as ft_block_sum does (0.0 + wave 0 + wave 1 + ...): without DPP each result is bit for bit ft_block_sum's.  The CALLER has a barrier
// between the reads of the call before and this call's writes (ft_block_sum brings its own: one more barrier per sum).
// A wave's sum without the LDS crossbar, for a sum nobody has to reproduce bit for bit (Q_m of a stage): four DPP levels inside the
// rows of 16 lanes (quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror: every lane then holds its row's sum), the four row
// sums through v_readlane and three scalar-operand additions.  ft_wave_sum's six __shfl_xor levels are twelve ds_bpermute_b32 on the
// critical path of every stage (measured at 32 x L = 16 with them: the block sum 0.77 us of a 2.5 us stage).  Needs a full EXEC mask.
template <int CTRL> __device__ __forceinline__ double mt_dpp(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double mt_row_of(double v, int lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}
__device__ __forceinline__ double mt_wave_sum_dpp(double v) {
    v += mt_dpp<0xB1>(v);
    v += mt_dpp<0x4E>(v);
    v += mt_dpp<0x141>(v);
    v += mt_dpp<0x140>(v);
    return ((mt_row_of(v, 0) + mt_row_of(v, 16)) + mt_row_of(v, 32)) + mt_row_of(v, 48);
}

template <bool DPP, int N> __device__ __forceinline__ void mt_block_sums(double (&v)[N], double (*red)[16]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // the stage's sum knows the kernel's workgroup, so that its reads below are issued together; the energies' keep ft_block_sum's loop
    // as it is (with their loop unrolled the compiler contracted H = -beta C + K / 2 another way than it does in the parent's kernels:
    // the last bit of H moved in three zero-table cases, two at L = 20 and one at L = 64)
    const int nw = DPP ? TJ_NT / FT_WAVE : (int)((blockDim.x + 63) >> 6);
#pragma unroll
    for (int k = 0; k < N; ++k) {
        v[k] = DPP ? mt_wave_sum_dpp(v[k]) : ft_wave_sum(v[k]);
        if (lane == 0) red[k][wave] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double t = 0.0;
        if (DPP) {
#pragma unroll 8                                         // (all 16 at once: 128 VGPRs and 12 B of scratch per lane)
            for (int i = 0; i < TJ_NT / FT_WAVE; ++i) t += red[k][i];
        } else {
            for (int i = 0; i < nw; ++i) t += red[k][i];
        }
        v[k] = t;
    }
}

// k_hmc_trajectory_sched's thread-to-site map and its LDS plan with one plane more (the resident plan: traj_resident.h, with the two
// orders of the plaquette and the stage body): links 64 KB, sin P 32 KB, cos P 32 KB of the CU's 160 KB.  Per stage, behind the barrier that closes the stage before: one ft_sincos per site into the two planes and the
// wave sums of sin P; ONE barrier; every thread adds the wave sums (Q_m), looks the wave-uniform slope up and forms
// gP = beta sn + c cs of its site and of the two neighbours the stencil needs from the planes (two FMAs more than one plane of gP
// would cost, and two barriers less), then the plain KICK / SHIFT: two barrier phases a stage, as the parent has.  h0 / h1 add
// V(Q_m) of the start and of the regularized end field; their three sums (cos P, sin P, v^2) share one barrier.
__global__ __launch_bounds__(TJ_NT) void k_meta_trajectory(const double* __restrict__ x, const double* __restrict__ v,
                                                           const double* __restrict__ u, int L, double beta, fthmc::Sched sched, MetaTab T,
                                                           double* __restrict__ x_new, double* __restrict__ dH, double* __restrict__ acc,
                                                           double* __restrict__ H0o, double* __restrict__ H1o, double* __restrict__ qm_out,
                                                           double* __restrict__ vb_out) {
    __shared__ double sx[2 * TJ_MAXL * TJ_MAXL];        // links
    __shared__ double ssn[TJ_MAXL * TJ_MAXL];           // sin P
    __shared__ double scs[TJ_MAXL * TJ_MAXL];           // cos P
    __shared__ double red[3][16];
    const int b = blockIdx.x, tid = threadIdx.x, n = L * L;
    const double* xb = x + (size_t)b * 2 * n;
    const double* vb = v + (size_t)b * 2 * n;
    const double* row = mt_row(T, b);                    // (a copy of the row in LDS was measured: no gain at nb = 81, the row stays cached)
    double v0[TJ_NSITE], v1[TJ_NSITE], k0[TJ_NSITE], k1[TJ_NSITE];
    int st[TJ_NSITE], sjm[TJ_NSITE], sim[TJ_NSITE], sjp[TJ_NSITE], sip[TJ_NSITE];
    double kin = 0.0;
#pragma unroll
    for (int k = 0; k < TJ_NSITE; ++k) {
        const int s = tid + k * TJ_NT;
        st[k] = s < n ? s : -1;
        v0[k] = v1[k] = k0[k] = k1[k] = 0.0; sjm[k] = sim[k] = sjp[k] = sip[k] = 0;
        if (s < n) {
            const int i = s / L, j = s - i * L;
            sjp[k] = i * L + (j + 1 == L ? 0 : j + 1);  sip[k] = (i + 1 == L ? 0 : i + 1) * L + j;
            sjm[k] = i * L + (j == 0 ? L - 1 : j - 1);  sim[k] = (i == 0 ? L - 1 : i - 1) * L + j;
            sx[s] = xb[s]; sx[n + s] = xb[n + s];
            v0[k] = vb[s]; v1[k] = vb[n + s];
            kin += v0[k] * v0[k] + v1[k] * v1[k];
        }
    }
    __syncthreads();
    // H = -beta sum cos P + K / 2 (the parent's sums in the parent's order: summation order of BatchAction) + V(Q_m) of the links in LDS;
    // behind a barrier, like every call of mt_block_sums here
    auto energy = [&](double ksum, double* qm, double* V) {
        double s3[3] = {0.0, 0.0, ksum};
#pragma unroll
        for (int k = 0; k < TJ_NSITE; ++k)
            if (st[k] >= 0) {
                double sn_, cs_;
                ft_sincos(tj_plaq_energy(sx, n, st[k], sjp[k], sip[k]), &sn_, &cs_);
                s3[0] += cs_; s3[1] += sn_;
            }
        mt_block_sums<false>(s3, red);
        const double hp = (-beta) * s3[0] + 0.5 * s3[2];
        double c;
        mt_bias_row(row, T, s3[1], qm, V, &c);
        return hp + *V;
    };
    double qm0, vb0, qm1, vb1;
    const double h0 = energy(kin, &qm0, &vb0);
#pragma unroll
    for (int k = 0; k < TJ_NSITE; ++k)
        if (st[k] >= 0) { sx[st[k]] += sched.b0 * v0[k]; sx[n + st[k]] += sched.b0 * v1[k]; }
    bool shifted = false;                                // sx holds the shifted links of the own sites, k0 / k1 the links themselves
    for (int it = 0; it < sched.n; ++it) {
        const fthmc::SchedStage sg = sched.stage(it);
        __syncthreads();
        double q1[1] = {0.0};
#pragma unroll
        for (int k = 0; k < TJ_NSITE; ++k)
            if (st[k] >= 0) {
                double sn_, cs_;
                ft_sincos(tj_plaq_force(sx, n, st[k], sjp[k], sip[k]), &sn_, &cs_);
                ssn[st[k]] = sn_; scs[st[k]] = cs_;
                q1[0] += sn_;
            }
        mt_block_sums<true>(q1, red);                       // its barrier also publishes the two planes
        double qm, V, c;
        mt_bias_row(row, T, q1[0], &qm, &V, &c);
#pragma unroll
        for (int k = 0; k < TJ_NSITE; ++k)
            if (st[k] >= 0) {
                const double sc = beta * ssn[st[k]] + c * scs[st[k]];
                const double f0 = sc - (beta * ssn[sjm[k]] + c * scs[sjm[k]]), f1 = (beta * ssn[sim[k]] + c * scs[sim[k]]) - sc;
                tj_stage(sg, shifted, f0, f1, sx, n, st[k], v0[k], v1[k], k0[k], k1[k]);
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
    const double h1 = energy(kin, &qm1, &vb1);
    const double d = h1 - h0;
    const bool ok = u[b] < exp(-d);
    if (tid == 0) {
        if (dH) dH[b] = d;
        if (acc) acc[b] = ok ? 1.0 : 0.0;
        if (H0o) H0o[b] = h0;
        if (H1o) H1o[b] = h1;
        if (qm_out) qm_out[b] = ok ? qm1 : qm0;
        if (vb_out) vb_out[b] = ok ? vb1 : vb0;
    }
    double* xo = x_new + (size_t)b * 2 * n;
#pragma unroll
    for (int k = 0; k < TJ_NSITE; ++k)
        if (st[k] >= 0) {
            xo[st[k]] = ok ? sx[st[k]] : xb[st[k]];
            xo[n + st[k]] = ok ? sx[n + st[k]] : xb[n + st[k]];
        }
}

}  // namespace

namespace fthmc {

int launch_meta_trajectory(const double* x, const double* v, const double* u, int B, int L, double beta, const Sched& sched, const MetaTab& T,
                           double* x_new, double* dH, double* acc, double* H0, double* H1, double* qm_out, double* vb_out, hipStream_t s) {
    if (L > TJ_MAXL) return FTHMC_ERR_UNSUPPORTED;
    if (sched.n < 1 || sched.nper < 1 || sched.nper > 3) return FTHMC_ERR_ARG;
    hipLaunchKernelGGL(k_meta_trajectory, dim3(B), dim3(TJ_NT), 0, s, x, v, u, L, beta, sched, T, x_new, dH, acc, H0, H1, qm_out, vb_out);
    FT_LAUNCH_CHECK(); return FTHMC_OK;
}
int launch_meta_sums(const double* x, int B, int L, double* sums, hipStream_t s) {
    hipLaunchKernelGGL(k_meta_sums, dim3(B), dim3(chain_threads(L)), 0, s, x, L, sums);
    FT_LAUNCH_CHECK(); return FTHMC_OK;
}
int launch_meta_gp(const double* x, int B, int L, double beta, const double* sums, const MetaTab& T, double* gp, hipStream_t s) {
    const int gx = (L * L + 255) / 256;
    hipLaunchKernelGGL(k_meta_gp, dim3(gx > 64 ? 64 : gx, B), dim3(256), 0, s, x, L, beta, sums, T, gp);
    FT_LAUNCH_CHECK(); return FTHMC_OK;
}
int launch_meta_energy(const double* sums, int B, const MetaTab& T, double* H, double* qv, hipStream_t s) {
    hipLaunchKernelGGL(k_meta_energy, dim3((B + 255) / 256), dim3(256), 0, s, sums, B, T, H, qv);
    FT_LAUNCH_CHECK(); return FTHMC_OK;
}
int launch_meta_energy_qm(const double* qm, int B, const MetaTab& T, double* H, double* vb, hipStream_t s) {
    hipLaunchKernelGGL(k_meta_energy_qm, dim3((B + 255) / 256), dim3(256), 0, s, qm, B, T, H, vb);
    FT_LAUNCH_CHECK(); return FTHMC_OK;
}
int launch_meta_force(const double* x, int B, int L, double beta, const MetaTab& T, double* F, hipStream_t s) {
    hipLaunchKernelGGL(k_meta_force, dim3(B), dim3(chain_threads(L)), 0, s, x, L, beta, T, F);
    FT_LAUNCH_CHECK(); return FTHMC_OK;
}
int launch_meta_action(const double* x, int B, int L, double beta, const MetaTab& T, double* S, double* qm, double* vb, hipStream_t s) {
    hipLaunchKernelGGL(k_meta_action, dim3(B), dim3(chain_threads(L)), 0, s, x, L, beta, T, S, qm, vb);
    FT_LAUNCH_CHECK(); return FTHMC_OK;
}
int launch_meta_deposit(const double* qm, int B, int G, int nb, double qmax, double w, double* vtab, hipStream_t s) {
    hipLaunchKernelGGL(k_meta_deposit, dim3(G, (nb + 255) / 256), dim3(256), 0, s, qm, B / G, nb, qmax, w, vtab);
    FT_LAUNCH_CHECK(); return FTHMC_OK;
}

}  // namespace fthmc
