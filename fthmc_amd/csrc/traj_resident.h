// The resident plain trajectory's plan, what its kernels share of it: one workgroup of TJ_NT threads per chain, the links in LDS
// (sx[2][n], 64 KB at L = TJ_MAXL), the momenta in registers, every thread the owner of TJ_NSITE sites (tid + k TJ_NT) of its chain
// for the whole launch; between H0 and the Metropolis select nothing touches HBM.  The kernels: wilson.hip k_hmc_trajectory and
// k_hmc_trajectory_sched<PB>, meta.hip k_meta_trajectory.  Each keeps its own planes beside the links and its own MD loop.
// Everything here is inlined into kernels whose code is pinned instruction for instruction (tools/isa_diff.py): what went in is what
// left every one of them the code it was.  Their owned-site map and load, regularize pass and Metropolis epilogue are still written
// out per kernel -- as functions they gave other code (DESIGN, "What wilson.hip states once", has the measurements).
#pragma once
#include "common.h"
#include "kernels.h"

namespace {

constexpr int TJ_NT = 1024, TJ_MAXL = fthmc::HMC_RESIDENT_MAXL, TJ_NSITE = TJ_MAXL * TJ_MAXL / TJ_NT;

// The plaquette of owned site s (jp, ip: its neighbours at j + 1 and i + 1) in its two orders of the four links.  A bit contract
// each, not to be merged: the energies sum in BatchAction's order, the MD in the force kernels'.
__device__ __forceinline__ double tj_plaq_energy(const double* sx, int n, int s, int jp, int ip) {
    return sx[s] + sx[n + ip] - sx[jp] - sx[n + s];
}
__device__ __forceinline__ double tj_plaq_force(const double* sx, int n, int s, int jp, int ip) {
    return sx[s] - sx[n + s] - sx[jp] + sx[n + ip];
}

// -beta sum cos P of the links in sx over the chain (summation order of BatchAction), valid in every thread
__device__ __forceinline__ double tj_action(const int (&st)[TJ_NSITE], const int (&sjp)[TJ_NSITE], const int (&sip)[TJ_NSITE], const double* sx,
                                            int n, double beta, double* red) {
    double c = 0.0;
#pragma unroll
    for (int k = 0; k < TJ_NSITE; ++k)
        if (st[k] >= 0) { double sn_, cs_; ft_sincos(tj_plaq_energy(sx, n, st[k], sjp[k], sip[k]), &sn_, &cs_); c += cs_; }
    return (-beta) * ft_block_sum(c, red);
}

// One stage of a schedule (integrator.h) at owned site s with the force (f0, f1) of the field in sx:
//   KICK(a, b): v -= a F, x += b v  |  SHIFT(c): the thread keeps its own links in k0 / k1 and puts x - c F in their place for the
//   NEXT stage's force, whose kick first puts the kept links back (shifted: the stage before was a SHIFT): sx itself is as if never
//   touched (restored bit for bit, not recomputed)
__device__ __forceinline__ void tj_stage(const fthmc::SchedStage& sg, bool shifted, double f0, double f1, double* sx, int n, int s,
                                         double& v0, double& v1, double& k0, double& k1) {
    if (sg.kind == fthmc::FT_STAGE_SHIFT) {
        k0 = sx[s]; k1 = sx[n + s];
        sx[s] = k0 - sg.a * f0; sx[n + s] = k1 - sg.a * f1;
    } else {
        v0 -= sg.a * f0; v1 -= sg.a * f1;
        const double y0 = shifted ? k0 : sx[s], y1 = shifted ? k1 : sx[n + s];
        sx[s] = y0 + sg.b * v0; sx[n + s] = y1 + sg.b * v1;
    }
}

}  // namespace
