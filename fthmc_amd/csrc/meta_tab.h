// The bias table of the metadynamics samplers as the device reads it: V[G][nb] on the nodes
// q_i = -qmax + i delta, delta = 2 qmax / (nb - 1), piecewise linear between them and a quadratic wall outside; chain b reads row
// b / (B / G).  One definition for meta.hip (plain HMC under the bias) and flow_small.hip (the bias through the flow, one launch).
#pragma once
#include "common.h"
#include "kernels.h"

namespace {

using fthmc::MetaTab;

// (fp contract off in the functions that hold the lookup's and the deposit's arithmetic, as in local.hip / topo.hip: which
// products and sums become one FMA must not be left to the optimiser's view of different kernels)

// t = (q + qmax) / delta -> inside: node i = floor(t) <= nb - 2 with t >= 0, f = t - i
__device__ __forceinline__ bool mt_locate(double q, int nb, double qmax, int* i, double* f, double* delta) {
#pragma clang fp contract(off)
    const double d = (2.0 * qmax) / (double)(nb - 1);
    const double t = (q + qmax) / d;
    const double fl = floor(t);
    *delta = d;
    if (!(t >= 0.0) || !(fl <= (double)(nb - 2))) return false;                     // a NaN q is outside
    *i = (int)fl;
    *f = t - fl;
    return true;
}

// V(q) and c = V'(q) / 2 pi of one table row (inside the table c is ONE quotient, dV / (delta 2 pi): the lookup sits on the critical
// path of every stage of the one-launch trajectory)
__device__ __forceinline__ void mt_lookup(const double* row, int nb, double qmax, double wall, double q, double* V, double* c) {
#pragma clang fp contract(off)
    int i; double f, delta;
    if (mt_locate(q, nb, qmax, &i, &f, &delta)) {
        const double v0 = row[i], dv = row[i + 1] - v0;
        *V = v0 + f * dv;
        *c = dv / (delta * FT_TWO_PI);
    } else {
        const double d = fabs(q) - qmax;
        const double edge = q < 0.0 ? row[0] : row[nb - 1];
        *V = edge + ((0.5 * wall) * d) * d;
        *c = (q < 0.0 ? -(wall * d) : wall * d) / FT_TWO_PI;
    }
}
__device__ __forceinline__ const double* mt_row(const MetaTab& T, int b) { return T.v + (size_t)(b / T.cpr) * T.nb; }

// V and c = V' / 2 pi at the charge of a chain's sin sum, from the chain's row (wherever the caller keeps it)
__device__ __forceinline__ void mt_bias_row(const double* row, const MetaTab& T, double ssum, double* qm, double* V, double* c) {
#pragma clang fp contract(off)
    const double q = ssum / FT_TWO_PI;
    mt_lookup(row, T.nb, T.qmax, T.wall, q, V, c);
    *qm = q;
}
__device__ __forceinline__ void mt_bias(const MetaTab& T, int b, double ssum, double* qm, double* V, double* c) {
    mt_bias_row(mt_row(T, b), T, ssum, qm, V, c);
}

}  // namespace
