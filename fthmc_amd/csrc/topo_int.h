// The integer reductions of the instanton hit (topo.hip): every angle the update forms is 2 pi (or pi) times a fraction
// whose numerator is reduced FIRST, in 64-bit integers, so that the angle stays in [0, 2 pi) whatever the charge k.  Plain C++
// (host and device): tests/hip/instanton_walk.cpp walks these functions under UBSan for the largest k and L.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FT_TOPO_HD __host__ __device__ __forceinline__
#else
#define FT_TOPO_HD inline
#endif

namespace fthmc {

constexpr int IT_MAX_HITS = 1024;             // hits of one call at most: |k| <= IT_MAX_HITS

// the mathematical remainder: 0 <= it_mod(a, m) < m for m > 0
FT_TOPO_HD int64_t it_mod(int64_t a, int64_t m) {
    const int64_t r = a % m;
    return r < 0 ? r + m : r;
}
// x1[i][j] += 2 pi it_shift_num_x1(k, i, L) / L^2
FT_TOPO_HD int64_t it_shift_num_x1(int k, int i, int L) { return it_mod((int64_t)k * (int64_t)i, (int64_t)L * (int64_t)L); }
// x0[L-1][j] -= 2 pi it_shift_num_seam(k, j, L) / L
FT_TOPO_HD int64_t it_shift_num_seam(int k, int j, int L) { return it_mod((int64_t)k * (int64_t)j, (int64_t)L); }
// theta of the step k -> k + s: pi it_theta_num(k, s, L) / L^2
FT_TOPO_HD int64_t it_theta_num(int k, int s, int L) { return it_mod(2 * (int64_t)k + (int64_t)s, 2 * (int64_t)L * (int64_t)L); }

}  // namespace fthmc
