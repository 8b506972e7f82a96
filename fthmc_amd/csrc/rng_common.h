// Device helpers of the random draws (rng.hip): the Philox4x32-10 block function, the 53-bit uniform and the three per-draw
// expressions.  In a header so that tests/hip/device_probe.hip applies exactly these functions to arrays of raw words
// (tests/test_rng_gpu.py), inputs no seed reaches in a test's lifetime included.
#pragma once
#include "common.h"

namespace fthmc_rng {

struct u4 { uint32_t x, y, z, w; };

__device__ __forceinline__ u4 philox4x32_10(u4 c, uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(M0, c.x), lo0 = M0 * c.x;
        const uint32_t hi1 = __umulhi(M1, c.z), lo1 = M1 * c.z;
        c = u4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
        k0 += W0; k1 += W1;
    }
    return c;
}

__device__ __forceinline__ double u53(uint32_t hi, uint32_t lo) {     // (0, 1]
    const uint64_t m = (((uint64_t)hi << 32) | lo) >> 11;
    return ((double)m + 1.0) * (1.0 / 9007199254740992.0);
}

// Box-Muller in fp64: one Philox block -> two N(0,1) values, (cos, sin) of one angle at one radius; u1 in (0, 1]: log is finite.
// The two products are formed where they are asked for: a chain's odd tail asks for the first only
struct normal_pair {
    double rad, sn, cs;
    __device__ __forceinline__ explicit normal_pair(u4 r) {
        const double u1 = u53(r.x, r.y), u2 = u53(r.z, r.w);
        rad = sqrt(-2.0 * log(u1));
        sincos(FT_TWO_PI * u2, &sn, &cs);
    }
    __device__ __forceinline__ double first() const { return rad * cs; }
    __device__ __forceinline__ double second() const { return rad * sn; }
};

// the Metropolis uniform: 1 - (0, 1] = [0, 1), exact in fp64
__device__ __forceinline__ double accept_uniform(uint32_t hi, uint32_t lo) { return 1.0 - u53(hi, lo); }

// one prior value from two words, w = hi - lo as the kernel rounds it: t = 1 - (0, 1] = [0, 1) exactly, then ONE rounding of
// t w + lo.  The result is >= lo; it stays below lo + w unless that rounding reaches it (fthmc_random_uniform, include/fthmc_hip.h)
__device__ __forceinline__ double uniform_value(uint32_t hi, uint32_t lo_word, double lo, double w) {
    return fma(1.0 - u53(hi, lo_word), w, lo);
}

}  // namespace fthmc_rng
