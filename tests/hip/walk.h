// What the stand-alone walkers of the entry points share (meta_walk.cpp, ft_meta_walk.cpp, tempering_walk.cpp, instanton_walk.cpp,
// local_walk.cpp, loops_walk.cpp): the C header, the stand-in device addresses, the counters of calls and of expected refusals,
// and WANT.  Each walker states its own calls and its own want(...), which reports a miss in the walker's terms.
#pragma once
#include "../../include/fthmc_hip.h"

#include <stdio.h>
#include <stdlib.h>

static long calls = 0, refusals = 0;

// device pointers are never dereferenced by the host side: stand-in addresses
static inline double* dev(int k) { return (double*)(uintptr_t)(0x10000000ull + 0x1000000ull * (unsigned)k); }
static inline const int64_t* seeds() { return (const int64_t*)(uintptr_t)0x70000000ull; }
static inline int32_t* ints(int k) { return (int32_t*)(uintptr_t)(0x80000000ull + 0x1000000ull * (unsigned)k); }
static inline void* wsp() { return (void*)(uintptr_t)0x90000000ull; }

// one call, counted: did it answer the expected code?
static inline bool answered(int rc, int code) {
    ++calls;
    if (code != FTHMC_OK) ++refusals;
    return rc == code;
}
// want(...) of the walker: 0, or 1 behind its report of the miss -- main() ends there
#define WANT(...) do { if (want(__VA_ARGS__)) return 1; } while (0)

static inline int walked() {
    printf("{\"calls\": %ld, \"refusals\": %ld}\n", calls, refusals);
    return 0;
}
