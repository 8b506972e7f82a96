// Stand-alone walk of csrc/integrator.h (plain C++, no HIP) for tests/test_integrators.py: built with AddressSanitizer + UBSan
// by `make -f san.mk san_integrator` and run as a program of its own.  All three integrators, nstep 1 .. 64, every cap from 0 to
// one past the stage count, into heap arrays of exactly `cap` entries (a write past cap is a heap overflow the sanitizer reports);
// the refusals; the expanded list against Sched::stage and against the sums every schedule must have.
#include "integrator.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>

using namespace fthmc;

static int fail(const char* what, int integ, int nstep, int cap) {
    fprintf(stderr, "integrator_walk: %s (integrator %d, nstep %d, cap %d)\n", what, integ, nstep, cap);
    return 1;
}

int main() {
    long calls = 0, refusals = 0;
    const double dts[3] = {0.125, 0.1, 1.0 / 3.0};
    for (int integ = 0; integ < 3; ++integ)
        for (int nstep = 1; nstep <= 64; ++nstep) {
            const int n = integrator_forces(integ, nstep);
            const int want = integ == 0 ? nstep : (integ == 1 ? 2 * nstep : 3 * nstep + 1);
            if (n != want) return fail("wrong stage count", integ, nstep, 0);
            const double dt = dts[nstep % 3];
            for (int cap = 0; cap <= n + 1; ++cap) {
                int* kind = (int*)malloc(sizeof(int) * (cap ? cap : 1));
                double* a = (double*)malloc(sizeof(double) * (cap ? cap : 1));
                double* b = (double*)malloc(sizeof(double) * (cap ? cap : 1));
                if (!kind || !a || !b) return fail("out of memory", integ, nstep, cap);
                for (int i = 0; i < cap; ++i) { kind[i] = -7; a[i] = -7.0; b[i] = -7.0; }
                double b0 = -7.0;
                const int rc = expand_sched(integ, dt, nstep, &b0, kind, a, b, cap);
                ++calls;
                if (cap < n) {
                    ++refusals;
                    if (rc != -3) return fail("a short cap was not refused", integ, nstep, cap);
                    if (b0 != -7.0) return fail("b0 written by a refused call", integ, nstep, cap);
                    for (int i = 0; i < cap; ++i)
                        if (kind[i] != -7 || a[i] != -7.0 || b[i] != -7.0) return fail("arrays written by a refused call", integ, nstep, cap);
                } else {
                    if (rc != n) return fail("wrong return value", integ, nstep, cap);
                    Sched sc;
                    if (make_sched(integ, dt, nstep, &sc) != n || sc.n != n || sc.b0 != b0) return fail("make_sched disagrees", integ, nstep, cap);
                    double kick = 0.0, drift = b0;
                    for (int i = 0; i < n; ++i) {
                        const SchedStage st = sc.stage(i);
                        if (st.kind != kind[i] || st.a != a[i] || st.b != b[i]) return fail("stage() and the expanded list disagree", integ, nstep, cap);
                        if (kind[i] == FT_STAGE_SHIFT) {
                            if (b[i] != 0.0 || i + 1 >= n || i == 0) return fail("a SHIFT stage with a drift, or at an end", integ, nstep, cap);
                        } else { kick += a[i]; drift += b[i]; }
                    }
                    const double tau = dt * nstep;
                    if (fabs(kick - tau) > 1e-13 * tau || fabs(drift - tau) > 1e-13 * tau) return fail("coefficients do not sum to tau", integ, nstep, cap);
                    for (int i = n; i < cap; ++i)
                        if (kind[i] != -7 || a[i] != -7.0 || b[i] != -7.0) return fail("written past the stage count", integ, nstep, cap);
                }
                free(kind); free(a); free(b);
            }
        }
    // refusals: unknown integrators, nstep < 1, a count beyond int, null pointers
    double b0 = 0.0, a1[1], b1[1]; int k1[1];
    Sched sc;
    const int bad_int[4] = {-1, 3, 7, 1 << 30};
    for (int i = 0; i < 4; ++i) {
        if (integrator_forces(bad_int[i], 4) != -2 || make_sched(bad_int[i], 0.1, 4, &sc) != -2 ||
            expand_sched(bad_int[i], 0.1, 4, &b0, k1, a1, b1, 1) != -2) return fail("unknown integrator accepted", bad_int[i], 4, 1);
        refusals += 3;
    }
    for (int integ = 0; integ < 3; ++integ) {
        if (integrator_forces(integ, 0) != -1 || integrator_forces(integ, -5) != -1) return fail("nstep < 1 accepted", integ, 0, 0);
        if (integ > 0 && integrator_forces(integ, 0x7fffffff) != -1) return fail("a stage count beyond int accepted", integ, 0x7fffffff, 0);
        if (expand_sched(integ, 0.1, 1, nullptr, k1, a1, b1, 8) != -3 || expand_sched(integ, 0.1, 1, &b0, nullptr, a1, b1, 8) != -3)
            return fail("a null pointer accepted", integ, 1, 8);
        refusals += 4;
    }
    if (integrator_forces(0, 0x7fffffff) != 0x7fffffff) return fail("leapfrog's largest nstep refused", 0, 0x7fffffff, 0);
    printf("{\"calls\": %ld, \"refusals\": %ld}\n", calls, refusals);
    return 0;
}
