// The molecular-dynamics integrators as ONE statement: a schedule.  Plain C++, no HIP: the host sequencer (api.hip), the
// one-launch kernels (wilson.hip k_hmc_trajectory_sched, flow_small.hip k_ft_small<..., SCHED>) and the exported
// fthmc_integrator_schedule all read stage `it` from the same periodic form below.
//
// A trajectory's MD is an initial drift x += b0 v followed by stages; g(y) is the gradient of the action:
//   KICK(a, b):  v -= a g(x*);  x += b v      x* = x, or the shifted field when a SHIFT stage came just before
//   SHIFT(c):    x~ = x - c g(x)              the next stage evaluates its gradient at x~; x and v are untouched
// Every stage costs one force evaluation.
//   leapfrog                         b0 = dt/2     nstep x KICK(dt, dt), the last b = dt/2
//   Omelyan 2MN (position version)   b0 = lam dt   per step KICK(dt/2, (1 - 2 lam) dt), KICK(dt/2, 2 lam dt); the very last b = lam dt
//     (Omelyan, Mryglod & Folk 2003: lam minimises the norm of the leading error term)
//   force-gradient, 4th order        b0 = 0        KICK(dt/6, dt/2); per step SHIFT(dt^2/24), KICK(2 dt/3, dt/2); between steps
//     (B A B_FG A B with the end kicks of neighbouring steps merged; the force-gradient term as ONE shifted re-evaluation of the
//      force, Yin & Mawhinney 2011)                KICK(dt/3, dt/2); last KICK(dt/6, 0)
#ifndef FTHMC_INTEGRATOR_H
#define FTHMC_INTEGRATOR_H

#ifndef FTHMC_INT_LEAPFROG
#define FTHMC_INT_LEAPFROG        0
#define FTHMC_INT_OMELYAN         1
#define FTHMC_INT_FORCE_GRADIENT  2
#endif

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FT_SCHED_HD __host__ __device__
#else
#define FT_SCHED_HD
#endif

namespace fthmc {

constexpr double FT_OMELYAN_LAMBDA = 0.1931833275037836;
enum { FT_STAGE_KICK = 0, FT_STAGE_SHIFT = 1 };

struct SchedStage {
    int kind;        // FT_STAGE_KICK / FT_STAGE_SHIFT
    double a, b;     // KICK(a, b); SHIFT: a = c, b = 0
};

// The periodic form: stage `it` of `n` is `last` at it == n - 1, else `first` at it == 0, else per[it % nper].  (Plain data: it
// travels to the one-launch kernels inside their argument blocks.)
struct Sched {
    double b0;
    int n, nper;
    SchedStage first, last, per[3];
    FT_SCHED_HD SchedStage stage(int it) const {
        if (it == n - 1) return last;
        if (it == 0) return first;
        const int k = it % nper;
        return k == 0 ? per[0] : (k == 1 ? per[1] : per[2]);
    }
};

// force evaluations (= stages) of a trajectory; < 0: unknown integrator (-2) or nstep < 1 (-1)
inline int integrator_forces(int integrator, int nstep) {
    if (integrator != FTHMC_INT_LEAPFROG && integrator != FTHMC_INT_OMELYAN && integrator != FTHMC_INT_FORCE_GRADIENT) return -2;
    if (nstep < 1) return -1;
    const long long n = integrator == FTHMC_INT_LEAPFROG ? (long long)nstep
                      : integrator == FTHMC_INT_OMELYAN ? 2ll * nstep : 3ll * nstep + 1;
    return n > 0x7fffffffll ? -1 : (int)n;
}

// the schedule of (integrator, dt, nstep); returns integrator_forces() (< 0: *s is not written)
inline int make_sched(int integrator, double dt, int nstep, Sched* s) {
    const int n = integrator_forces(integrator, nstep);
    if (n < 0) return n;
    Sched q{};
    q.n = n;
    const SchedStage none{FT_STAGE_KICK, 0.0, 0.0};
    q.per[0] = q.per[1] = q.per[2] = none;
    if (integrator == FTHMC_INT_LEAPFROG) {
        q.b0 = 0.5 * dt;
        q.nper = 1;
        q.per[0] = SchedStage{FT_STAGE_KICK, dt, dt};
        q.first = q.per[0];
        q.last = SchedStage{FT_STAGE_KICK, dt, 0.5 * dt};
    } else if (integrator == FTHMC_INT_OMELYAN) {
        const double lam = FT_OMELYAN_LAMBDA;
        q.b0 = lam * dt;
        q.nper = 2;
        q.per[0] = SchedStage{FT_STAGE_KICK, 0.5 * dt, (1.0 - 2.0 * lam) * dt};
        q.per[1] = SchedStage{FT_STAGE_KICK, 0.5 * dt, 2.0 * lam * dt};
        q.first = q.per[0];
        q.last = SchedStage{FT_STAGE_KICK, 0.5 * dt, lam * dt};
    } else {
        q.b0 = 0.0;
        q.nper = 3;
        q.per[0] = SchedStage{FT_STAGE_KICK, dt / 3.0, 0.5 * dt};            // between steps: the merged end kicks
        q.per[1] = SchedStage{FT_STAGE_SHIFT, dt * dt / 24.0, 0.0};
        q.per[2] = SchedStage{FT_STAGE_KICK, 2.0 * dt / 3.0, 0.5 * dt};
        q.first = SchedStage{FT_STAGE_KICK, dt / 6.0, 0.5 * dt};
        q.last = SchedStage{FT_STAGE_KICK, dt / 6.0, 0.0};
    }
    *s = q;
    return n;
}

// the expanded list: kind[i], a[i], b[i] of stage i < n (cap: the arrays' length).  Returns n; -3 if cap < n (nothing is
// written then), integrator_forces()'s codes otherwise.
inline int expand_sched(int integrator, double dt, int nstep, double* b0, int* kind, double* a, double* b, int cap) {
    Sched q;
    const int n = make_sched(integrator, dt, nstep, &q);
    if (n < 0) return n;
    if (cap < n || !b0 || !kind || !a || !b) return -3;
    *b0 = q.b0;
    for (int it = 0; it < n; ++it) {
        const SchedStage st = q.stage(it);
        kind[it] = st.kind; a[it] = st.a; b[it] = st.b;
    }
    return n;
}

}  // namespace fthmc

#endif
