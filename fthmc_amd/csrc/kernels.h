// Internal launch interface between the translation units of libfthmc_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "integrator.h"

namespace fthmc {

// FlowLayerArgs::stash_far (api.hip sweep_forward): a layer's stash counts as gone from the caches when the layers behind it write this
// much before the backward returns to it -- the 256 MB Infinity Cache over two chain groups, each writing and reading back
constexpr size_t STASH_FAR_BYTES = (size_t)64 << 20;

// one workgroup per chain: its size for an L x L lattice.  Every chain sum (action, charge, kinetic energy, k_traj_energy, the instanton
// hit's C and Sn) is launched with it, so that the same sum is bit-identical wherever it is formed
inline int chain_threads(int L) { return L * L >= 4096 ? 1024 : (L * L >= 1024 ? 512 : 256); }

// ---- wilson.hip
int launch_wrap(const double* x, double* o, size_t n, int reg, hipStream_t s);
int launch_axpy(const double* x, const double* p, double a, double* o, size_t n, hipStream_t s);
int launch_plaq(const double* x, double* P, int B, int L, hipStream_t s);
// wave_part (optional): 32 B doubles of scratch; with it a few chains of a large lattice (B < 128, L >= 128) run one wave per
// workgroup instead of one workgroup per chain -- the same sums in the same order, bit-identical
// beta_b (optional, here and below): per-chain beta, a device array [B] read in place of `beta` (the per-chain-beta entry points,
// fthmc_*_pb); null: the instances and argument lists every other caller has always run
// Csum (optional, with beta_b only): sum cos P per chain, the beta-free row of the carried state
int launch_action_charge(const double* x, int B, int L, double beta, double* S, double* Q,
                         double* plaq, hipStream_t s, double* wave_part = nullptr, const double* beta_b = nullptr,
                         double* Csum = nullptr);
int launch_kinetic(const double* v, int B, int L, double* K, hipStream_t s);
int launch_lincomb(const double* a, double ca, const double* b, double cb, double c0, double* out,
                   int B, hipStream_t s);
int launch_stats_accumulate(const double* acc, const double* plaq, const double* Q, double* qold, const double* dH, int B,
                            double* vec, hipStream_t s);
int launch_wilson_force(const double* x, int B, int L, double beta, double* F, hipStream_t s);
void set_leap_rows(int v);      // 1 (default): row-strip leapfrog kernel when L % 64 == 0; 0: 16 x 16 tiles always
int launch_leap_step(const double* x, const double* p, double* xo, double* po, int B, int L,
                     double beta, double a, double dt, hipStream_t s, const double* beta_b = nullptr);
int launch_wilson_gp(const double* x, int B, int L, double beta, double* gp, hipStream_t s, const double* beta_b = nullptr);
// whole plain-HMC trajectory in one launch (L <= HMC_RESIDENT_MAXL: links in LDS, momenta in registers; the plan: traj_resident.h)
constexpr int HMC_RESIDENT_MAXL = 64;
int launch_hmc_trajectory_fused(const double* x, const double* v, const double* u, int B, int L, double beta,
                                double dt, int nstep, double* x_new, double* dH, double* acc, double* H0,
                                double* H1, hipStream_t s);
int launch_kick_from_gp(const double* gp, double* v, double* xq, double* Fout, int B, int L,
                        double dt, double a, hipStream_t s, double* xreg = nullptr);   // xreg: also regularize(x') (end of the MD)
// the SHIFT stage of a schedule (integrator.h): xs = x - c adj(gP); x, v and gP are only read
int launch_shift_from_gp(const double* gp, const double* x, double* xs, int B, int L, double c, hipStream_t s);
// plain HMC of a schedule in one launch (L <= 64): launch_hmc_trajectory_fused's twin
int launch_hmc_trajectory_sched(const double* x, const double* v, const double* u, int B, int L, double beta, const Sched& sched,
                                double* x_new, double* dH, double* acc, double* H0, double* H1, hipStream_t s,
                                const double* beta_b = nullptr);
// the scalars of one end of a flowed trajectory in one launch: (S_eff, plaq, Q) of the flowed field (or carried over: state_in)
// and H = S_eff + sum v^2 / 2
int launch_traj_energy(const double* xphys, int B, int L, double beta, const double* lj_part, int np, int nsets,
                       const double* state_in, const double* v, double* trip, double* H, hipStream_t s,
                       const double* beta_b = nullptr);   // beta_b: trip and state_in are the BETA-FREE triple (log det J, sum cos P, Q)
// S_eff (has_ld: minus row 0) and plaq from the beta-free state st[3][B] = (log det J, sum cos P, Q) and beta_b
int launch_pb_from_state(const double* st, const double* beta_b, int B, int L, int has_ld, double* seff, double* plaq, hipStream_t s);
// one replica-exchange round of parity 0 / 1 over M ladders of K chains (wilson.hip k_replica_swap); every ladder in order
int launch_replica_swap(const double* betas, int K, int M, int parity, const double* C, const double* u, double* beta_b, int* rung,
                        int* chain_of, double* swap_acc, double* d, hipStream_t s);
// betas_host (host, K doubles) is read DURING the call: it travels to `betas` by value, in kernel arguments
int launch_ladder_init(const double* betas_host, double* betas, int K, int M, double* beta_b, int* rung, int* chain_of, hipStream_t s);
int launch_axpy_copy(const double* x, const double* p, double a, double* xo, double* po, size_t n, hipStream_t s);
int launch_plane_from(const double* g, int B, int L, int mu, double sign, double* out, hipStream_t s);   // out[b][mu][:] = sign * g[b][:]
int launch_metropolis(const double* x_old, const double* x_prop, const double* u, const double* H0,
                      const double* H1, int B, int L, int xform, double* x_new, double* dH,
                      double* acc, const double* obs_old, const double* obs_new, double* obs_out,
                      int n_obs, hipStream_t s, double* o1 = nullptr, double* o2 = nullptr);   // o1, o2: selected observables 1, 2

int launch_train_metrics(const double* logq, const double* logp, const double* q, const double* qi, int B,
                         double inv_beta_vol, double dkl_factor, double* row, hipStream_t s);
int launch_adam(double* p, const double* g, double* m, double* v, double* hp, size_t n, double b1, double b2, double eps,
                double wd, int decoupled, hipStream_t s);       // hp: [t, lr, ticket] on the device

// ---- loops.hip: the table of rectangular Wilson loops W[b][R-1][T-1], R <= Rmax, T <= Tmax (fthmc_wilson_loops)
constexpr int LP_THREADS = 256;               // threads of a walking workgroup
constexpr int LP_SITES = 1024;                // sites a workgroup walks at a time: four per thread, 32 KB of LDS planes
constexpr int LP_LDS_MAXL = 1024;             // beyond it a row of the planes (32 L bytes) lives in global scratch
constexpr int LP_BIG_WGS = 1024;              // workgroups (and scratch slots) of that path
// How a call is cut up, and its workspace in doubles: prefix[B][L+1][L] | part[B][Rmax][nblk][Tmax] | scratch (L > LP_LDS_MAXL).
// ok = false: a size beyond size_t (no workspace can hold it)
struct LoopsGeom {
    bool ok, lds;
    int rows, nblk, nwg;                      // rows per workgroup, partials per (chain, R), workgroups of the large-L path
    size_t prefix, part, scratch, total;
};
inline LoopsGeom loops_geom(int B, int L, int Rmax, int Tmax) {
    LoopsGeom g{};
    g.lds = L <= LP_LDS_MAXL;
    if (g.lds) {
        g.rows = LP_SITES / L < 1 ? 1 : (LP_SITES / L > L ? L : LP_SITES / L);
        g.nblk = (L + g.rows - 1) / g.rows;
    } else {
        g.rows = 1;
        g.nblk = L * ((L + LP_SITES - 1) / LP_SITES);
        const long long items = (long long)B * Rmax * L;
        g.nwg = items < LP_BIG_WGS ? (int)items : LP_BIG_WGS;
    }
    auto pad = [](size_t n) { return (n + 31) / 32 * 32; };    // regions start on 256 B: the planes are read 16 bytes at a time
    size_t p = 0;
    g.prefix = pad((size_t)B * (size_t)(L + 1) * (size_t)L);            // < 2^22 2^30: fits
    g.ok = !__builtin_mul_overflow((size_t)B * (size_t)Rmax, (size_t)g.nblk * (size_t)Tmax, &p) && p < ((size_t)1 << 59);
    g.part = g.ok ? pad(p) : 0;
    g.scratch = g.lds ? 0 : pad((size_t)g.nwg * 4 * ((size_t)L + (size_t)Tmax));
    g.total = g.prefix + g.part + g.scratch;
    return g;
}
// prefix, part, scratch: the three regions of the workspace (api.hip carves them)
int launch_wilson_loops(const double* x, int B, int L, int Rmax, int Tmax, double* W, double* Wmean, double* prefix, double* part,
                        double* scratch, hipStream_t s);

// ---- local.hip: heatbath / overrelaxation sweeps of the plain Wilson action (fthmc_local_update)
constexpr int LU_MAXL = 64;                   // up to here a chain's links stay in one workgroup's LDS for the whole call
constexpr int LU_MAX_ATTEMPTS = 64;           // rejection attempts of one heatbath draw, at most: a link that uses them up keeps its value
// classes: bit (2 mu + parity) set = that class is updated; sweep0: index of the call's first heatbath sweep in the Philox counter;
// resident: the one-launch kernel (L <= LU_MAXL), else one launch per class and sweep; beta_b: per-chain beta or null
int launch_local_update(const double* x, int B, int L, double beta, const double* beta_b, const int64_t* seeds, int n_hb, int n_or,
                        int nsweep, uint32_t sweep0, int classes, double* x_out, bool resident, hipStream_t s);
// annealing (fthmc_anneal): n_step steps of W += (betas[k] - betas[k+1]) sum cos P, then nsweep compound sweeps at
// betas[k+1] (a device array [n_step + 1]); resident: the whole ramp in one launch (L <= LU_MAXL), else per step a work kernel and the
// class kernels; work_in, c_trace ([B][n_step + 1]): optional; x_out may be x, work_out may be work_in
constexpr int AN_MAX_STEPS = 65536;
int launch_anneal(const double* x, int B, int L, const double* betas, int n_step, const int64_t* seeds, int n_hb, int n_or, int nsweep,
                  uint32_t sweep0, const double* work_in, double* x_out, double* work_out, double* c_trace, bool resident, hipStream_t s);

// ---- topo.hip: instanton hits, the Metropolis update across topological sectors (fthmc_instanton_hit)
// split: one wave per workgroup + decision + apply (part: [B][chain_threads(L) / 64][2] doubles, kbuf: [B] int32) in place of one
// workgroup per chain (part, kbuf unused); k_out, nacc_out, cs_out: optional; x_out may be x
inline size_t instanton_part_doubles(int B, int L) { return (size_t)B * (size_t)(chain_threads(L) / 64) * 2; }
int launch_instanton(const double* x, int B, int L, double beta, const double* beta_b, const int64_t* seeds, int n_hit, uint32_t hit0,
                     bool split, double* x_out, int32_t* k_out, int32_t* nacc_out, double* cs_out, double* part, int32_t* kbuf, hipStream_t s);

// ---- meta.hip: metadynamics HMC, plain HMC under a bias potential in the continuous charge (fthmc_meta_*)
// the table of a call: v[G][nb] on the nodes -qmax + i 2 qmax / (nb - 1), chain b reads row b / cpr (cpr = B / G), the wall outside
struct MetaTab { const double* v; int cpr, nb; double qmax, wall; };
// the whole biased trajectory in one launch (L <= 64): launch_hmc_trajectory_sched's twin; qm_out, vb_out: of the field x_new holds
int launch_meta_trajectory(const double* x, const double* v, const double* u, int B, int L, double beta, const Sched& sched, const MetaTab& T,
                           double* x_new, double* dH, double* acc, double* H0, double* H1, double* qm_out, double* vb_out, hipStream_t s);
// the sequenced path: sums[B][2] = (sum sin P, sum cos P); gP = beta sin P + c_b cos P; H[b] += V(Q_m), qv[2][B] = (Q_m, V)
int launch_meta_sums(const double* x, int B, int L, double* sums, hipStream_t s);
int launch_meta_gp(const double* x, int B, int L, double beta, const double* sums, const MetaTab& T, double* gp, hipStream_t s);
int launch_meta_energy(const double* sums, int B, const MetaTab& T, double* H, double* qv, hipStream_t s);
// the same at a carried charge qm[B] (no field): H[b] += V(qm[b]), vb[b] = V(qm[b]); each optional
int launch_meta_energy_qm(const double* qm, int B, const MetaTab& T, double* H, double* vb, hipStream_t s);
// the bias on its own
int launch_meta_force(const double* x, int B, int L, double beta, const MetaTab& T, double* F, hipStream_t s);
int launch_meta_action(const double* x, int B, int L, double beta, const MetaTab& T, double* S, double* qm, double* vb, hipStream_t s);
// one hill of height w per walker at qm[b], added to the table in chain order (in place)
int launch_meta_deposit(const double* qm, int B, int G, int nb, double qmax, double w, double* vtab, hipStream_t s);

// ---- defect.hip: boundary-condition tempering, plain HMC with a per-chain coupling g_b on a line of plaquettes (fthmc_defect_*)
// the defect of a call: the plaquettes ((i0 + a) mod L, j0), 0 <= a < Ld, the same for every chain
struct DefectLine { int i0, j0, Ld; };
// the whole trajectory in one launch (L <= 64): launch_hmc_trajectory_sched's twin; csum_out, dsum_out, q_out: of the field x_new holds
int launch_defect_trajectory(const double* x, const double* v, const double* u, int B, int L, double beta, const double* g_b,
                             const DefectLine& df, const Sched& sched, double* x_new, double* dH, double* acc, double* H0, double* H1,
                             double* csum_out, double* dsum_out, double* q_out, hipStream_t s);
// the sequenced path: S[b] = (-beta) C (optional), sums[3][B] = (C, Dsum, Q); gP = w sin P; H[b] += (beta - g_b) Dsum.  B <= 65535 (launch_defect_gp)
int launch_defect_sums(const double* x, int B, int L, double beta, const DefectLine& df, double* S, double* sums, hipStream_t s);
int launch_defect_gp(const double* x, int B, int L, double beta, const double* g_b, const DefectLine& df, double* gp, hipStream_t s);
int launch_defect_energy(const double* sums, int B, double beta, const double* g_b, double* H, hipStream_t s);
// the pieces on their own
int launch_defect_force(const double* x, int B, int L, double beta, const double* g_b, const DefectLine& df, double* F, hipStream_t s);
int launch_defect_action(const double* x, int B, int L, double beta, const double* g_b, const DefectLine& df, double* S, double* csum,
                         double* dsum, double* Q, hipStream_t s);
// the chains on rung `top` translated by shift[b] = (s0, s1), every other chain copied; x_out != x
int launch_defect_translate(const double* x, int B, int L, const int32_t* rung, int top, const int32_t* shift, double* x_out, hipStream_t s);

// ---- rng.hip
int launch_random_momenta(const int64_t* seeds, int B, int n, double* v, double* u, hipStream_t s);
int launch_random_uniform(const int64_t* seeds, int B, int n, double lo, double hi, double* out, hipStream_t s);
int launch_chain_seeds(int64_t seed, int64_t lo, int B, int64_t traj, int64_t* counter, int advance, int64_t* seeds, hipStream_t s);

// ---- flow.hip
constexpr int FLOW_TILE = 16;                 // VALU variant (flow.hip): 16 x 16 sites per tile
constexpr int FLOW_R0 = FLOW_TILE + 6;        // plaquette / net-input window edge
constexpr int FLOW_N0 = FLOW_R0 * FLOW_R0;    // window size of one gP partial
constexpr int FLOW_WINT = 9856;               // doubles per layer, kernel-side weight layout
// The expansion of layer l is guarded by STAMPS inside the layer's own region (its last FLOW_WSTAMPS doubles, one per
// workgroup of k_pack_weights): a workgroup that finds its stamp equal to the token of the call (caller's weight version,
// address of the canonical weights, layer) leaves at once, otherwise it expands its slice and writes the token.  The
// first FLOW_WHEAD_LAYERS layer regions are a FIXED head of every workspace layout (ws_layout): no other region of any call,
// whatever its shape, overlaps them, so a stamp vouches for the data it sits behind; layers beyond the head are expanded
// by every call.
constexpr int FLOW_WSTAMPS = 8, FLOW_WSTAMP0 = FLOW_WINT - FLOW_WSTAMPS;
constexpr int FLOW_WHEAD_LAYERS = 64;
constexpr int FLOW_GW_STRIDE = 960;           // doubles per (chain, tile) weight-gradient partial

// tile geometry of a variant: partial buffers are indexed [chain][tile][window]
struct FlowGeom {
    int tr, tc;
    int nti(int L) const { return (L + tr - 1) / tr; }
    int ntj(int L) const { return (L + tc - 1) / tc; }
    int ntiles(int L) const { return nti(L) * ntj(L); }
    int n0() const { return (tr + 6) * (tc + 6); }
};
// tile of the MFMA forward kernel: 16 x 16 measured faster than 8 x 16 at 3 workgroups per CU (79 vs 94 us)
constexpr int MF_FWD_TR = 16, MF_FWD_TC = 16;
inline FlowGeom flow_fwd_geom(bool mfma) { return mfma ? FlowGeom{MF_FWD_TR, MF_FWD_TC} : FlowGeom{FLOW_TILE, FLOW_TILE}; }
inline FlowGeom flow_geom(bool) { return FlowGeom{FLOW_TILE, FLOW_TILE}; }          // VALU variant: partial buffers [chain][tile][window]
// workspace sizing: the larger of the two variants
inline size_t flow_ntiles_max(int L) {
    size_t a = flow_geom(false).ntiles(L), b = 2 * FlowGeom{16, 16}.ntiles(L);   // VALU / forward tiles; weight-gradient partials: two per 16 x 16 tile
    return a > b ? a : b;
}
inline size_t flow_gp_part_max(int L) { return (size_t)flow_geom(false).ntiles(L) * flow_geom(false).n0(); }

// canonical (955/layer, PyTorch order) -> kernel layout (FLOW_WINT/layer)
// token = 0: expand unconditionally (and clear the stamps); else see FLOW_WSTAMPS above
int launch_pack_weights(const double* w, int n_layers, double* wint, hipStream_t s, unsigned long long token = 0ull);

// layer l of a flow: stripe direction and offset (fthmc/utils/layers.py: the eight masks of a block, in order)
inline int layer_mu(int l) { return l % 2; }
inline int layer_off(int l) { return (l / 2) % 4; }

struct FlowLayerArgs {
    const double* x;         // [B][2][L][L] layer input
    const double* wint;      // this layer's weights, kernel layout
    double* y;               // fwd / rev: output field (may alias x)
    const double* pin;       // fwd / rev, plaquette-level map: input plaquette field [B][L][L] (then x is unused)
    double* pout;            // fwd / rev, plaquette-level map: output plaquette field [B][L][L]
    double* logj_part;       // fwd / rev: [B][ntiles]
    const double* up_link;   // bwd: upstream link gradient [B][2][L][L] or null
    const double* up_gp;     // bwd: upstream plaquette-gradient field [B][L][L] or null
    const double* glogj;     // bwd: [B] or null (then glogj_const)
    double glogj_const;
    double* gp_part;         // bwd, scatter form: [B][ntiles][FLOW_N0]
    double* gp_out;          // bwd, gather form: plaquette-gradient field after this layer [B][L][L] (not up_gp)
    double* gw_part;         // bwd with wgrad: [B*ntiles][FLOW_GW_STRIDE]
    double tol;              // rev
    long long* dbg;          // optional: per-(chain,tile) stage time stamps [16] (diagnostic runs only)
    double* stash;           // optional: this layer's activation stash (MFMA forward writes, stash backward reads)
    int stash_h;             // forward: also stash h1, h2 (training: the weight gradients need them)
    int stash_far;           // forward: this layer's stash will have left the caches when the backward comes for it (sweep_forward)
    int inplace;             // forward, MFMA variant: y == x and the layer loads and stores only the links it changes (flow_fwd.hip INPL:
                             // the sweep instances of the exact tiles; any other instance copies the field onto itself)
    double* gz;              // training: gradients wrt the pre-activations of this layer, written by the backward kernel at
                             // every tile's own sites and read by k_flow_wgrad: per chain gz2 [n][8], gz1 [n][8]
                             // (channel-minor), g_out [n/4][4] (dL/ds_0, dL/ds_1, dL/dt, 0 at the active sites, compact)
    int dbg_stop;            // -DFT_DIAG builds: the forward kernel returns after this stage (instruction counts per stage); 0 = run all
    int B, L, mu, off, act;
    // k_flow_wgrad over SEVERAL layers in one launch (small lattices: every layer's gz and stash are there at once): layers
    // 0 .. nlb - 1 (mu, off from the layer index), their stash / gz / partial regions `*_lstride` doubles apart; nlb = 0: one layer
    int nlb;
    size_t stash_lstride, gz_lstride, gwp_lstride;
    int tpw;                 // k_flow_wgrad: (chain, tile) items a workgroup walks (flow_wgrad_tpw; 0 = 1)
    int wg_ns;               // k_flow_wgrad: stride of the walk = workgroups that stand on consecutive tiles (set by the launcher)
    // host side: everything zero / null but the layer's weights, shape and stripe
    FlowLayerArgs() = default;
    FlowLayerArgs(const double* wint_, int B_, int L_, int mu_, int off_, int act_) {
        *this = FlowLayerArgs();
        wint = wint_; B = B_; L = L_; mu = mu_; off = off_; act = act_;
    }
    // layer l of a flow whose expanded weights start at wint0
    FlowLayerArgs(const double* wint0, int l, int B_, int L_, int act_)
        : FlowLayerArgs(wint0 + (size_t)l * FLOW_WINT, B_, L_, layer_mu(l), layer_off(l), act_) {}
};
int launch_flow_fwd(const FlowLayerArgs& a, hipStream_t s);
int launch_flow_rev(const FlowLayerArgs& a, hipStream_t s);
int launch_flow_bwd(const FlowLayerArgs& a, bool wgrad, hipStream_t s);
// flow_fwd.hip: MFMA forward (same arguments and results as launch_flow_fwd; optionally writes the stash)
int launch_flow_fwd_mfma(const FlowLayerArgs& a, hipStream_t s);
// the shapes whose sweeps run layers 1 .. nl - 1 in place (api.hip sweep_forward): the exact tiles of flow_fwd.hip (16 x 16 tiles
// that divide a power-of-two lattice) with the activation its sweep instances are compiled for
inline bool flow_fwd_inplace_ok(int L, int act) {
    return L % MF_FWD_TR == 0 && L % MF_FWD_TC == 0 && (L & (L - 1)) == 0 && act == 0 /* FTHMC_ACT_SILU */;
}
// the inverse layer on the same kernel (conv net unchanged, scalar map inverted by safeguarded Newton)
int launch_flow_rev_mfma(const FlowLayerArgs& a, hipStream_t s);
// flow_bwd_gather.hip: backward from the stash in gather form: a tile produces the complete
// gP_out = up_gp + layer contribution of its own sites (a.gp_out, out of place), no partial windows;
// with a.gz (training) it also writes the pre-activation gradients for launch_flow_wgrad
constexpr int MG_TR = 16, MG_TC = 16;
inline FlowGeom flow_gather_geom() { return FlowGeom{MG_TR, MG_TC}; }
int launch_flow_bwd_gather(const FlowLayerArgs& a, hipStream_t s);
// flow_wgrad.hip: weight gradients of one layer from a.gz and the stashed h1, h2, cos / sin: a workgroup walks a.tpw
// (chain, 16 x 16 tile) items and writes TWO 955-entry partials (halves of the tiles' sites) to
// a.gw_part [flow_wgrad_nparts(B, L, tpw)][FLOW_GW_STRIDE]
int launch_flow_wgrad(const FlowLayerArgs& a, hipStream_t s);
inline size_t flow_gz_doubles(int B, int L) { return (size_t)B * 17 * L * L; }
inline int flow_wgrad_parts(int L) { return 2 * FlowGeom{MG_TR, MG_TC}.ntiles(L); }          // per chain at one item per workgroup: sizes the workspace
// How the (chain, 16 x 16 tile) items of a launch are shared among workgroups that WALK several of them (k_flow_wgrad,
// k_flow_bwd_train; the kernels' side: flow_bwd_common.h walk_of_block).  tpw: items per workgroup -- as many as leave one
// workgroup for each of the chip's `slots`, at most max_tpw (round_up: no slot takes more than one workgroup); ns: workgroups
// of one XCD that walk side by side, one per slot of the XCD (fewer when the launch is smaller than the chip), at most max_ns;
// nparts: the workgroups that walk at least one item = the rows of partials the launch writes (the kernels number those 0, 1,
// 2, ...); grid.x = 8 XCDs x rounds x ns.  All in 64-bit arithmetic, for the callers that ask before they check the shape (ws_layout).
struct WalkPlan { int slots, max_tpw, max_ns; bool round_up; };
constexpr WalkPlan WALK_WGRAD = {512, 8, 64, false};        // two workgroups per CU: 512 slots, 32 CUs x 2 per XCD
constexpr WalkPlan WALK_BWD_TRAIN = {256, 64, 32, true};    // one workgroup per CU: 256 slots, 32 per XCD
inline long walk_items(int B, int L) { return (long)B * FlowGeom{MG_TR, MG_TC}.ntiles(L); }
inline int walk_tpw(const WalkPlan& p, long items) {
    const long t = (items + (p.round_up ? p.slots - 1 : 0)) / p.slots;
    return t < 1 ? 1 : t > p.max_tpw ? p.max_tpw : (int)t;
}
inline int walk_ns(const WalkPlan& p, long items, int tpw) {
    const long n = (items + 8 * tpw - 1) / (8 * tpw);
    return n < 1 ? 1 : n > p.max_ns ? p.max_ns : (int)n;
}
inline long walk_nparts(const WalkPlan& p, long items, int tpw) {
    const long ns = walk_ns(p, items, tpw), k0 = items / (tpw * ns), rem = items - k0 * tpw * ns;
    return k0 * ns + (rem < ns ? rem : ns);
}
inline long walk_grid_x(long items, int tpw, int ns) {
    const long KR = (items + (long)tpw * ns - 1) / ((long)tpw * ns), R = (KR + 7) / 8;
    return 8 * R * ns;
}
// k_flow_wgrad: tpw counts the items of every layer of the launch (blockIdx.y), ns and the partials those of one layer
inline int flow_wgrad_tpw(int B, int L, int nlayers) { return walk_tpw(WALK_WGRAD, walk_items(B, L) * (nlayers > 0 ? nlayers : 1)); }
inline int flow_wgrad_ns(int B, int L, int tpw) { return walk_ns(WALK_WGRAD, walk_items(B, L), tpw); }
inline int flow_wgrad_nparts(int B, int L, int tpw) { return (int)walk_nparts(WALK_WGRAD, walk_items(B, L), tpw); }
// flow_bwd_train.hip: the training backward WITH the layer's weight gradients in one kernel (the pre-activation gradients never
// leave LDS): one workgroup per CU walks (chain, tile) items and writes ONE 955-entry partial to a.gw_part
// [flow_bwd_train_nparts(B, L)][FLOW_GW_STRIDE]; a.gp_out as launch_flow_bwd_gather.  Built for the shapes 16 x 16 tiles divide with
// L a power of two (flow_bwd_train_shape); FTHMC_ERR_UNSUPPORTED otherwise: the caller keeps the two-kernel form.
int launch_flow_bwd_train(const FlowLayerArgs& a, hipStream_t s);
inline bool flow_bwd_train_shape(int L) { return L >= 32 && (L & (L - 1)) == 0; }
inline int flow_bwd_train_tpw(int B, int L) { return walk_tpw(WALK_BWD_TRAIN, walk_items(B, L)); }
inline int flow_bwd_train_ns(int B, int L, int tpw) { return walk_ns(WALK_BWD_TRAIN, walk_items(B, L), tpw); }
// the launcher serves flow_stash_fits32 shapes only, where this fits an int with room to spare
inline long flow_bwd_train_nparts(int B, int L) { return walk_nparts(WALK_BWD_TRAIN, walk_items(B, L), flow_bwd_train_tpw(B, L)); }
// doubles per layer of the stash (layout: flow_mfma_common.h struct Stash): 19 per site, 35 with h1, h2 (training)
inline size_t flow_stash_doubles(int B, int L, bool train = false) { return (size_t)B * (train ? 35 : 19) * L * L; }
// the tuned kernels form a chain's plane offsets inside one layer's stash in 32 bits (flow_mfma_common.h: uniform_at, stash_view)
// -- one layer's stash below 32 GiB; beyond that the launchers return FTHMC_ERR_UNSUPPORTED
inline bool flow_stash_fits32(int B, int L, bool train) { return flow_stash_doubles(B, L, train) < ((size_t)1 << 32); }
// ranges the tuned kernels state as assumptions (__builtin_assume in k_flow_fwd / k_flow_bwd_gather): checked by their launchers
inline bool flow_shape_ok(int B, int L, int off) { return B > 0 && B <= (1 << 20) && L >= 4 && L <= 8192 && (L & 3) == 0 && off >= 0 && off < 4; }
// ---- flow_generic.hip: any s/t net shape (hidden sizes, kernel size, mixture components); plain kernels, HBM-resident planes
constexpr int FLOW_ARCH_MAXH = 8;
// Shape of the s/t conv net: 2 -> hid[0] -> ... -> hid[nh - 1] -> nmix + 1 channels, k x k kernels.  A VALUE that travels with
// every call (fthmc_arch_t of the C ABI; NULL there = the default): nothing about the shape is process state.
struct FlowArch {
    int nh; int hid[FLOW_ARCH_MAXH]; int k; int nmix;
    int tanh_out;            // a tanh behind the last conv (make_conv_net(use_final_tanh=True))
    bool is_default() const { return nh == 2 && hid[0] == 8 && hid[1] == 8 && k == 3 && nmix == 2 && !tanh_out; }   // the tuned kernels serve it
    int chan(int i) const { return i == 0 ? 2 : (i <= nh ? hid[i - 1] : nmix + 1); }                   // channels in front of conv i
    int params() const {                                    // doubles per layer in the canonical (PyTorch-order) weight layout
        int p = 0;
        for (int i = 0; i <= nh; ++i) p += chan(i + 1) * chan(i) * k * k + chan(i + 1);
        return p;
    }
    int cmax() const { int m = 2; for (int i = 1; i <= nh + 1; ++i) m = chan(i) > m ? chan(i) : m; return m; }   // widest activation
    int csum() const { int c = 0; for (int i = 1; i <= nh + 1; ++i) c += chan(i); return c; }
    // per layer: P [B][n], IN [B][2][n], Z_1 .. Z_{nh+1} [B][c_i][n]
    size_t stash_doubles(int B, int L) const { return (size_t)B * L * L * (3 + csum()); }
};
inline FlowArch flow_arch_default() { return FlowArch{2, {8, 8, 0, 0, 0, 0, 0, 0}, 3, 2, 0}; }
// validated copy of a caller's shape (FTHMC_ERR_UNSUPPORTED beyond the limits of flow_generic.hip)
int make_flow_arch(int n_hidden, const int* hidden_sizes, int kernel_size, int n_mix, int final_tanh, FlowArch* out);
// T: double (every first-order call), or Dual (dual.h: the forward-over-reverse sweeps of fthmc_ft_force_vjp; weights and the
// per-chain log J coefficients stay plain doubles)
struct Dual;
template <typename T> struct GenLayerArgsT {
    FlowArch arch;           // the net's shape
    const T* x;              // [B][2][L][L] layer input (null with pin)
    const T* pin;            // plaquette-level map: input plaquette field [B][L][L]
    const double* w;         // this layer's weights, canonical layout
    T* y;                    // forward / reverse: output links (may alias x), or null
    T* pout;                 // plaquette-level map: output plaquette field
    T* logj;                 // [B] or null
    int logj_accumulate;     // logj[b] += instead of =
    double tol;              // reverse
    T* stash;                // this layer's region (arch.stash_doubles): written by the forward, read by the backward
    T* hbuf;                 // [B][cmax][n] scratch: activations of the conv input
    T* gbuf;                 // [2][B][cmax][n] scratch: gradients, ping-pong
    const T* up_gp;          // backward: upstream plaquette gradient [B][L][L] or null
    const T* up_link;        // backward: upstream link gradient [B][2][L][L] or null
    const double* glogj;     // backward: [B] or null (then glogj_const)
    double glogj_const;
    T* gp_out;               // backward: plaquette gradient behind this layer (not up_gp)
    T* gw;                   // backward: this layer's weight gradient (canonical layout) or null
    int B, L, mu, off, act;
};
using GenLayerArgs = GenLayerArgsT<double>;
int launch_gen_fwd(const GenLayerArgs& a, bool rev, hipStream_t s);
int launch_gen_bwd(const GenLayerArgs& a, hipStream_t s);
// the same layer sequences on dual numbers (forward direction, no log J: FTHMC_ERR_UNSUPPORTED otherwise); gw: value and tangent
// of this layer's weight gradient
int launch_gen_fwd(const GenLayerArgsT<Dual>& a, bool rev, hipStream_t s);
int launch_gen_bwd(const GenLayerArgsT<Dual>& a, hipStream_t s);
// seeds of the backward sweeps: gp[b] = coef[b] beta sin P(x[b]) (coef NULL: 1), dual: plus its tangent coef[b] beta cos P P'
int launch_gen_seed(const double* x, const double* coef, int B, int L, double beta, double* gp, hipStream_t s);
int launch_gen_seed(const Dual* x, const double* coef, int B, int L, double beta, Dual* gp, hipStream_t s);
// x + eps g as one dual field; the link gradient (adjoint of the plaquette stencil) of the TANGENT of a dual gP field; tangents
int launch_dual_pack(const double* x, const double* g, Dual* out, size_t n, hipStream_t s);
int launch_dual_links(const Dual* gp, double* gx, int B, int L, hipStream_t s);
int launch_dual_tangent(const Dual* in, double* out, size_t n, hipStream_t s, double scale = 1.0);   // out = scale * tangent

// ---- flow_dual.hip: the default net's coupling layer on dual numbers as fused tile kernels (the force-norm training step,
// fthmc_train_force_grad): forward x -> y, and the backward from the layer's input with the tangent weight gradients
struct FlowDualArgs {
    const Dual* x;           // [B][2][L][L] layer input
    Dual* y;                 // forward: output field (not x)
    const double* wint;      // this layer's weights, kernel layout (k_pack_weights)
    const Dual* up_gp;       // backward: upstream plaquette gradient [B][L][L]
    Dual* gp_part;           // backward: [B * ntiles][window] partial plaquette gradients (launch_gather_gp_dual adds them onto up_gp)
    double* gw_part;         // backward: [flow_dual_nparts][FLOW_GW_STRIDE] tangent weight-gradient partials, canonical order
    double glogj_const;      // backward: d/d logJ
    int B, L, mu, off, act;
    int ntj, ntiles, items;  // set by the launcher
};
// tile 0: 8 x 8 sites (77.5 KB of LDS in the backward), tile 1: 8 x 16 (132 KB); either backward holds 330 / 416 registers per
// lane (256 VGPRs + accumulator registers), so ONE workgroup is resident per CU whatever the LDS would allow
inline FlowGeom flow_dual_geom(int tile) { return tile == 0 ? FlowGeom{8, 8} : FlowGeom{8, 16}; }
// served: the tile divides the lattice (L = 8: one tile whose window wraps onto itself), item and row counts in int, one
// workgroup row per chain in the small launches
inline bool flow_dual_shape(int B, int L, int tile) {
    const FlowGeom g = flow_dual_geom(tile);
    return B > 0 && B <= 65535 && L >= 8 && L <= 8192 && L % g.tr == 0 && L % g.tc == 0 && (long)B * g.ntiles(L) < (1L << 30);
}
// workgroups of the backward = rows of its partial buffer: two rounds (8 x 8) / one round (8 x 16) of the 256 CUs, fewer for small
// launches;
// workgroup k walks the items k, k + rows, ...
inline int flow_dual_nparts(int B, int L, int tile) {
    const long items = (long)B * flow_dual_geom(tile).ntiles(L), cap = tile == 0 ? 512 : 256;
    return (int)(items < cap ? items : cap);
}
inline size_t flow_dual_gp_part(int B, int L, int tile) { const FlowGeom g = flow_dual_geom(tile); return (size_t)B * g.ntiles(L) * g.n0(); }   // dual numbers
int launch_flow_dual_fwd(const FlowDualArgs& a, int tile, hipStream_t s);
int launch_flow_dual_bwd(const FlowDualArgs& a, int tile, hipStream_t s);
int launch_gather_gp_dual(const Dual* gp_part, int B, int L, int tile, Dual* gp, hipStream_t s);
// fthmc_set_dual_path: 0 the generic dual sweep (flow_generic.hip) always, 1 (default) the fused kernels where they serve the call
// (api.hip force_dual_tile picks the tile), 2 / 3 the fused kernels with 8 x 8 tiles always / 8 x 16 tiles wherever those divide
// L (the A/B of the tile shapes)
void set_dual_path(int v);
int get_dual_path();

// ---- flow_small.hip: L <= 16, one workgroup per chain, whole sequences of the flowed path in one launch
struct SmallArgs {
    const double* x;         // [B][2][L][L] latent links
    const double* v;         // leapfrog / trajectory: momenta
    const double* u;         // trajectory: accept uniforms [B]
    const double* wint;      // n_layers * FLOW_WINT, kernel weight layout
    double* stash;           // n_layers * flow_stash_doubles(B, L): the activation stash of a force evaluation
    const double* state_in;  // trajectory: [3][B] (S_eff, plaq, Q) of x, or null
    double* state_out;       // trajectory: [3][B] of x_new, or null
    double* x_out;           // action: F(x) (or null); leapfrog: x'; trajectory: x_new
    double* v_out;           // leapfrog: v'
    double* F;               // force
    double *dH, *acc, *H0, *H1, *S_eff, *logdet, *plaq, *Q;   // per chain [B], each may be null
    double *logq, *logp;     // training: [B]
    double* gz;              // training: n_layers * flow_gz_doubles(B, L): every layer's pre-activation gradients (for k_flow_wgrad)
    double beta, dt;
    int nstep, mode, B, nl, act;   // mode: 0 action (forward sweep), 1 force, 2 leapfrog, 3 trajectory, 4 training sweep
    long long* dbg;          // profiling runs: [B][32] cycles per stage, accumulated by thread 0 of each chain (else null)
};
bool ft_small_shape(int L, int n_layers);       // the fused path is built for this lattice size (default net shape, MFMA kernels)
int launch_ft_small(const SmallArgs& a, int L, hipStream_t s);
int launch_ft_small_sched(const SmallArgs& a, const Sched& sched, int L, hipStream_t s);   // mode 2 / 3 of a schedule (integrator.h)
// mode 3 of a schedule with per-chain beta beta_b[B] (replica exchange); state_in / state_out: (log det J, sum cos P, Q)
int launch_ft_small_pb(const SmallArgs& a, const Sched& sched, const double* beta_b, int L, hipStream_t s);
// mode 3 of a schedule under the bias V(Q_m) of the flowed field (metadynamics); state_in / state_out: the table-free
// [4][B] (S_eff unbiased, plaq, Q, Q_m); qm_out, vb_out (optional): Q_m and V(Q_m) of F(x_new)
int launch_ft_small_meta(const SmallArgs& a, const Sched& sched, const MetaTab& T, double* qm_out, double* vb_out, int L, hipStream_t s);
// mode 3 of a schedule with the couplings g_b on the defect df of the flowed field; state_in / state_out: the g-free
// [4][B] = (S_eff of the periodic action, plaq, Q, Dsum)
int launch_ft_small_defect(const SmallArgs& a, const Sched& sched, const double* g_b, const DefectLine& df, double* dsum_out, int L, hipStream_t s);
void set_small_path(int v);
int get_small_path();
// 0: VALU kernels everywhere; 1 (default): MFMA kernels for forward and backward-wrt-x
void set_flow_variant(int v);
int get_flow_variant();
// out[b] (+)= sign * sum_t part[b][t]
int launch_sum_parts(const double* part, int B, int nparts, double sign, int accumulate,
                     double* out, hipStream_t s, int nsets = 1);   // nsets partial sets [set][B][nparts], summed in order
// gp[b][i][j] (+)= sum of every partial window position that maps to (i, j)
int launch_gather_gp(const double* gp_part, int B, int L, FlowGeom g, int accumulate, double* gp, hipStream_t s);
// gx = gy + adj(gp)
int launch_adj_add(const double* gp, const double* gy, int B, int L, double* gx, hipStream_t s);
// gw[idx] (+)= scale * sum_p gw_part[p][idx], idx < 955
// tmp: FLOW_REDUCE_GROUPS * FLOW_GW_STRIDE doubles of scratch (two-level reduction), or null
constexpr int FLOW_REDUCE_GROUPS = 128;
// rows of tmp the two-level reduction of `nparts` partials uses per layer (0: one level, no tmp)
inline int flow_reduce_groups(int nparts) {
    if (nparts <= 64) return 0;
    int groups = (nparts + 31) / 32; if (groups > FLOW_REDUCE_GROUPS) groups = FLOW_REDUCE_GROUPS;
    const int chunk = (nparts + groups - 1) / groups;
    return (nparts + chunk - 1) / chunk;
}
int launch_reduce_gw(const double* gw_part, int nparts, double scale, int accumulate, double* gw,
                     double* tmp, hipStream_t s, int nlayers = 1, size_t part_lstride = 0);   // nlayers > 1: layer l reads gw_part + l * part_lstride, writes gw + l * 955; tmp: nlayers * flow_reduce_groups(nparts) rows

}  // namespace fthmc
