/* fthmc_hip.h -- C ABI of the MI355X (gfx950) ftHMC hot path.
 *
 * The reference (nftqcd/fthmc) is pure Python on PyTorch and has no FFI of its
 * own; each entry point below replaces the Python callable cited next to it
 * (paths relative to the reference root).  All pointers are DEVICE pointers to
 * contiguous fp64 data unless marked `host`.  Nothing here allocates or
 * synchronises: every call only enqueues kernels on `stream` (a hipStream_t
 * passed as void*; NULL = the null stream) and returns 0 or a negative
 * FTHMC_ERR_* code.  Scratch space is caller-owned (`ws`, sized by
 * fthmc_ws_bytes) so that calls can be captured into a hipGraph.  A workspace
 * belongs to one stream at a time: calls in flight on different streams (e.g.
 * two groups of independent chains) need a workspace each.
 *
 * Field layout: x[B][2][L][L], angle of the U(1) link in radians, mu-major
 * (the reference's [batch, Nd, Nt, Nx]).  L % 4 == 0, 4 <= L <= FTHMC_MAX_L,
 * 1 <= B <= FTHMC_MAX_B for every entry point that takes (B, L), and B <= FTHMC_MAX_B,
 * n_per_chain <= 2 FTHMC_MAX_L^2 for fthmc_random_momenta; beyond, FTHMC_ERR_ARG.
 * With the default net shape the flow entry points run the tuned kernels, which accept
 * less: L <= 8192 (the largest byte offset inside a stash plane, 64 L^2 - 8, fits 32
 * bits) and B <= 2^20, else FTHMC_ERR_ARG; and one layer's stash below 2^32 doubles --
 * 19 B L^2 for the force, 35 B L^2 for training -- else FTHMC_ERR_UNSUPPORTED (callers
 * split larger batches into chain groups, ops.train_grad(groups=...)).  Other net shapes
 * (fthmc_arch_t, flow_generic.hip) check no limit beyond the plain-lattice ones.
 * Flow weights: n_layers * FTHMC_W_PER_LAYER doubles; per layer the six
 * nn.Conv2d tensors of `layers[i].plaq_coupling.net` in state_dict order and
 * PyTorch [Cout][Cin][kh][kw] layout:
 *     w0[8][2][3][3] b0[8] w1[8][8][3][3] b1[8] w2[3][8][3][3] b2[3]
 * (hidden_sizes=[8,8], kernel_size=3, n_mixture_comps=2: the reference default,
 * fthmc/config.py:283-303).  Layer i uses mu = i % 2, off = (i / 2) % 4
 * (fthmc/utils/layers.py:409-412).
 */
#ifndef FTHMC_HIP_H
#define FTHMC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FTHMC_W_PER_LAYER 955
/* shape limits of the plain-lattice kernels (int site counts: 2 L^2 plus a loop stride of at
 * most 4096 below 2^31; one workgroup of up to 1024 threads per chain along x: B * 1024 < 2^32) */
#define FTHMC_MAX_L 32764
#define FTHMC_MAX_B 4194303

#define FTHMC_OK               0
#define FTHMC_ERR_ARG         -1   /* bad shape / null pointer              */
#define FTHMC_ERR_UNSUPPORTED -2   /* architecture outside the built kernels */
#define FTHMC_ERR_LAUNCH      -3   /* hipGetLastError() after a launch       */
#define FTHMC_ERR_WS          -4   /* workspace too small                    */

/* activation_fn of the s/t conv net (fthmc/utils/layers.py:117-135) */
#define FTHMC_ACT_SILU        0
#define FTHMC_ACT_RELU        1
#define FTHMC_ACT_LEAKY_RELU  2

/* trajectory modes */
#define FTHMC_MODE_MD         0   /* intended integrator, ipynb/ft_hmc.py:394-435 */
#define FTHMC_MODE_LITERAL    1   /* FieldTransformation.leapfrog as packaged, fthmc/ft_hmc.py:180-188 */

const char* fthmc_version(void);
const char* fthmc_strerror(int code);
/* text of the HIP error behind the last FTHMC_ERR_LAUNCH on this thread ("" if none) */
const char* fthmc_last_error(void);

/* Kernel variant of the coupling-layer forward / backward-wrt-x kernels: 1 (default) MFMA f64 16x16x4 implicit-GEMM
 * convolutions, 0 fp64-VALU convolutions.  Same results to rounding.  A process-wide DEBUG switch (A/B measurement and
 * cross-checks), like fthmc_set_small_path below: each entry point reads both once, when it is entered; they are the only
 * mutable state of the library and nothing a production caller touches. */
int fthmc_set_variant(int v);
int fthmc_get_variant(void);
/* Shape of the s/t conv net, an ARGUMENT of every entry point that runs the net (the reference passes it to the layer
 * constructors: make_conv_net fthmc/utils/layers.py:138-167, make_u1_equiv_layers :399-429; TrainConfig.hidden_sizes /
 * kernel_size / n_s_nets, fthmc/config.py:283-303): in_channels 2 -> hidden[0] -> ... -> hidden[n_hidden - 1] -> n_mix + 1,
 * square kernels of odd size, `n_mix` mixture components, `final_tanh` != 0: a tanh behind the last conv (make_conv_net's
 * use_final_tanh, layers.py:144,163-164; the reference passes False, :419).  NULL = the default (2, {8, 8}, 3, 2, 0) -- the reference default and
 * every BASELINE config -- which runs on the tuned kernels; any other shape runs on plain kernels (csrc/flow_generic.hip:
 * same results, one launch per operation, activations through HBM).  Weights: n_layers * fthmc_arch_params(arch) doubles,
 * per layer [w0 b0 w1 b1 ...] in PyTorch order; the workspace sizes follow the shape.  Limits: n_hidden <= 8, hidden sizes
 * <= 256, kernel_size <= 15 (and kernel_size / 2 <= L), n_mix <= 64; FTHMC_ERR_UNSUPPORTED otherwise.
 * The tuned kernels address one layer's activation stash with 32-bit element offsets: B * 19 * L * L (training: * 35)
 * must stay below 2^32 doubles (32 GiB per layer; FTHMC_ERR_UNSUPPORTED beyond -- shard the chains instead).
 * The shape is read during the call only: the library keeps no net shape between calls, two threads may run two different
 * flows on two streams at the same time. */
typedef struct fthmc_arch_t {
    int n_hidden;
    int hidden[8];
    int kernel_size;
    int n_mix;
    int final_tanh;
} fthmc_arch_t;
int fthmc_arch_params(const fthmc_arch_t* arch);   /* doubles per layer; 955 for the default */
/* Lattices of L = 8, 12, 16 take a fused path by default (csrc/flow_small.hip): one workgroup holds a whole chain in
 * LDS, and fthmc_ft_trajectory / _ft_leapfrog / _ft_force / _ft_action / _flow_forward are ONE launch each instead of
 * one launch per layer.  0 switches it off (the tiled kernels then serve every L): A/B runs and parity tests. */
int fthmc_set_small_path(int on);

/* Weight versions (the `_v` entry points below and fthmc_pack_weights).  The tuned kernels read a kernel-layout EXPANSION of
 * the canonical weights (77 KB per layer) that every entry point which runs the net writes into the head of its workspace
 * first (one launch, ~7 us; the reference packs nothing: its convs read nn.Conv2d parameters, fthmc/utils/layers.py:138-167).
 * A caller whose weights stay put between calls -- a sampler replaying a captured trajectory -- states their CONTENT VERSION
 * (any 64-bit number it changes whenever the weights' contents change; 0 = no statement): the launch then compares, on the
 * device, a token of (version, address of w, layer) with the stamp the last expansion left next to each layer's expansion
 * and expands only the layers whose stamp differs.  The library keeps no state between calls and trusts nothing: a wrong,
 * stale or reused version, another tensor, a call without a version in between (it clears the stamps it overwrites) all end
 * in an expansion, i.e. in the same numbers.  The one promise left with the caller is the meaning of the number: equal
 * version + equal address = equal contents.
 * The expansions of the first 64 layers are the HEAD of every workspace layout (fthmc_ws_head_bytes() bytes; no call of
 * any shape keeps anything else there); deeper layers are expanded by every call.  A workspace must be zero in its head
 * before its first use with a version (fresh memory may hold the stamps of an earlier life of the same address). */
size_t fthmc_ws_head_bytes(void);

/* Expand the canonical weights (n_layers x params, the layout of every `w` argument below) into the workspace under
 * `weights_version` (0: unconditionally) and do nothing else: what every entry point that runs the net does first. */
int fthmc_pack_weights(const double* w, const fthmc_arch_t* arch, int n_layers, uint64_t weights_version,
                       void* ws, size_t ws_bytes, void* stream);
int fthmc_get_small_path(void);

/* Bytes of scratch the flow / trajectory entry points need for (B, L, n_layers). */
size_t fthmc_ws_bytes(const fthmc_arch_t* arch, int B, int L, int n_layers);
/* Scratch for fthmc_train_grad (larger: the forward also stashes h1, h2 of every layer). */
size_t fthmc_train_ws_bytes(const fthmc_arch_t* arch, int B, int L, int n_layers);

/* ---- angle maps ------------------------------------------------------- */
/* out = remainder(x + pi, 2 pi) - pi.  fthmc/utils/layers.py:41-43 (torch_mod),
 * fthmc/utils/qed_helpers.py:49-50 (torch_wrap), fthmc/ft_hmc.py:173-175 (wrap). */
int fthmc_wrap(const double* x, double* out, size_t n, void* stream);
/* fthmc/utils/qed_helpers.py:40-42 (regularize) */
int fthmc_regularize(const double* x, double* out, size_t n, void* stream);

/* ---- Wilson action / plaquette / topological charge ------------------- */
/* P[b][i][j] = x0 - x1 - x0[i][j+1] + x1[i+1][j].
 * fthmc/utils/qed_helpers.py:94-105 (batch_plaqs), :80-90 (compute_u1_plaq). */
int fthmc_plaquettes(const double* x, double* P, int B, int L, void* stream);
/* S[b] = -beta sum cos P; Q[b] = sum wrap(P) / 2pi; plaq[b] = -S / (beta L^2) (formed that way on every path, tiled and
 * small-lattice alike, as the reference forms it, fthmc/hmc.py:125: at beta = 0 it is 0 / 0 = NaN there and here).
 * Any of S/Q/plaq may be NULL.  fthmc/utils/qed_helpers.py:177-186 (BatchAction),
 * :108-116 (batch_charges), fthmc/hmc.py:125 (plaq). */
int fthmc_wilson_action_charge(const double* x, int B, int L, double beta,
                               double* S, double* Q, double* plaq, void* stream);
/* F = dS/dx.  fthmc/utils/qed_helpers.py:265-272 (force, via autograd there). */
int fthmc_wilson_force(const double* x, int B, int L, double beta, double* F, void* stream);

/* ---- plain HMC --------------------------------------------------------- */
/* x_, p_ = leapfrog(x, p): fthmc/utils/qed_helpers.py:275-295.  x_out/p_out must
 * not alias x/p.  ws: fthmc_ws_bytes(NULL, B, L, 0). */
int fthmc_leapfrog(const double* x, const double* p, int B, int L, double beta,
                   double dt, int nstep, double* x_out, double* p_out,
                   void* ws, size_t ws_bytes, void* stream);
/* K[b] = sum_b v^2 (no 1/2).  Used for H = S + K/2 (qed_helpers.py:301) */
int fthmc_kinetic(const double* v, int B, int L, double* K, void* stream);
/* Run statistics of one trajectory (the per-trajectory metrics of fthmc/ft_hmc.py:266-270, 311-331 and hmc.py:118-149) folded
 * into running sums on the device: vec8[0..7] += sum over the B chains of (1, acc, plaq, Q, Q^2, |Q - qold|, dH, exp(-dH)),
 * then qold <- Q.  One launch, fixed summation order. */
int fthmc_stats_accumulate(const double* acc, const double* plaq, const double* Q, double* qold, const double* dH, int B,
                           double* vec8, void* stream);
/* One trajectory per chain with supplied momenta v[B][2][L][L] and uniforms u[B]:
 * H0 = S(x) + v^2/2; leapfrog; xr = regularize(x_); dH = H1 - H0;
 * acc = u < exp(-dH); x_new = acc ? xr : x.   fthmc/utils/qed_helpers.py:298-311
 * (there the whole tensor is one system; chains are independent here, identical
 * for B = 1).  Outputs dH[B], acc[B] (0.0 / 1.0); H0/H1 may be NULL. */
int fthmc_hmc_trajectory(const double* x, const double* v, const double* u,
                         int B, int L, double beta, double dt, int nstep,
                         double* x_new, double* dH, double* acc, double* H0, double* H1,
                         void* ws, size_t ws_bytes, void* stream);

/* Momentum refresh for the production path: v[b][0..n) ~ N(0,1), u[b] ~ U[0,1) from a
 * Philox4x32-10 stream keyed by seeds[b] (device int64[B]).  Replaces torch.randn_like /
 * torch.rand of fthmc/utils/qed_helpers.py:300,306 and fthmc/ft_hmc.py:204,212; a chain's
 * draws depend only on its seed, so sharding chains over GPUs does not change them.
 * u may be NULL. */
int fthmc_random_momenta(const int64_t* seeds, int B, int n_per_chain, double* v, double* u,
                         void* stream);

/* ---- coupling layers ---------------------------------------------------- */
/* (y, logJ[B]) = GaugeEquivCouplingLayer.forward(x): fthmc/utils/layers.py:196-202
 * with NCPPlaqCouplingLayer.forward :348-371.  w: one layer (955 doubles).
 * y may alias x. */
int fthmc_flow_layer_fwd(const double* x, const double* w, const fthmc_arch_t* arch, int B, int L, int mu, int off,
                         int act, double* y, double* logJ,
                         void* ws, size_t ws_bytes, void* stream);
/* VJP of the layer wrt x: gx = d/dx [ sum(gy * y) + sum_b glogJ[b] logJ[b] ]
 * (what autograd does for fthmc/utils/qed_helpers.py:226-242 and train.py:210).
 * gw != NULL additionally returns the same VJP wrt the 955 weights; the workspace must then hold
 * fthmc_train_ws_bytes(arch, B, L, 1). */
int fthmc_flow_layer_bwd(const double* x, const double* w, const fthmc_arch_t* arch, const double* gy, const double* glogJ,
                         int B, int L, int mu, int off, int act,
                         double* gx, double* gw,
                         void* ws, size_t ws_bytes, void* stream);
/* The same pair for callers that keep a layer's activations between its forward and its backward (an autograd graph:
 * fthmc/utils/layers.py:196-202 under loss.backward(), train.py:210): the forward also fills `stash`
 * (fthmc_layer_stash_bytes(arch, B, L) bytes, caller-owned), the backward reads it and recomputes nothing.
 * fthmc_layer_stash_bytes is 0 where no stash exists (fthmc_set_variant(0)): use fthmc_flow_layer_bwd there. */
size_t fthmc_layer_stash_bytes(const fthmc_arch_t* arch, int B, int L);
int fthmc_flow_layer_fwd_stash(const double* x, const double* w, const fthmc_arch_t* arch, int B, int L, int mu, int off, int act,
                               double* y, double* logJ, double* stash, void* ws, size_t ws_bytes, void* stream);
int fthmc_flow_layer_bwd_stash(const double* stash, const double* w, const fthmc_arch_t* arch, const double* gy, const double* glogJ,
                               int B, int L, int mu, int off, int act, double* gx, double* gw,
                               void* ws, size_t ws_bytes, void* stream);
/* (x, logJ[B]) = GaugeEquivCouplingLayer.reverse(y): fthmc/utils/layers.py:204-210,
 * :373-396.  The scalar inverse is solved per site to |f(x) - y| <= tol by
 * safeguarded Newton/bisection on [-pi, pi] (the reference bisects to a global
 * 1e-6, layers.py:294-320).  x may alias y (a layer rewrites only its active links, and every
 * plaquette a workgroup uses is built from links the layer leaves alone plus its own). */
int fthmc_flow_layer_rev(const double* y, const double* w, const fthmc_arch_t* arch, int B, int L, int mu, int off,
                         int act, double tol, double* x, double* logJ,
                         void* ws, size_t ws_bytes, void* stream);

/* Plaquette-level coupling map on a plaquette field P[B][L][L] (no links involved):
 * (fP, logJ[B]) = NCPPlaqCouplingLayer.forward(P): fthmc/utils/layers.py:348-371 -- P' at the active
 * plaquettes, P at the frozen and passive ones; and its inverse NCPPlaqCouplingLayer.reverse(fP):
 * fthmc/utils/layers.py:373-396 (logJ of the inverse = -sum log dP'/dP; `tol` as fthmc_flow_layer_rev).
 * Served by the MFMA kernels only (FTHMC_ERR_UNSUPPORTED with fthmc_set_variant(0)).  logJ may be NULL. */
int fthmc_plaq_coupling_fwd(const double* P, const double* w, const fthmc_arch_t* arch, int B, int L, int mu, int off, int act,
                            double* fP, double* logJ, void* ws, size_t ws_bytes, void* stream);
int fthmc_plaq_coupling_rev(const double* fP, const double* w, const fthmc_arch_t* arch, int B, int L, int mu, int off, int act,
                            double tol, double* P, double* logJ, void* ws, size_t ws_bytes, void* stream);
/* VJP of fthmc_plaq_coupling_fwd (autograd through NCPPlaqCouplingLayer.forward, layers.py:348-371, on a plaquette field):
 * gP = d/dP [ sum(gfP * fP) + sum_b glogJ[b] logJ[b] ]; gw != NULL additionally the same wrt the layer's weights (the workspace
 * must then hold fthmc_train_ws_bytes(arch, B, L, 1)).  The layer is run forward once inside. */
int fthmc_plaq_coupling_bwd(const double* P, const double* w, const fthmc_arch_t* arch, const double* gfP, const double* glogJ,
                            int B, int L, int mu, int off, int act, double* gP, double* gw,
                            void* ws, size_t ws_bytes, void* stream);

/* ---- whole flow ---------------------------------------------------------- */
/* Each entry point of this section has a `_v` twin with a trailing `weights_version` (see "Weight versions" above);
 * the plain form is the twin with version 0. */
/* y = F(x), logdet[B] = sum_l logJ_l.  fthmc/ft_hmc.py:143-150 (flow_forward),
 * fthmc/utils/qed_helpers.py:191-198 (ft_flow).  y, logdet may be NULL. */
int fthmc_flow_forward(const double* x, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L, int act,
                       double* y, double* logdet, void* ws, size_t ws_bytes, void* stream);
int fthmc_flow_forward_v(const double* x, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L, int act,
                       double* y, double* logdet, void* ws, size_t ws_bytes, void* stream, uint64_t weights_version);
/* x = F^-1(y), logdet[B].  fthmc/ft_hmc.py:152-160, qed_helpers.py:201-209.  x may alias y: the last layer maps
 * y -> x and the remaining layers run in place on x (see fthmc_flow_layer_rev). */
int fthmc_flow_reverse(const double* y, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L, int act,
                       double tol, double* x, double* logdet,
                       void* ws, size_t ws_bytes, void* stream);
int fthmc_flow_reverse_v(const double* y, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L, int act,
                       double tol, double* x, double* logdet,
                       void* ws, size_t ws_bytes, void* stream, uint64_t weights_version);
/* S_eff[b] = S_W(F(x)) - logdet.  fthmc/utils/qed_helpers.py:212-223 (ft_action),
 * fthmc/ft_hmc.py:135-141.  Optional outputs (NULL to skip): logdet[B],
 * plaq[B], Q[B] of the physical field F(x). */
int fthmc_ft_action(const double* x, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L, int act,
                    double beta, double* S_eff, double* logdet, double* plaq, double* Q,
                    void* ws, size_t ws_bytes, void* stream);
int fthmc_ft_action_v(const double* x, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L, int act,
                    double beta, double* S_eff, double* logdet, double* plaq, double* Q,
                    void* ws, size_t ws_bytes, void* stream, uint64_t weights_version);
/* F = d(sum_b S_eff)/dx.  fthmc/utils/qed_helpers.py:226-242 (ft_force),
 * fthmc/ft_hmc.py:162-171. */
int fthmc_ft_force(const double* x, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L, int act,
                   double beta, double* F, void* ws, size_t ws_bytes, void* stream);
int fthmc_ft_force_v(const double* x, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L, int act,
                   double beta, double* F, void* ws, size_t ws_bytes, void* stream, uint64_t weights_version);
/* Second order: the vector-Jacobian products autograd takes through ft_action / ft_force.  Every net shape, the default one
 * included, runs on the plain kernels (csrc/flow_generic.hip; the force VJP on their dual-number instances, csrc/dual.h),
 * reductions in a fixed order: the same inputs give the same bits, whatever fthmc_set_variant / fthmc_set_small_path say.
 * Shape limits: those of the plain kernels (n_layers = 0 allowed).  gx[B][2][L][L], gw[n_layers * fthmc_arch_params(arch)]:
 * either may be NULL (not wanted), not both.  ws: fthmc_vjp_ws_bytes(arch, B, L, n_layers); its first fthmc_ws_head_bytes()
 * bytes (the weight expansions of the other entry points) are never written.
 *
 * gx, gw = d/dx, d/dw of sum_b [ gS[b] S_eff[b] + glogdet[b] logdet[b] ]   (glogdet NULL = 0)
 * autograd of fthmc/utils/qed_helpers.py:212-223 (ft_action), fthmc/ft_hmc.py:135-141 */
int fthmc_ft_action_vjp(const double* x, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L, int act,
                        double beta, const double* gS, const double* glogdet, double* gx, double* gw,
                        void* ws, size_t ws_bytes, void* stream);
/* with F = d(sum_b S_eff)/dx (fthmc_ft_force) and a cotangent g[B][2][L][L]: gx = (dF/dx)^T g = H g, gw = d/dw <g, F>
 * autograd of fthmc/utils/qed_helpers.py:226-242 with create_graph=True (the reference's force is
 * torch.autograd.grad(ft_action(x).sum(), x, create_graph=...)); n_layers = 0: the Hessian of the Wilson action */
int fthmc_ft_force_vjp(const double* x, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L, int act,
                       double beta, const double* g, double* gx, double* gw, void* ws, size_t ws_bytes, void* stream);
/* Scratch for the two calls above (0 for a refused shape). */
size_t fthmc_vjp_ws_bytes(const fthmc_arch_t* arch, int B, int L, int n_layers);
/* Force-norm training (TrainConfig.with_force): the loss sum_b |F_b|^2 of the flowed force F = d(sum_b S_eff)/dx at a fixed x and
 * its gradient with respect to the weights, in one call.  ipynb/ft_hmc.py:253-299 (force = ft_force(param, layers, xi, True);
 * loss = sum(force**2); loss.backward()).
 *   F[B][2][L][L]  the first-order force, from the sweep fthmc_ft_force runs under the current switches (NULL: not wanted)
 *   force_sq[B]    sum over the links of F_b^2, fixed order
 *   gw             d(sum_b force_sq[b])/dw, n_layers x fthmc_arch_params(arch) in the canonical layout (NULL: the metrics-only
 *                  call); = twice the tangent weight gradient of the force sweep on the dual field x + eps F (csrc/dual.h)
 * The dual sweep of the default net runs on fused tile kernels (csrc/flow_dual.hip) where 8 x 8 tiles divide the lattice
 * (L % 8 == 0), and on the plain dual kernels of fthmc_ft_force_vjp everywhere else: same results to rounding, fixed summation
 * order either way.  n_layers = 0: the Wilson force, gw untouched.  ws: fthmc_train_force_ws_bytes(arch, B, L, n_layers), which
 * is a workspace of fthmc_ft_force (head included: the first-order sweep expands the weights there) with the dual regions behind
 * it; the size covers the path the current fthmc_set_dual_path setting selects and is 0 for a refused shape. */
size_t fthmc_train_force_ws_bytes(const fthmc_arch_t* arch, int B, int L, int n_layers);   /* ipynb/ft_hmc.py:253-299 */
int fthmc_train_force_grad(const double* xi, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L,
                           int act, double beta, double* F, double* force_sq, double* gw,
                           void* ws, size_t ws_bytes, void* stream);                         /* ipynb/ft_hmc.py:253-299 */
/* Which dual sweep serves fthmc_train_force_grad (ipynb/ft_hmc.py:253-299): 1 (default) the fused kernels where they are built
 * for the shape (8 x 16 tiles where they divide L and fill the chip, else 8 x 8), 0 the plain dual kernels always, 2 / 3 the
 * fused kernels with 8 x 8 tiles always / 8 x 16 tiles wherever those divide L (tile A/B).  A process-wide DEBUG switch like
 * fthmc_set_small_path, read once per call. */
int fthmc_set_dual_path(int on);
int fthmc_get_dual_path(void);
/* 1 if the fused dual kernels serve a fthmc_train_force_grad call of this shape under the current setting, 0 if the plain
 * dual kernels do, < 0 for a refused arch */
int fthmc_train_force_path(const fthmc_arch_t* arch, int B, int L);
/* x_, v_ = leapfrog with ft_force.  ipynb/ft_hmc.py:394-418. */
int fthmc_ft_leapfrog(const double* x, const double* v, const double* w, const fthmc_arch_t* arch, int n_layers,
                      int B, int L, int act, double beta, double dt, int nstep,
                      double* x_out, double* v_out, void* ws, size_t ws_bytes, void* stream);
int fthmc_ft_leapfrog_v(const double* x, const double* v, const double* w, const fthmc_arch_t* arch, int n_layers,
                      int B, int L, int act, double beta, double dt, int nstep,
                      double* x_out, double* v_out, void* ws, size_t ws_bytes, void* stream, uint64_t weights_version);
/* One ftHMC trajectory per chain in the latent field x with supplied v, u[B].
 * mode FTHMC_MODE_MD: ipynb/ft_hmc.py:420-435 without the flow-inverse wrapper;
 * FTHMC_MODE_LITERAL: fthmc/ft_hmc.py:190-224 as packaged.
 * Outputs: x_new (latent), dH[B], acc[B] (0/1), and plaq[B], Q[B] of F(x_new)
 * (fthmc/ft_hmc.py:266-270, 311-313); H0/H1/plaq/Q may be NULL.
 * Chaining: state_out[3][B] (nullable) receives [S_eff, plaq, Q] of x_new; passing it back as
 * state_in of the next call (x = this x_new) skips the H0 flow sweep, which would recompute
 * exactly these numbers (the reference recomputes, ft_hmc.py:205).  state_in NULL = stateless. */
int fthmc_ft_trajectory(const double* x, const double* v, const double* u, const double* w, const fthmc_arch_t* arch,
                        int n_layers, int B, int L, int act, double beta, double dt, int nstep,
                        int mode, double* x_new, double* dH, double* acc,
                        double* H0, double* H1, double* plaq, double* Q,
                        const double* state_in, double* state_out,
                        void* ws, size_t ws_bytes, void* stream);
int fthmc_ft_trajectory_v(const double* x, const double* v, const double* u, const double* w, const fthmc_arch_t* arch,
                        int n_layers, int B, int L, int act, double beta, double dt, int nstep,
                        int mode, double* x_new, double* dH, double* acc,
                        double* H0, double* H1, double* plaq, double* Q,
                        const double* state_in, double* state_out,
                        void* ws, size_t ws_bytes, void* stream, uint64_t weights_version);

/* ---- MD integrators ------------------------------------------------------ */
/* The MD of a trajectory as a schedule (csrc/integrator.h): an initial drift x += b0 v, then stages, each one force evaluation;
 * g = the gradient of the action (what the kicks subtract):
 *   KICK(a, b):  v -= a g(x*); x += b v     (x* = x, or the shifted field if a SHIFT stage came just before)
 *   SHIFT(c):    x~ = x - c g(x)            (the next stage evaluates g at x~; x and v are untouched)
 * FTHMC_INT_LEAPFROG:        b0 = dt/2; nstep x KICK(dt, dt), the last b = dt/2                              nstep forces
 * FTHMC_INT_OMELYAN:         2nd-order minimum norm, position version, lambda = 0.1931833275037836: b0 = lambda dt; per step
 *                            KICK(dt/2, (1 - 2 lambda) dt), KICK(dt/2, 2 lambda dt); the very last b = lambda dt     2 nstep forces
 * FTHMC_INT_FORCE_GRADIENT:  4th order, B A B_FG A B with the end kicks of neighbouring steps merged and the force-gradient
 *                            term as one shifted re-evaluation of the force: b0 = 0; KICK(dt/6, dt/2); per step
 *                            SHIFT(dt^2/24), KICK(2dt/3, dt/2); between steps KICK(dt/3, dt/2); last KICK(dt/6, 0)   3 nstep + 1 forces */
#define FTHMC_INT_LEAPFROG        0
#define FTHMC_INT_OMELYAN         1
#define FTHMC_INT_FORCE_GRADIENT  2
#define FTHMC_STAGE_KICK          0
#define FTHMC_STAGE_SHIFT         1
/* Host only.  Force evaluations (= stages) per trajectory; -2 for an unknown integrator, -1 for nstep < 1 (or a count beyond int). */
int fthmc_integrator_forces(int integrator, int nstep);
/* Host only.  The expanded schedule: *b0 and kind[i], a[i], b[i] of stage i (a SHIFT stage: a = c, b = 0); `cap` = length of the
 * arrays.  Returns the number of stages; fthmc_integrator_forces' codes, or -3 if cap is too small or a pointer is null -- nothing
 * is written then. */
int fthmc_integrator_schedule(int integrator, double dt, int nstep, double* b0, int* kind, double* a, double* b, int cap);
/* fthmc_leapfrog / fthmc_hmc_trajectory with the integrator as an argument.  FTHMC_INT_LEAPFROG delegates to them (bit-identical);
 * an unknown integrator: FTHMC_ERR_UNSUPPORTED.  ws as theirs. */
int fthmc_md(const double* x, const double* p, int B, int L, double beta, double dt, int nstep, int integrator,
             double* x_out, double* p_out, void* ws, size_t ws_bytes, void* stream);
int fthmc_hmc_trajectory_int(const double* x, const double* v, const double* u, int B, int L, double beta, double dt, int nstep,
                             int integrator, double* x_new, double* dH, double* acc, double* H0, double* H1,
                             void* ws, size_t ws_bytes, void* stream);
/* fthmc_ft_leapfrog_v / fthmc_ft_trajectory_v with the integrator as an argument (before weights_version).  FTHMC_INT_LEAPFROG
 * delegates to them (bit-identical); FTHMC_MODE_LITERAL with another integrator (that mode discards the MD) and an unknown
 * integrator: FTHMC_ERR_UNSUPPORTED.  ws as theirs: fthmc_ws_bytes. */
int fthmc_ft_md_v(const double* x, const double* v, const double* w, const fthmc_arch_t* arch, int n_layers,
                  int B, int L, int act, double beta, double dt, int nstep,
                  double* x_out, double* v_out, void* ws, size_t ws_bytes, void* stream, int integrator, uint64_t weights_version);
int fthmc_ft_trajectory_int_v(const double* x, const double* v, const double* u, const double* w, const fthmc_arch_t* arch,
                              int n_layers, int B, int L, int act, double beta, double dt, int nstep,
                              int mode, double* x_new, double* dH, double* acc,
                              double* H0, double* H1, double* plaq, double* Q,
                              const double* state_in, double* state_out,
                              void* ws, size_t ws_bytes, void* stream, int integrator, uint64_t weights_version);

/* ---- Per-chain beta and replica exchange (parallel tempering).  The reference has no counterpart, as for the integrators: it
 * samples one beta per run.  B = M K chains form M ladders of K consecutive chains; beta_b[B] (device) holds every chain's beta.
 *
 * fthmc_ft_trajectory_pb_v generalises fthmc_ft_trajectory_int_v: the device array beta_b in place of `double beta`, FTHMC_MODE_MD
 * only (another mode: FTHMC_ERR_UNSUPPORTED), every integrator, every branch of the scalar call (the one-launch kernel of the small
 * lattices, the tuned kernels, other net shapes / the VALU variant / ragged lattices / n_layers = 0).  With a constant beta_b its
 * x_new, dH, acc, H0, H1, plaq, Q are those of the scalar call.  The carried state is BETA-FREE:
 *     state[3][B] = (log det J, C = sum cos P, Q) of the accepted field,
 * from which a call forms S_W = (-beta_b[b]) C, S_eff = S_W - log det J and plaq = (-S_W) / (beta_b[b] L^2) -- so a chained call
 * equals a stateless one at ANY beta_b, and an exchange of betas between two chains leaves the state valid.  ws: fthmc_ws_bytes.
 * fthmc_hmc_trajectory_pb generalises fthmc_hmc_trajectory_int in the same way (plain HMC; no state). */
int fthmc_ft_trajectory_pb_v(const double* x, const double* v, const double* u, const double* w, const fthmc_arch_t* arch,
                             int n_layers, int B, int L, int act, const double* beta_b, double dt, int nstep,
                             int mode, double* x_new, double* dH, double* acc,
                             double* H0, double* H1, double* plaq, double* Q,
                             const double* state_in, double* state_out,
                             void* ws, size_t ws_bytes, void* stream, int integrator, uint64_t weights_version);
int fthmc_hmc_trajectory_pb(const double* x, const double* v, const double* u, int B, int L, const double* beta_b, double dt, int nstep,
                            int integrator, double* x_new, double* dH, double* acc, double* H0, double* H1,
                            void* ws, size_t ws_bytes, void* stream);
/* One round of replica exchange.  betas[K]: the ladder, strictly increasing; rung[B]: the rung of every chain; chain_of[B]: per
 * ladder, the chain (its index INSIDE the ladder, 0 .. K - 1) on every rung -- the inverse of rung within the ladder.  For every
 * ladder m and every k = parity (mod 2), k + 1 < K: a = chain on rung k, c = chain on rung k + 1,
 *     d = (beta_k - beta_{k+1}) (C[c] - C[a]);   accept iff u[m (K - 1) + k] < exp(d)
 * with C[B] = sum cos P of the chains' (flowed) fields, row 1 of the beta-free state: all rungs share ONE flow, so the log det J
 * terms of the exact ratio cancel.  An accepted pair exchanges its rung, beta_b and chain_of entries; fields never move.
 * Optional outputs [M][K - 1]: swap_acc = 1 / 0, or -1 for a pair not attempted in this round; d (0 where not attempted).  The pairs
 * of a round are disjoint: no atomics, two calls give the same bits.  u[M][K - 1]: uniforms on [0, 1), an input as for a trajectory.
 * K < 2, M < 1, K M > FTHMC_MAX_B, parity not 0 / 1, a null pointer: FTHMC_ERR_ARG. */
int fthmc_replica_swap(const double* betas, int K, int M, int parity, const double* C, const double* u, double* beta_b, int32_t* rung,
                       int32_t* chain_of, double* swap_acc, double* d, void* stream);
/* Every ladder in order: betas <- betas_host (host, K doubles, read DURING the call: they travel in kernel arguments, so the call
 * only enqueues, can be captured, and the host array may be freed when it returns), and for chain b = m K + k: beta_b = betas[k],
 * rung = k, chain_of = k.  A ladder that is not strictly increasing: FTHMC_ERR_ARG; sizes and pointers as fthmc_replica_swap. */
int fthmc_ladder_init(const double* betas_host, int K, int M, double* betas, double* beta_b, int32_t* rung, int32_t* chain_of,
                      void* stream);

/* ---- Wilson loops and Polyakov-loop correlators.  The reference has no counterpart, as for the integrators and the ladder: its
 * only gauge-invariant observables are the plaquette and the charge.  With indices mod L, the loop with corner (i, j), extent R
 * along i and T along j has the angle
 *     theta = sum_{a<R} x0[i+a][j] + sum_{c<T} x1[i+R][j+c] - sum_{a<R} x0[i+a][j+T] - sum_{c<T} x1[i][j+c]
 * and W[b][R-1][T-1] = (1 / L^2) sum_{i,j} cos theta, 1 <= R <= Rmax, 1 <= T <= Tmax: R = T = 1 is the mean of cos P with P as
 * fthmc_plaquettes forms it; the column T = L is the Polyakov-loop correlator < P(i) P*(i + R) >, P(i) = exp(i sum_j x1[i][j]);
 * W(L, L) = 1.  Wmean[Rmax][Tmax] (optional): the mean over the chains, added in index order.  fp64 throughout; no atomics: two
 * calls give the same bits.  Enqueue-only, capturable, no allocation: ws holds fthmc_wilson_loops_ws_bytes(B, L, Rmax, Tmax) bytes
 * (0 for a refused shape or a size beyond size_t).  Null x / W, B or L out of range, Rmax or Tmax outside [1, L]: FTHMC_ERR_ARG; a
 * short (or null) workspace: FTHMC_ERR_WS. */
size_t fthmc_wilson_loops_ws_bytes(int B, int L, int Rmax, int Tmax);
int fthmc_wilson_loops(const double* x, int B, int L, int Rmax, int Tmax, double* W /* [B][Rmax][Tmax] */,
                       double* Wmean /* [Rmax][Tmax] or NULL */, void* ws, size_t ws_bytes, void* stream);

/* ---- Local updates: heatbath and overrelaxation sweeps of the plain Wilson action.  The reference has no counterpart: it updates
 * by molecular dynamics only.  With P(i,j) = x0[i][j] + x1[i+1][j] - x0[i][j+1] - x1[i][j] a link sits in two plaquettes and its
 * conditional weight is exp(kappa cos(x - phi)), kappa = beta |A|, phi = -arg A, A = exp(i a) + exp(-i b) with
 *     x0[i][j]:  a = x1[i+1][j] - x0[i][j+1] - x1[i][j],          b = x0[i][j-1] + x1[i+1][j-1] - x1[i][j-1]
 *     x1[i][j]:  a = -(x0[i][j] + x1[i+1][j] - x0[i][j+1]),       b = -(x0[i-1][j] - x0[i-1][j+1] - x1[i-1][j])
 * i.e. kappa = 2 beta |cos((a + b) / 2)|, phi = (b - a) / 2 (+ pi where that cosine is negative).  The four classes (mu, parity) --
 * x0 links by the parity of j, x1 links by the parity of i -- are updated in place in the order (0,0), (0,1), (1,0), (1,1);
 * `classes` is the mask of those a sweep touches (bit 2 mu + parity; 15 = a full sweep), every other link is copied.
 *   overrelaxation: x <- regularize(2 phi - x) = regularize((b - a) - x): the link's two plaquettes exchange their angles, the
 *     action is unchanged, nothing is drawn;
 *   heatbath: x <- regularize(phi +- acos f) by Best-Fisher rejection for the von Mises distribution: at most 64 attempts (a link
 *     that uses them up, probability < 1e-30, keeps its value); kappa < 2^-60 takes the algorithm's limit, the uniform draw f = z.
 * The call runs nsweep compound sweeps, each n_hb heatbath sweeps followed by n_or overrelaxation sweeps.  Attempt t of the link
 * (mu, i, j) in heatbath sweep k = sweep0 + (compound sweep) n_hb + (heatbath sweep inside it) reads the Philox4x32-10 block at
 * counter (i L + j, k, 3, mu << 8 | t) under the key of seeds[b]: u1 from words (0, 1), u2 from words (2, 3), the sign of the
 * angle from bit 0 of word 1.  A link's draws depend on nothing else: nsweep = 2 equals two calls with sweep0, sweep0 + n_hb; a
 * full sweep equals its four classes one call each; chain b of a batch equals the chain alone; fthmc_set_small_path(0 / 1)
 * (one launch per class / the whole call in one launch with the chain's links in LDS, L <= 64) gives the same bits.
 * beta_b (nullable): per-chain beta [B], read in place of `beta`.  x_out may be x.  Enqueue-only, capturable, no workspace.
 * A null x / x_out (seeds: with n_hb > 0), B or L out of range, a negative count or sweep0, classes outside 1 .. 15, or
 * sweep0 + nsweep n_hb > 2^32: FTHMC_ERR_ARG. */
int fthmc_local_update(const double* x, int B, int L, double beta, const double* beta_b, const int64_t* seeds, int n_hb, int n_or,
                       int nsweep, int64_t sweep0, int classes, double* x_out, void* stream);

/* ---- Annealed importance sampling: a ramp of beta through the local updates above, with the Jarzynski work of every chain.  The
 * reference has no counterpart.  betas: a DEVICE array [n_step + 1].  With x_0 = x and W = work_in[b] (NULL: 0), step
 * k = 0 .. n_step - 1 of chain b is
 *     C_k = sum_{i,j} cos P(x_k),   P = ((x0[i][j] + x1[i+1][j]) - x0[i][j+1]) - x1[i][j]   (the order of the roundings),
 *     W  <- W + (betas[k] - betas[k+1]) C_k     (the difference, the product and the sum each rounded: no fused multiply-add),
 *     x_{k+1} = x_k after nsweep compound sweeps (n_hb heatbath, then n_or overrelaxation) at betas[k+1], all four classes, with the
 *               heatbath-sweep indices of fthmc_local_update(..., nsweep, sweep0 + k nsweep n_hb, 15, ...).
 * x_out = x_{n_step}, work_out[b] = W, and c_trace[b][k] = C_k for k = 0 .. n_step (optional; the last entry is the sum of the final
 * field).  exp(-W) is the importance weight of x_out as a sample of exp(betas[n_step] sum cos P) when x was drawn from
 * exp(betas[0] sum cos P) (Jarzynski: < exp(-W) > = Z(betas[n_step]) / Z(betas[0])).  C_k is added in a fixed order: thread t of the
 * chain's nt = min(1024, L^2 / 2 rounded up to 64) threads adds the sites t, t + nt, ... from 0.0, the 64 lanes of a wave by the xor
 * butterfly, the waves in order.  Inside the one-launch kernel a chain's work stays in registers and is stored once.
 *   * The fields are bit for bit those of the chain of fthmc_local_update calls above; they do not depend on work_in, c_trace or path.
 *   * A ramp cut at any step m equals two calls, the second with betas + m, work_in = the first's work_out and
 *     sweep0 + m nsweep n_hb: the same bits in the fields, the work and the trace.  Chain b of a batch equals the chain alone.
 *   * x_out may be x, work_out may be work_in.  n_step = 0 copies the field, copies the work and writes C_0.
 *   * betas is read on the device: the call only enqueues, can be captured, and a replay follows the schedule the array holds then.
 *     Finite betas >= 0 are the caller's promise (they are not looked at on the host).
 * path: 1 = the whole ramp in one launch, one workgroup per chain with the chain's links in LDS, L <= 64; 2 = sequenced: per step
 * one work kernel, then the class kernels, any L; 0 = as fthmc_local_update chooses (fthmc_set_small_path).  For L <= 64 both give
 * the same bits in every output.  No workspace, no hidden state.
 * A null x / x_out / betas / work_out (seeds: with n_hb > 0), B or L out of range, a negative count or sweep0, n_hb + n_or = 0 with
 * n_step > 0, n_step > 65536, path outside 0 .. 2, path 1 with L > 64, or sweep0 + n_step nsweep n_hb > 2^32: FTHMC_ERR_ARG. */
int fthmc_anneal(const double* x, int B, int L, const double* betas /* device [n_step + 1] */, int n_step, const int64_t* seeds, int n_hb,
                 int n_or, int nsweep, int64_t sweep0, int path, const double* work_in /* [B] or NULL = 0 */, double* x_out,
                 double* work_out /* [B] */, double* c_trace /* [B][n_step + 1] or NULL */, void* stream);

/* ---- Instanton hits: a Metropolis update of the plain Wilson action across topological sectors.  The reference has no counterpart:
 * it updates by leapfrog molecular dynamics only.  With A the constant-field-strength configuration of charge 1,
 *     A1[i][j] = (2 pi / L^2) i,      A0[L-1][j] = -(2 pi / L) j,      A0[i][j] = 0 for i < L - 1,
 * x + k A moves every plaquette by k w, w = 2 pi / L^2 (the one at (L-1, L-1) by k w - 2 pi k).  A call runs n_hit Metropolis steps
 * in the net charge k, from k = 0, and applies the k it ends with.  Step h = 0 .. n_hit - 1 of chain b reads the Philox4x32-10 block
 * at counter (hit0 + h, 0, 4, 0) under the key of seeds[b]: u = 1 - u53(words 0, 1) in [0, 1), s = +1 where bit 0 of word 2 is set,
 * else -1; it accepts k -> k + s iff u < exp(-dS),
 *     dS = 2 beta s sin(pi / L^2) [C sin theta + Sn cos theta],      theta = ((2 k + s) mod 2 L^2) pi / L^2,
 * where C = sum cos P and Sn = sum sin P are the sums of the field the call RECEIVED, P(i,j) = x0[i][j] + x1[i+1][j] - x0[i][j+1] -
 * x1[i][j] (they are not reduced again inside a call).  The net charge is applied as
 *     x1[i][j]   <- regularize(x1[i][j]   + 2 pi ((k i) mod L^2) / L^2)
 *     x0[L-1][j] <- regularize(x0[L-1][j] - 2 pi ((k j) mod L) / L)
 * with the mathematical (non-negative) remainder in 64-bit integers: a shift lies in [0, 2 pi) whatever k, and a link whose reduced
 * integer is 0 -- all of x0 above its last row, row 0 of x1, column 0 of the last row of x0, everything when k = 0 -- is copied bit
 * for bit.  beta_b (nullable): per-chain beta [B], read in place of `beta`.  Outputs (each nullable): k_out[B] the applied charge,
 * nacc_out[B] the accepted steps, cs_out[B][2] = (C, Sn).  x_out may be x.  n_hit = 0 copies the field and writes k = nacc = 0.
 * path: 1 = one workgroup per chain, the whole call in one launch, no workspace; 2 = a few chains of a large lattice: one wave per
 * workgroup for the sums, a decision kernel, an apply kernel, workspace fthmc_instanton_ws_bytes; 0 = the library chooses: 2 when
 * B < 64 and L >= 128, else 1.  Both give the same bits in every output; chain b of a batch equals the chain alone.
 * fthmc_instanton_ws_bytes is 0 where the path that (B, L, path) selects needs no workspace (and for refused arguments), else
 * a multiple of 256 bytes like every workspace size of this header.
 * Enqueue-only, capturable.  A null x / x_out (seeds: with n_hit > 0), B or L out of range, n_hit outside 0 .. 1024, hit0 < 0 or
 * hit0 + n_hit > 2^32, path outside 0 .. 2: FTHMC_ERR_ARG; a short (or null) workspace where one is needed: FTHMC_ERR_WS. */
size_t fthmc_instanton_ws_bytes(int B, int L, int path);
int fthmc_instanton_hit(const double* x, int B, int L, double beta, const double* beta_b, const int64_t* seeds, int n_hit, int64_t hit0,
                        int path, double* x_out, int32_t* k_out /* [B] or NULL */, int32_t* nacc_out /* [B] or NULL */,
                        double* cs_out /* [B][2] or NULL */, void* ws, size_t ws_bytes, void* stream);

/* ---- Metadynamics HMC: plain HMC under a history-dependent bias potential V(Q_m) in the continuous charge
 *     Q_m(x) = (1 / 2 pi) sum sin P,      P(i,j) = x0[i][j] + x1[i+1][j] - x0[i][j+1] - x1[i][j].
 * The reference has no counterpart to any of the five entry points below: it samples the unbiased action only.
 * The table vtab[G][nb] (device doubles) holds V on the nodes q_i = -qmax + i delta, delta = 2 qmax / (nb - 1); chain b reads row
 * b / (B / G): G = 1 one potential for all walkers, G = B one per chain.  Lookup at q: t = (q + qmax) / delta, i = floor(t),
 * f = t - i; inside (t >= 0 and i <= nb - 2) V = V_i + f (V_{i+1} - V_i) and V' = (V_{i+1} - V_i) / delta; outside, with
 * d = |q| - qmax and V_edge the nearer end node, V = V_edge + wall d^2 / 2 and V' = sign(q) wall d (q = +qmax lands here, d = 0).
 * Biased action S_b = -beta sum cos P + V(Q_m), H = S_b + sum v^2 / 2; the force is the plain stencil on
 *     gP = beta sin P + c cos P,  c = V'(Q_m) / 2 pi:   F0 = gP(i,j) - gP(i,j-1),  F1 = gP(i-1,j) - gP(i,j)
 * (fthmc_wilson_force's sign).  Under a frozen table <O> = sum O e^{V(Q_m)} / sum e^{V(Q_m)} is the unbiased expectation value. */

/* No reference counterpart.  Scratch of fthmc_meta_trajectory: 0 for path 1 (the one-launch path needs none) and for refused
 * arguments, else the sequenced path's (path 0 may take it: x_new == x, L > 64), a multiple of 256 bytes. */
size_t fthmc_meta_ws_bytes(int B, int L, int path);

/* No reference counterpart.  One biased HMC trajectory of every chain: H0 = S_b(x) + v^2 / 2, the MD of (integrator, dt, nstep)
 * (FTHMC_INT_*) under the biased force, the end point regularized, H1, accept iff u[b] < exp(-(H1 - H0)).  x_new, dH, acc, H0,
 * H1 as fthmc_hmc_trajectory_int; qm_out[B], vb_out[B]: Q_m and V(Q_m) of the field x_new holds.  dH .. vb_out may be NULL.
 * path: 1 = one launch per trajectory, one workgroup per chain (L <= 64, x_new must not be x, no workspace); 2 = the sequenced
 * path (any L, x_new may be x, workspace fthmc_meta_ws_bytes); 0 = the library chooses: 1 when L <= 64, the MFMA variant is
 * set and x_new != x, as fthmc_hmc_trajectory_int chooses.  With an all-zero table and no wall path 1 gives the bits of
 * fthmc_hmc_trajectory_int's one-launch kernels and path 2 those of its sequenced form.  A chain's result does not depend on B or
 * on its place in the batch (G = B).  Enqueue-only, capturable.  The sequenced path launches the plain kernels' shapes, which put the
 * chain on grid y: it serves B <= 65535 (beyond: FTHMC_ERR_UNSUPPORTED, and fthmc_meta_ws_bytes is 0); the one-launch path,
 * fthmc_meta_deposit, fthmc_meta_force and fthmc_meta_action take B up to FTHMC_MAX_B.
 * A null x / v / u / x_new / vtab, B or L out of range, nstep < 1, G < 1 or B % G != 0, nb < 2 or nb > 65536, a qmax that is not
 * finite and positive, a wall that is not finite and >= 0, path outside 0 .. 2, path 1 with L > 64 or x_new == x: FTHMC_ERR_ARG;
 * an unknown integrator, B > 65535 on the sequenced path: FTHMC_ERR_UNSUPPORTED; a short (or null) workspace where one is needed:
 * FTHMC_ERR_WS. */
int fthmc_meta_trajectory(const double* x, const double* v, const double* u, int B, int L, double beta, double dt, int nstep,
                          int integrator, const double* vtab, int G, int nb, double qmax, double wall, int path,
                          double* x_new, double* dH, double* acc, double* H0, double* H1, double* qm_out /* [B] or NULL */,
                          double* vb_out /* [B] or NULL */, void* ws, size_t ws_bytes, void* stream);

/* No reference counterpart.  One hill per walker, added to the table IN PLACE: for qm[b] inside the table (the lookup's rule) node i
 * of the chain's row gains w (1 - f) and node i + 1 gains w f, each product rounded before it is added; outside nothing is added.
 * The walkers of one row are added in chain order, without atomics: a node's value is ((V + h_b1) + h_b2) + ... over the chains
 * b1 < b2 < ... that touch it.  Refusals as above (w: finite and >= 0; a null qm). */
int fthmc_meta_deposit(const double* qm, int B, int G, int nb, double qmax, double w, double* vtab /* in place */, void* stream);

/* No reference counterpart.  The bias on its own, for tests and measurements: F[B][2][L][L] = dS_b / dx, and per chain S = S_b,
 * qm = Q_m, vb = V(Q_m) (each of the three may be NULL).  Refusals as above. */
int fthmc_meta_force(const double* x, int B, int L, double beta, const double* vtab, int G, int nb, double qmax, double wall,
                     double* F, void* stream);
int fthmc_meta_action(const double* x, int B, int L, double beta, const double* vtab, int G, int nb, double qmax, double wall,
                      double* S, double* qm, double* vb, void* stream);

/* ---- Metadynamics ftHMC: the same bias through the flow.  Latent field x, physical field y = F(x) (n_layers coupling layers),
 *     S_b(x) = -beta sum cos P(y) - log det J(x) + V(Q_m(y)),      H = S_b + sum v^2 / 2.
 * Table, rows, lookup and wall as above.  The force with respect to x is fthmc_ft_force's backward sweep seeded with
 * gP = beta sin P(y) + c cos P(y), c = V'(Q_m(y)) / 2 pi, in place of beta sin P(y).  Every output of a chain depends on the chain
 * and its own table row only, never on B or on the chain's place in the batch.
 * The reference has no counterpart to any of the four entry points below.
 * What they refuse, in this order: a null x (v, u, x_new; F) / vtab, w null with n_layers > 0, B or L out of range, n_layers < 0,
 * nstep < 1, G < 1 or B % G != 0, nb < 2 or nb > 65536, a qmax that is not finite and positive, a wall that is not finite and >= 0:
 * FTHMC_ERR_ARG; an unknown activation or integrator, a refused arch, B > 65535 where the sequenced kernels run (they put the chain
 * on grid y): FTHMC_ERR_UNSUPPORTED; then the workspace (FTHMC_ERR_WS) and the weights-version check.  Enqueue-only, capturable. */

/* No reference counterpart.  Scratch of the three calls below: fthmc_ws_bytes(arch, B, L, n_layers) and behind it the two rows of
 * chain sums (sum sin P, sum cos P), rounded like every region (a multiple of 256 bytes); 0 for refused arguments. */
size_t fthmc_ft_meta_ws_bytes(const fthmc_arch_t* arch, int B, int L, int n_layers);

/* No reference counterpart.  One biased flowed trajectory of every chain (FTHMC_MODE_MD only): H0, the MD of (integrator, dt,
 * nstep) under the biased force, the end point regularized, H1, accept iff u[b] < exp(-(H1 - H0)).  x_new .. H1 as
 * fthmc_ft_trajectory_int_v; plaq, Q, qm_out, vb_out [B]: of F(x_new), vb_out under the table of this call.  dH .. vb_out may be NULL.
 * state_in / state_out (either may be NULL): [4][B] = (S_eff WITHOUT the bias, plaq, Q, Q_m) of x / of x_new.  The state is
 * table-free: a chained call looks V(Q_m) up in the table it is given, so hills deposited between two calls leave it valid, and a
 * chained call gives the bits of a stateless one at any table.
 * L = 8, 12, 16 with the default net and the small path on: one launch (k_ft_small's biased instance); every other shape
 * fthmc_ft_trajectory_int_v serves: its sequence with the biased seed in every force and V(Q_m) added to either energy.  With
 * an all-zero table and no wall either gives the bits of fthmc_ft_trajectory_int_v. */
int fthmc_ft_meta_trajectory_v(const double* x, const double* v, const double* u, const double* w, const fthmc_arch_t* arch, int n_layers,
                               int B, int L, int act, double beta, double dt, int nstep, int integrator, const double* vtab, int G,
                               int nb, double qmax, double wall, double* x_new, double* dH, double* acc, double* H0, double* H1,
                               double* plaq, double* Q, double* qm_out, double* vb_out, const double* state_in /* [4][B] or NULL */,
                               double* state_out /* [4][B] or NULL */, void* ws, size_t ws_bytes, void* stream,
                               uint64_t weights_version);

/* No reference counterpart.  The biased flowed force and action on their own, for tests and measurements (always the sequenced
 * kernels): F[B][2][L][L] = dS_b / dx; per chain S_b, logdet = log det J, qm = Q_m(F(x)), vbias = V(Q_m) (each of the four may be
 * NULL). */
int fthmc_ft_meta_force_v(const double* x, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L, int act, double beta,
                          const double* vtab, int G, int nb, double qmax, double wall, double* F, void* ws, size_t ws_bytes,
                          void* stream, uint64_t weights_version);
int fthmc_ft_meta_action_v(const double* x, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L, int act, double beta,
                           const double* vtab, int G, int nb, double qmax, double wall, double* S_b, double* logdet, double* qm,
                           double* vbias, void* ws, size_t ws_bytes, void* stream, uint64_t weights_version);

/* ---- Boundary-condition tempering: plain HMC whose action carries a per-chain coupling on a short line of plaquettes, the defect
 * (Hasenbusch 2017; Bonanno, Bonati, D'Elia 2021; after the open boundaries of Luescher and Schaefer 2011).  The reference has no
 * counterpart to any of the five entry points below: it samples the periodic lattice only.
 * P(i,j) is the plaquette as fthmc_plaquettes forms it.  The defect is the row of plaquettes
 *     D = {((i0 + a) mod L, j0) : 0 <= a < Ld},      0 <= Ld <= L,  0 <= i0, j0 < L,
 * the same for every chain of a call.  Chain b has the defect coupling g_b[b] = beta c_b (a device array [B], c_b in [0, 1] the
 * caller's promise: 0 opens the line, 1 is the periodic lattice).  With C = sum over all plaquettes of cos P (BatchAction's order of
 * the four links, the chain sums of fthmc_wilson_action_charge) and Dsum = the same cosines summed over D
 *     S_d = (-beta) C + (beta - g_b) Dsum,      H = S_d + sum v^2 / 2,
 *     gP(p) = w(p) sin P(p),  w = g_b on D, beta elsewhere:   F0 = gP(i,j) - gP(i,j-1),  F1 = gP(i-1,j) - gP(i,j)
 * (fthmc_wilson_force's sign).  With g_b = beta for every chain the second term of S_d is an exact zero and every weight is beta:
 * fthmc_defect_trajectory then gives the bits of fthmc_hmc_trajectory_pb with beta_b = beta on the same path.
 * A ladder of such chains at ONE beta is exchanged by fthmc_replica_swap as it is, given betas := the ladder of g, C := Dsum and
 * beta_b := g_b: the pair (a on rung k, c on rung k + 1) is accepted with min(1, exp((g_k - g_{k+1}) (Dsum_c - Dsum_a))).
 * What the calls refuse: a null x (v, u, x_new; F) / g_b, B or L out of range, nstep < 1, Ld outside [0, L], i0 or j0 outside [0, L),
 * a beta that is not finite, path outside 0 .. 2, path 1 with L > 64 or x_new == x: FTHMC_ERR_ARG; an unknown integrator, B > 65535 on
 * the sequenced path: FTHMC_ERR_UNSUPPORTED; a short (or null) workspace where one is needed: FTHMC_ERR_WS. */

/* No reference counterpart.  Scratch of fthmc_defect_trajectory, by fthmc_meta_ws_bytes' rule: 0 for path 1 (the one-launch path needs
 * none) and for refused arguments, else the sequenced path's (path 0 may take it: x_new == x, L > 64), a multiple of 256 bytes. */
size_t fthmc_defect_ws_bytes(int B, int L, int path);

/* No reference counterpart.  One trajectory of every chain: H0 = S_d(x) + v^2 / 2, the MD of (integrator, dt, nstep) (FTHMC_INT_*) under
 * the force above, the end point regularized, H1, accept iff u[b] < exp(-(H1 - H0)).  x_new, dH, acc, H0, H1 as
 * fthmc_hmc_trajectory_int; csum_out[B], dsum_out[B], q_out[B]: C, Dsum and the integer charge (the rounded sum of the wrapped
 * plaquettes over 2 pi) of the field x_new holds.  dH .. q_out may be NULL.
 * path: 1 = one launch per trajectory, one workgroup per chain (L <= 64, x_new must not be x, no workspace); 2 = the sequenced path
 * (any L, x_new may be x, workspace fthmc_defect_ws_bytes, B <= 65535); 0 = the library chooses, as fthmc_meta_trajectory does.
 * Enqueue-only, capturable; two calls give the same bits; a chain's result does not depend on B or on its place in the batch. */
int fthmc_defect_trajectory(const double* x, const double* v, const double* u, int B, int L, double beta, const double* g_b /* [B] */,
                            int i0, int j0, int Ld, double dt, int nstep, int integrator, int path, double* x_new, double* dH,
                            double* acc, double* H0, double* H1, double* csum_out /* [B] or NULL */, double* dsum_out /* [B] or NULL */,
                            double* q_out /* [B] or NULL */, void* ws, size_t ws_bytes, void* stream);

/* No reference counterpart.  The pieces on their own, for tests and tools: F[B][2][L][L] = dS_d / dx, and per chain S = S_d, csum = C,
 * dsum = Dsum, Q = the integer charge (each of the four may be NULL).  B up to FTHMC_MAX_B. */
int fthmc_defect_force(const double* x, int B, int L, double beta, const double* g_b, int i0, int j0, int Ld, double* F, void* stream);
int fthmc_defect_action(const double* x, int B, int L, double beta, const double* g_b, int i0, int j0, int Ld, double* S, double* csum,
                        double* dsum, double* Q, void* stream);

/* No reference counterpart.  The translation that moves the defect relative to the field: for the chains with rung[b] == top
 *     x_out[b][mu][(i + s0) mod L][(j + s1) mod L] = x[b][mu][i][j],      (s0, s1) = shift[b][0 .. 1] (any integers),
 * every other chain is copied; a copy bit for bit either way.  rung: int32 [B], shift: int32 [B][2], both on the device.  A symmetry of
 * the periodic rung only.  x_out must not be x (it closes the two-buffer ping-pong of path 1: the trajectory goes x -> x_new, the
 * translation x_new -> x).  A null x / x_out / rung / shift, x_out == x, B or L out of range: FTHMC_ERR_ARG. */
int fthmc_defect_translate(const double* x, int B, int L, const int32_t* rung, int top, const int32_t* shift, double* x_out, void* stream);

/* ---- training ------------------------------------------------------------ */
/* Reverse-KL loss pieces and weight gradients for a fixed prior draw xi
 * (fthmc/train.py:191-210, fthmc/utils/samplers.py:40-56):
 *   x = F(xi); logq = -2 L^2 log(2 pi) - logdet; logp = -S_W(x);
 *   loss = mean(logq - logp); gw = d loss / d w  (n_layers*955).
 * Outputs (any may be NULL): x[B][2][L][L], logq[B], logp[B], gw.
 * ws: fthmc_train_ws_bytes(arch, B, L, n_layers). */
int fthmc_train_grad(const double* xi, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L, int act,
                     double beta, double* x, double* logq, double* logp, double* gw,
                     void* ws, size_t ws_bytes, void* stream);

/* The prior draw of a training step on the device: out[b][0..n) ~ U[lo, hi) from Philox4x32-10 keyed by the per-chain
 * seed (MultivariateUniform.sample_n, fthmc/utils/distributions.py:65-76, called at fthmc/train.py:191 through
 * apply_flow_to_prior, fthmc/utils/samplers.py:40-56).  A chain's draw depends on its seed only, not on the sharding.
 * Each value is t * w + lo rounded ONCE (an fma), with w = hi - lo as fp64 rounds it and t = 1 - k / 2^53 for an integer
 * 1 <= k <= 2^53, i.e. t in [0, 1 - 2^-53] exactly.  So lo <= out <= hi always, out = lo for t = 0, and out < hi exactly
 * where the top value's distance from hi, w 2^-53, is more than half the spacing of the doubles below hi.  That holds on
 * (0, 1) and on the prior's (-pi, pi), and roughly wherever w > |hi| (lo <= 0 <= hi with |lo| not much smaller than hi); it
 * fails already on (1, 2) or (3, 4), and on (1e6, 1e6 + 1) the draws of the last half spacing below hi come out as hi:
 * U[lo, hi) is a property of the range, not of the call. */
int fthmc_random_uniform(const int64_t* seeds, int B, int n_per_chain, double lo, double hi, double* out, void* stream);

/* Per-chain seeds of one trajectory / training step, formed on the device: seeds[b] = the 63-bit SplitMix64 mix of
 * (seed, global chain id lo + b, t) -- the same numbers as the host helper of the multi-GPU layer (fthmc_amd/parallel.py
 * chain_seeds; SURVEY 7 "RNG": a chain's stream is keyed by its global id, never by the rank).  t = traj + *counter when
 * `counter` (a device int64) is given, else traj; with advance != 0 the kernel then adds 1 to *counter, so that a
 * captured launch draws fresh seeds at every replay without a host-to-device copy.  Replaces the host side of
 * torch.randn_like / prior.sample_n in the loops of fthmc/ft_hmc.py:204 and fthmc/train.py:191. */
int fthmc_chain_seeds(int64_t seed, int64_t lo, int B, int64_t traj, int64_t* counter, int advance, int64_t* seeds, void* stream);

/* Metrics of one training step from its pieces (train_step, fthmc/train.py:206-228; calc_dkl / calc_ess,
 * fthmc/utils/distributions.py:23-37; batch_charges, fthmc/utils/qed_helpers.py:108-116), ONE rank's batch:
 *   row[0] = loss_dkl = dkl_factor * mean(logq - logp)       row[1] = ess = exp(2 lse(logw) - lse(2 logw)) / B
 *   row[2 + k B + b], k = 0..4:  logp, logq, q = Q(x), dq = |Q(x) - Q(xi)|, plaq = logp / (beta L^2)   of chain b
 * (2 + 5 B doubles: what train_step returns, stacked, so that a training loop copies ONE buffer to the host, when it
 * wants to look).  ws: fthmc_ws_bytes(NULL, B, L, 0). */
int fthmc_train_metrics(const double* xi, const double* x, const double* logq, const double* logp, int B, int L,
                        double beta, double dkl_factor, double* row, void* ws, size_t ws_bytes, void* stream);

/* The optimizer step of the training loop on the flat parameter buffer: torch.optim.Adam (decoupled = 0; fthmc/train.py:297
 * optim.Adam(model['layers'].parameters(), lr=config.base_lr)) or AdamW (decoupled = 1; train.py:86), torch's update formulas
 * element by element, in ONE launch over all n = n_layers * params values:  w, exp_avg, exp_avg_sq updated in place from gw.
 * hyper: THREE doubles on the device -- [0] the number of steps taken so far (the launch moves it on), [1] the learning rate,
 * [2] scratch, zero-initialised -- so that a captured launch can be replayed step after step and a scheduler changes the
 * rate by writing hyper[1]. */
int fthmc_adam_step(double* w, const double* gw, double* exp_avg, double* exp_avg_sq, double* hyper, size_t n,
                    double beta1, double beta2, double eps, double weight_decay, int decoupled, void* stream);

/* ---- measurement hook (the only entry point that synchronises) ---------- */
/* Average duration in milliseconds (host double) of `reps` back-to-back launches of one
 * coupling-layer kernel on `stream`, bracketed by HIP events recorded on that stream.
 * kind 0: forward kernel; 1: backward-wrt-x kernel of the force path (reads the forward's
 * activation stash with the MFMA variant, recomputes the forward with the VALU variant);
 * 2: fused plain-HMC leapfrog step (Wilson force stencil); 3: whole plain-HMC trajectory of 10
 * steps in one launch (L <= 64). */
int fthmc_time_kernel(int kind, const double* x, const double* w, const fthmc_arch_t* arch, int B, int L, int mu, int off,
                      int act, double beta, int reps, double* ms_avg_host,
                      void* ws, size_t ws_bytes, void* stream);

/* Measurement hook: average milliseconds per launch of the small-lattice fused trajectory kernel (two action sweeps,
 * nstep force sweeps, Metropolis), `reps` launches back to back between two HIP events on `stream`.  Synchronises. */
int fthmc_time_small(const double* x, const double* v, const double* u, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L, int act,
                     double beta, double dt, int nstep, int reps, double* ms_avg_host, void* ws, size_t ws_bytes, void* stream);
/* Measurement hook: one trajectory on the small-lattice fused path (fthmc_set_small_path) with cycle stamps of thread 0
 * of every chain; cycles_host32[k] = mean over chains of the cycles spent in stage k, summed over the trajectory
 * (0..6 forward layer stages, 8..13 backward layer stages, 16 copy, 17 Wilson seed, 18 kick, 19 action / charge).
 * Synchronises. */
int fthmc_small_profile(const double* x, const double* v, const double* u, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L,
                        int act, double beta, double dt, int nstep, double* cycles_host32, void* ws, size_t ws_bytes,
                        void* stream);
/* Diagnostic (synchronises, mallocs on the host): one launch of the MFMA forward (kind 0), stash backward
 * (kind 1), training backward (kind 2, ws: fthmc_train_ws_bytes) or weight-gradient (kind 3, same ws) kernel with per-workgroup
 * cycle stamps at every stage boundary;
 * cycles_host16[k] = mean cycles spent between stamp k-1 and stamp k. */
int fthmc_profile_stages(int kind, const double* x, const double* w, const fthmc_arch_t* arch, int B, int L, int mu, int off,
                         int act, double beta, double* cycles_host16,
                         void* ws, size_t ws_bytes, void* stream);

/* ---- Flowed boundary-condition tempering: the defect above on the PHYSICAL field of ftHMC.  Latent field x, physical field
 * y = F(x) (n_layers coupling layers); the defect D, the couplings g_b [B] (device) and ONE beta per call as for fthmc_defect_*.
 * With C = sum cos P(y) and Dsum = the cosines of D among them, in fthmc_defect_action's order,
 *     S(x) = (-beta) C + (beta - g_b) Dsum - log det J(x),      H = S + sum v^2 / 2.
 * The force with respect to x is fthmc_ft_force's backward sweep seeded with gP(p) = w(p) sin P(y)(p), w = g_b on D and beta
 * elsewhere, in place of beta sin P(y): one pass over the field, no chain-wide sum.  Every output of a chain depends on the chain and
 * its own g_b only, never on B or on the chain's place in the batch.
 * The reference has no counterpart to any of the four entry points below.
 * What they refuse, in this order: a null x (v, u, x_new; F) / g_b, w null with n_layers > 0, B or L out of range, n_layers < 0,
 * nstep < 1, Ld outside [0, L], i0 or j0 outside [0, L), a beta that is not finite: FTHMC_ERR_ARG; an unknown activation or
 * integrator, a refused arch, B > 65535 where the sequenced kernels run (they put the chain on grid y): FTHMC_ERR_UNSUPPORTED; then
 * the workspace (FTHMC_ERR_WS) and the weights-version check.  Enqueue-only, capturable. */

/* No reference counterpart.  Scratch of the three calls below: fthmc_ws_bytes(arch, B, L, n_layers) and behind it the three rows of
 * chain sums (C, Dsum, Q), rounded like every region (a multiple of 256 bytes); 0 for refused arguments. */
size_t fthmc_ft_defect_ws_bytes(const fthmc_arch_t* arch, int B, int L, int n_layers);

/* No reference counterpart.  One flowed trajectory of every chain with the defect (FTHMC_MODE_MD only): H0, the MD of (integrator,
 * dt, nstep) under the force above, the end point regularized, H1, accept iff u[b] < exp(-(H1 - H0)).  x_new .. H1 as
 * fthmc_ft_trajectory_int_v; plaq, Q, dsum_out [B]: of F(x_new).  dH .. dsum_out may be NULL.
 * state_in / state_out (either may be NULL): [4][B] = (S_eff of the PERIODIC action = (-beta) C - log det J, plaq, Q, Dsum) of x /
 * of x_new.  The state is g-free: a call forms H = S_eff + (beta - g_b) Dsum + K / 2 from it, so a swap of g between two chains
 * leaves it valid, and a chained call gives the bits of a stateless one at any g_b.
 * L = 8, 12, 16 with the default net and the small path on: one launch (k_ft_small's instance with a defect); every other shape
 * fthmc_ft_trajectory_int_v serves: its sequence with the weighted seed in every force and (beta - g_b) Dsum added to either
 * energy.  With g_b = beta for every chain, or with Ld = 0, either gives the bits of fthmc_ft_trajectory_int_v; with n_layers = 0
 * the call gives those of fthmc_defect_trajectory on path 2. */
int fthmc_ft_defect_trajectory_v(const double* x, const double* v, const double* u, const double* w, const fthmc_arch_t* arch, int n_layers,
                                 int B, int L, int act, double beta, const double* g_b /* [B] */, int i0, int j0, int Ld, double dt,
                                 int nstep, int integrator, double* x_new, double* dH, double* acc, double* H0, double* H1, double* plaq,
                                 double* Q, double* dsum_out, const double* state_in /* [4][B] or NULL */,
                                 double* state_out /* [4][B] or NULL */, void* ws, size_t ws_bytes, void* stream, uint64_t weights_version);

/* No reference counterpart.  The flowed force and action with the defect on their own, for tests and measurements (always the
 * sequenced kernels):
 * F[B][2][L][L] = dS / dx; per chain S, logdet = log det J, csum = C, dsum = Dsum, Q = the integer charge of F(x) (each of the five may
 * be NULL). */
int fthmc_ft_defect_force_v(const double* x, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L, int act, double beta,
                            const double* g_b, int i0, int j0, int Ld, double* F, void* ws, size_t ws_bytes, void* stream,
                            uint64_t weights_version);
int fthmc_ft_defect_action_v(const double* x, const double* w, const fthmc_arch_t* arch, int n_layers, int B, int L, int act, double beta,
                             const double* g_b, int i0, int j0, int Ld, double* S, double* logdet, double* csum, double* dsum, double* Q,
                             void* ws, size_t ws_bytes, void* stream, uint64_t weights_version);

#ifdef __cplusplus
}
#endif
#endif /* FTHMC_HIP_H */
