// TORCH_LIBRARY(fthmc_hip): the torch operator boundary of SURVEY.md 8(b), level 2, as a COMPILED dispatcher library.
//
// Every operator is a thin entry over the C ABI of libfthmc_hip.so (include/fthmc_hip.h): inputs are contiguous fp64 tensors
// on the HIP device, outputs and the per-call workspace are allocated by torch (caching allocator), the launch goes to
// at::hip::getCurrentHIPStream() and nothing synchronises; errors become c10::Error (RuntimeError).  Only the device dispatch
// key is registered: a CPU tensor fails in the dispatcher (there is no CPU fallback).  The s/t net's shape travels in the
// schema as plain integers (n_mix, hidden, kernel_size) and becomes the fthmc_arch_t of the call.
// Shape functions for tracing and the autograd formulas (which call the backward operators below) are attached from Python
// (fthmc_amd/torch_ops.py: torch.library.register_fake / register_autograd on these definitions).
//
// Built by csrc/Makefile with g++ (host code only; links libfthmc_hip.so next to it and PyTorch's libraries).
// Reference call sites each operator replaces: fthmc_amd/torch_ops.py docstring.
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <tuple>

#include "../../include/fthmc_hip.h"

namespace {

using at::Tensor;
using OptTensor = c10::optional<Tensor>;
using IntList = c10::optional<at::IntArrayRef>;
using Tensor2 = std::tuple<Tensor, Tensor>;
using Tensor3 = std::tuple<Tensor, Tensor, Tensor>;
using DeviceGuard = c10::hip::OptionalHIPGuardMasqueradingAsCUDA;

// ---------------------------------------------------------------- checked inputs
const double* cp(const Tensor& t) { return t.const_data_ptr<double>(); }
const double* cp_or_null(const Tensor& t) { return t.defined() ? cp(t) : nullptr; }
double* mp(Tensor& t) { return t.mutable_data_ptr<double>(); }

void on_device(const Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda(), name, ": tensor lives on ", t.device(), "; fthmc_hip runs on the MI355X only (no CPU fallback)");
}
Tensor dev64(const Tensor& t, const char* name) {
    on_device(t, name);
    TORCH_CHECK(t.scalar_type() == at::kDouble, name, ": dtype ", t.scalar_type(), "; the HIP path computes in float64");
    return t.contiguous();
}
Tensor i32(const Tensor& t, int64_t n, const char* name) {
    on_device(t, name);
    TORCH_CHECK(t.scalar_type() == at::kInt && t.is_contiguous() && t.numel() == n, name, ": expected a contiguous int32 tensor of ", n, " entries");
    return t;
}
Tensor field(const Tensor& t, const char* name) {
    Tensor f = dev64(t, name);
    TORCH_CHECK(f.dim() == 4 && f.size(1) == 2 && f.size(2) == f.size(3), name, ": expected [B, 2, L, L], got ", f.sizes());
    TORCH_CHECK(f.size(2) % 4 == 0, name, ": L = ", f.size(2), " must be a multiple of 4 (stripe masks have period 4)");
    return f;
}
// a second field of a call (momenta, a cotangent)
Tensor shaped_like(const Tensor& x, const Tensor& t, const char* name) {
    Tensor f = field(t, name);
    TORCH_CHECK(f.sizes() == x.sizes(), name, ": shaped like x expected");
    return f;
}
Tensor weights(const Tensor& w, int64_t expect, const char* name) {
    Tensor f = dev64(w, name).reshape({-1});
    TORCH_CHECK(f.numel() == expect, name, ": expected ", expect, " doubles for this net shape, got ", f.numel());
    return f;
}
Tensor perchain(const Tensor& t, int64_t B, const char* name) {
    Tensor f = dev64(t, name).reshape({-1});
    TORCH_CHECK(f.numel() == B, name, ": expected ", B, " entries, got ", f.numel());
    return f;
}
// an absent optional tensor is an undefined Tensor (cp_or_null hands the library a null pointer for it)
Tensor optional_perchain(const OptTensor& t, int64_t B, const char* name) { return t.has_value() ? perchain(*t, B, name) : Tensor(); }
Tensor seeds64(const OptTensor& t, int64_t B) {
    if (!t.has_value()) return Tensor();
    Tensor seeds = t->contiguous();
    TORCH_CHECK(seeds.is_cuda() && seeds.scalar_type() == at::kLong && seeds.numel() == B, "seeds: expected ", B, " int64 seeds on the HIP device");
    return seeds;
}
const int64_t* seeds_or_null(const Tensor& seeds) { return seeds.defined() ? seeds.const_data_ptr<int64_t>() : nullptr; }

void ok(int rc, const char* what) {
    TORCH_CHECK(rc == FTHMC_OK, what, " failed: ", fthmc_strerror(rc), " (code ", rc, ") ", rc == FTHMC_ERR_LAUNCH ? fthmc_last_error() : "");
}

// the fthmc_arch_t of a call from the schema's integers (hidden = None: the reference default [8, 8])
struct Arch {
    fthmc_arch_t a;
    bool is_default;
    Arch(int64_t n_mix, IntList hidden, int64_t kernel_size) {
        a = fthmc_arch_t{};
        a.n_mix = (int)n_mix; a.kernel_size = (int)kernel_size;
        if (hidden.has_value()) {
            TORCH_CHECK(hidden->size() <= 8, "hidden: at most 8 hidden layers");
            a.n_hidden = (int)hidden->size();
            for (size_t i = 0; i < hidden->size(); ++i) a.hidden[i] = (int)(*hidden)[i];
        } else { a.n_hidden = 2; a.hidden[0] = 8; a.hidden[1] = 8; }
        is_default = a.n_hidden == 2 && a.hidden[0] == 8 && a.hidden[1] == 8 && a.kernel_size == 3 && a.n_mix == 2;
    }
    const fthmc_arch_t* ptr() const { return is_default ? nullptr : &a; }
    int64_t params() const { const int p = fthmc_arch_params(ptr()); TORCH_CHECK(p > 0, "net shape beyond the limits of the HIP kernels"); return p; }
};

// ---------------------------------------------------------------- the per-call scratch, allocated by torch
Tensor scratch(size_t bytes, const Tensor& like) { return at::empty({(int64_t)((bytes + 7) / 8)}, like.options()); }

enum class Ws { plain, train, vjp, train_force };     // which size query of the C ABI a call's workspace answers to

struct Workspace {
    Tensor buf; size_t bytes;
    Workspace(Ws kind, const Tensor& like, const fthmc_arch_t* arch, int B, int L, int nl) {
        switch (kind) {
            case Ws::plain: bytes = fthmc_ws_bytes(arch, B, L, nl); break;
            case Ws::train: bytes = fthmc_train_ws_bytes(arch, B, L, nl); break;
            case Ws::vjp: bytes = fthmc_vjp_ws_bytes(arch, B, L, nl); break;
            case Ws::train_force: bytes = fthmc_train_force_ws_bytes(arch, B, L, nl); break;
        }
        TORCH_CHECK(bytes > 0, "unsupported shape (B = ", B, ", L = ", L, ", n_layers = ", nl, ")");
        buf = scratch(bytes, like);
    }
    void* ptr() { return buf.mutable_data_ptr<double>(); }
};

// ---------------------------------------------------------------- the prologue of every operator
// A call on a field: it runs with that tensor's device current -- the workspace and the outputs are allocated there and the launch
// goes to THAT device's current stream, whatever device the calling thread had selected (several GPUs in one process).
struct FieldCall {
    const DeviceGuard guard;
    const Tensor x;                     // checked and contiguous
    const int B, L;
    void* const stream;
    explicit FieldCall(const Tensor& x_, const char* name = "x")
        : guard(x_.device()), x(field(x_, name)), B((int)x.size(0)), L((int)x.size(2)),
          stream(c10::hip::getCurrentHIPStream(x.device().index()).stream()) {}
    Tensor like_x() const { return at::empty_like(x); }
    Tensor per_chain(at::ScalarType dtype = at::kDouble) const { return at::empty({B}, x.options().dtype(dtype)); }
    Workspace workspace() const { return Workspace(Ws::plain, x, nullptr, B, L, 0); }
};
// A call through the flow: the net shape from the schema's integers, and the weights of one layer ("w", n_layers = 1) or of all
// n_layers ("w_all") checked against it.
struct FlowCall : FieldCall {
    const Arch A;
    const Tensor w;
    const int nl;
    FlowCall(const Tensor& x_, const char* xname, const Tensor& w_, const char* wname, int64_t n_layers, int64_t n_mix, IntList hidden,
             int64_t kernel_size)
        : FieldCall(x_, xname), A(n_mix, hidden, kernel_size), w(weights(w_, n_layers * A.params(), wname)), nl((int)n_layers) {}
    Tensor like_w() const { return at::empty({w.numel()}, x.options()); }
    // a weight gradient that the library skips without layers: zeroed, and handed over only where there are layers
    Tensor zero_gw() const { return at::zeros({w.numel()}, x.options()); }
    double* gw_ptr(Tensor& gw) const { return nl > 0 ? mp(gw) : nullptr; }
    Workspace workspace(Ws kind = Ws::plain) const { return Workspace(kind, x, A.ptr(), B, L, nl); }
};

// ---------------------------------------------------------------- Wilson
Tensor3 wilson_action_charge(const Tensor& x, double beta) {
    FieldCall c(x);
    Tensor S = c.per_chain(), Q = c.per_chain(), plaq = c.per_chain();
    ok(fthmc_wilson_action_charge(cp(c.x), c.B, c.L, beta, mp(S), mp(Q), mp(plaq), c.stream), "fthmc_wilson_action_charge");
    return {S, Q, plaq};
}
Tensor wilson_force(const Tensor& x, double beta) {
    FieldCall c(x);
    Tensor F = c.like_x();
    ok(fthmc_wilson_force(cp(c.x), c.B, c.L, beta, mp(F), c.stream), "fthmc_wilson_force");
    return F;
}
// the table of Wilson loops [B, Rmax, Tmax] (no autograd formula: an observable)
Tensor wilson_loops(const Tensor& x, int64_t Rmax, int64_t Tmax) {
    FieldCall c(x);
    TORCH_CHECK(Rmax >= 1 && Rmax <= c.L && Tmax >= 1 && Tmax <= c.L, "wilson_loops: 1 <= Rmax, Tmax <= L = ", c.L, " expected, got ", Rmax, ", ", Tmax);
    const size_t bytes = fthmc_wilson_loops_ws_bytes(c.B, c.L, (int)Rmax, (int)Tmax);
    TORCH_CHECK(bytes > 0, "wilson_loops: unsupported shape (B = ", c.B, ", L = ", c.L, ", Rmax = ", Rmax, ", Tmax = ", Tmax, ")");
    Tensor ws = scratch(bytes, c.x), W = at::empty({c.B, Rmax, Tmax}, c.x.options());
    ok(fthmc_wilson_loops(cp(c.x), c.B, c.L, (int)Rmax, (int)Tmax, mp(W), nullptr, mp(ws), bytes, c.stream), "fthmc_wilson_loops");
    return W;
}
// heatbath / overrelaxation sweeps -> the updated field (no autograd formula: a sampler step)
Tensor local_update(const Tensor& x, double beta, const OptTensor& beta_b_, const OptTensor& seeds_, int64_t n_hb, int64_t n_or, int64_t nsweep,
                    int64_t sweep0, int64_t classes) {
    FieldCall c(x);
    TORCH_CHECK(n_hb >= 0 && n_or >= 0 && nsweep >= 0 && n_hb <= INT32_MAX && n_or <= INT32_MAX && nsweep <= INT32_MAX && sweep0 >= 0 &&
                classes >= 1 && classes <= 15, "local_update: counts >= 0, sweep0 >= 0 and classes in 1 .. 15 expected");
    Tensor beta_b = optional_perchain(beta_b_, c.B, "beta_b"), seeds = seeds64(seeds_, c.B);
    TORCH_CHECK(n_hb == 0 || seeds.defined(), "local_update: heatbath sweeps need seeds");
    Tensor out = c.like_x();
    ok(fthmc_local_update(cp(c.x), c.B, c.L, beta, cp_or_null(beta_b), seeds_or_null(seeds), (int)n_hb, (int)n_or, (int)nsweep, sweep0,
                          (int)classes, mp(out), c.stream), "fthmc_local_update");
    return out;
}
// instanton hits -> (the updated field, the applied charge k, the accepted steps), k and nacc int32 [B] (no autograd formula: a
// sampler step); the library chooses the launch shape
Tensor3 instanton_hit(const Tensor& x, double beta, const OptTensor& beta_b_, const OptTensor& seeds_, int64_t n_hit, int64_t hit0) {
    FieldCall c(x);
    TORCH_CHECK(n_hit >= 0 && n_hit <= 1024 && hit0 >= 0 && hit0 <= ((int64_t)1 << 32) - n_hit,
                "instanton_hit: n_hit in 0 .. 1024 and hit0 >= 0 with hit0 + n_hit <= 2^32 expected");
    Tensor beta_b = optional_perchain(beta_b_, c.B, "beta_b"), seeds = seeds64(seeds_, c.B);
    TORCH_CHECK(n_hit == 0 || seeds.defined(), "instanton_hit: hits need seeds");
    Tensor out = c.like_x(), k = c.per_chain(at::kInt), nacc = c.per_chain(at::kInt);
    const size_t bytes = fthmc_instanton_ws_bytes(c.B, c.L, 0);
    Tensor ws;
    if (bytes > 0) ws = scratch(bytes, c.x);
    ok(fthmc_instanton_hit(cp(c.x), c.B, c.L, beta, cp_or_null(beta_b), seeds_or_null(seeds), (int)n_hit, hit0, 0, mp(out),
                           k.mutable_data_ptr<int32_t>(), nacc.mutable_data_ptr<int32_t>(), nullptr, bytes > 0 ? mp(ws) : nullptr, bytes, c.stream),
       "fthmc_instanton_hit");
    return {out, k, nacc};
}
Tensor3 hmc_trajectory(const Tensor& x, const Tensor& v_, const Tensor& u_, double beta, double dt, int64_t nstep) {
    FieldCall c(x);
    Tensor v = shaped_like(c.x, v_, "v"), u = perchain(u_, c.B, "u");
    Tensor xn = c.like_x(), dH = c.per_chain(), acc = c.per_chain();
    Workspace ws = c.workspace();
    ok(fthmc_hmc_trajectory(cp(c.x), cp(v), cp(u), c.B, c.L, beta, dt, (int)nstep, mp(xn), mp(dH), mp(acc), nullptr, nullptr, ws.ptr(), ws.bytes,
                            c.stream), "fthmc_hmc_trajectory");
    return {xn, dH, acc};
}

// ---------------------------------------------------------------- one coupling layer
Tensor2 flow_layer_fwd(const Tensor& x, const Tensor& w, int64_t mu, int64_t off, int64_t n_mix, int64_t act, IntList hidden, int64_t kernel_size) {
    FlowCall c(x, "x", w, "w", 1, n_mix, hidden, kernel_size);
    Tensor y = c.like_x(), logJ = c.per_chain();
    Workspace ws = c.workspace();
    ok(fthmc_flow_layer_fwd(cp(c.x), cp(c.w), c.A.ptr(), c.B, c.L, (int)mu, (int)off, (int)act, mp(y), mp(logJ), ws.ptr(), ws.bytes, c.stream),
       "fthmc_flow_layer_fwd");
    return {y, logJ};
}
// the three backward schemas over one launch: gw is computed (and its larger workspace taken) only where asked for
Tensor2 layer_bwd(const Tensor& x, const Tensor& gy_, const Tensor& glogJ_, const Tensor& w, int64_t mu, int64_t off, int64_t n_mix, int64_t act,
                  IntList hidden, int64_t kernel_size, bool need_gw) {
    FlowCall c(x, "x", w, "w", 1, n_mix, hidden, kernel_size);
    Tensor gy = shaped_like(c.x, gy_, "gy"), glogJ = perchain(glogJ_, c.B, "glogJ");
    Tensor gx = c.like_x(), gw = need_gw ? c.like_w() : Tensor();
    Workspace ws = c.workspace(need_gw ? Ws::train : Ws::plain);
    ok(fthmc_flow_layer_bwd(cp(c.x), cp(c.w), c.A.ptr(), cp(gy), cp(glogJ), c.B, c.L, (int)mu, (int)off, (int)act, mp(gx),
                            need_gw ? mp(gw) : nullptr, ws.ptr(), ws.bytes, c.stream), "fthmc_flow_layer_bwd");
    return {gx, gw};
}
Tensor flow_layer_bwd_x(const Tensor& x, const Tensor& gy, const Tensor& glogJ, const Tensor& w, int64_t mu, int64_t off, int64_t n_mix,
                        int64_t act, IntList hidden, int64_t kernel_size) {
    return std::get<0>(layer_bwd(x, gy, glogJ, w, mu, off, n_mix, act, hidden, kernel_size, false));
}
Tensor flow_layer_bwd_w(const Tensor& x, const Tensor& gy, const Tensor& glogJ, const Tensor& w, int64_t mu, int64_t off, int64_t n_mix,
                        int64_t act, IntList hidden, int64_t kernel_size) {
    return std::get<1>(layer_bwd(x, gy, glogJ, w, mu, off, n_mix, act, hidden, kernel_size, true));
}
Tensor2 flow_layer_bwd(const Tensor& x, const Tensor& gy, const Tensor& glogJ, const Tensor& w, int64_t mu, int64_t off, int64_t n_mix,
                       int64_t act, IntList hidden, int64_t kernel_size) {
    return layer_bwd(x, gy, glogJ, w, mu, off, n_mix, act, hidden, kernel_size, true);
}
Tensor2 flow_layer_rev(const Tensor& y, const Tensor& w, int64_t mu, int64_t off, int64_t n_mix, int64_t act, double tol, IntList hidden,
                       int64_t kernel_size) {
    FlowCall c(y, "y", w, "w", 1, n_mix, hidden, kernel_size);      // c.x is y here
    Tensor x = c.like_x(), logJ = c.per_chain();
    Workspace ws = c.workspace();
    ok(fthmc_flow_layer_rev(cp(c.x), cp(c.w), c.A.ptr(), c.B, c.L, (int)mu, (int)off, (int)act, tol, mp(x), mp(logJ), ws.ptr(), ws.bytes, c.stream),
       "fthmc_flow_layer_rev");
    return {x, logJ};
}

// ---------------------------------------------------------------- whole flow
Tensor3 ft_action_force(const Tensor& x, const Tensor& w_all, int64_t n_layers, double beta, int64_t act, int64_t n_mix, IntList hidden,
                        int64_t kernel_size) {
    FlowCall c(x, "x", w_all, "w_all", n_layers, n_mix, hidden, kernel_size);
    Tensor S = c.per_chain(), logdet = c.per_chain(), F = c.like_x();
    Workspace ws = c.workspace();
    ok(fthmc_ft_action(cp(c.x), cp(c.w), c.A.ptr(), c.nl, c.B, c.L, (int)act, beta, mp(S), mp(logdet), nullptr, nullptr, ws.ptr(), ws.bytes, c.stream),
       "fthmc_ft_action");
    ok(fthmc_ft_force(cp(c.x), cp(c.w), c.A.ptr(), c.nl, c.B, c.L, (int)act, beta, mp(F), ws.ptr(), ws.bytes, c.stream), "fthmc_ft_force");
    return {S, logdet, F};
}
// second order (the autograd formula of ft_action_force, torch_ops.py): gw has n_layers * params entries (none without layers)
Tensor2 ft_action_vjp(const Tensor& x, const Tensor& w_all, int64_t n_layers, double beta, int64_t act, const Tensor& gS_, const OptTensor& glogdet_,
                      int64_t n_mix, IntList hidden, int64_t kernel_size) {
    FlowCall c(x, "x", w_all, "w_all", n_layers, n_mix, hidden, kernel_size);
    Tensor gS = perchain(gS_, c.B, "gS"), glogdet = optional_perchain(glogdet_, c.B, "glogdet");
    Tensor gx = c.like_x(), gw = c.zero_gw();
    Workspace ws = c.workspace(Ws::vjp);
    ok(fthmc_ft_action_vjp(cp(c.x), cp(c.w), c.A.ptr(), c.nl, c.B, c.L, (int)act, beta, cp(gS), cp_or_null(glogdet), mp(gx), c.gw_ptr(gw), ws.ptr(),
                           ws.bytes, c.stream), "fthmc_ft_action_vjp");
    return {gx, gw};
}
Tensor2 ft_force_vjp(const Tensor& x, const Tensor& w_all, int64_t n_layers, double beta, int64_t act, const Tensor& g_, int64_t n_mix,
                     IntList hidden, int64_t kernel_size) {
    FlowCall c(x, "x", w_all, "w_all", n_layers, n_mix, hidden, kernel_size);
    Tensor g = shaped_like(c.x, g_, "g");
    Tensor gx = c.like_x(), gw = c.zero_gw();
    Workspace ws = c.workspace(Ws::vjp);
    ok(fthmc_ft_force_vjp(cp(c.x), cp(c.w), c.A.ptr(), c.nl, c.B, c.L, (int)act, beta, cp(g), mp(gx), c.gw_ptr(gw), ws.ptr(), ws.bytes, c.stream),
       "fthmc_ft_force_vjp");
    return {gx, gw};
}
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> fthmc_trajectory(const Tensor& x, const Tensor& v_, const Tensor& u_, const Tensor& w_all,
                                                                    int64_t n_layers, double beta, double dt, int64_t nstep, int64_t mode,
                                                                    int64_t act, int64_t n_mix, IntList hidden, int64_t kernel_size) {
    TORCH_CHECK(mode == FTHMC_MODE_MD || mode == FTHMC_MODE_LITERAL, "mode: expected 0 (md) or 1 (literal), got ", mode);
    FlowCall c(x, "x", w_all, "w_all", n_layers, n_mix, hidden, kernel_size);
    Tensor v = shaped_like(c.x, v_, "v"), u = perchain(u_, c.B, "u");
    Tensor xn = c.like_x(), dH = c.per_chain(), acc = c.per_chain(), plaq = c.per_chain(), Q = c.per_chain();
    Workspace ws = c.workspace();
    ok(fthmc_ft_trajectory(cp(c.x), cp(v), cp(u), cp(c.w), c.A.ptr(), c.nl, c.B, c.L, (int)act, beta, dt, (int)nstep, (int)mode, mp(xn), mp(dH),
                           mp(acc), nullptr, nullptr, mp(plaq), mp(Q), nullptr, nullptr, ws.ptr(), ws.bytes, c.stream), "fthmc_ft_trajectory");
    return {xn, dH, acc, plaq, Q};
}
std::tuple<Tensor, Tensor, Tensor, Tensor> train_grad(const Tensor& xi, const Tensor& w_all, int64_t n_layers, double beta, int64_t act,
                                                      int64_t n_mix, IntList hidden, int64_t kernel_size) {
    FlowCall c(xi, "xi", w_all, "w_all", n_layers, n_mix, hidden, kernel_size);      // c.x is xi here
    Tensor x = c.like_x(), logq = c.per_chain(), logp = c.per_chain(), gw = c.like_w();
    Workspace ws = c.workspace(Ws::train);
    ok(fthmc_train_grad(cp(c.x), cp(c.w), c.A.ptr(), c.nl, c.B, c.L, (int)act, beta, mp(x), mp(logq), mp(logp), mp(gw), ws.ptr(), ws.bytes, c.stream),
       "fthmc_train_grad");
    return {x, logq, logp, gw};
}
// the force-norm training step (ipynb/ft_hmc.py:253-299): F, sum F_b^2 and d(sum_b |F_b|^2)/dw (none without layers)
Tensor3 train_force_grad(const Tensor& x, const Tensor& w_all, int64_t n_layers, double beta, int64_t act, int64_t n_mix, IntList hidden,
                         int64_t kernel_size) {
    FlowCall c(x, "x", w_all, "w_all", n_layers, n_mix, hidden, kernel_size);
    Tensor F = c.like_x(), fsq = c.per_chain(), gw = c.zero_gw();
    Workspace ws = c.workspace(Ws::train_force);
    ok(fthmc_train_force_grad(cp(c.x), cp(c.w), c.A.ptr(), c.nl, c.B, c.L, (int)act, beta, mp(F), mp(fsq), c.gw_ptr(gw), ws.ptr(), ws.bytes, c.stream),
       "fthmc_train_force_grad");
    return {F, fsq, gw};
}

// ---------------------------------------------------------------- per-chain beta and replica exchange
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> ft_trajectory_pb(const Tensor& x, const Tensor& v_, const Tensor& u_, const Tensor& w_all,
                                                                            int64_t n_layers, const Tensor& beta_b_, double dt, int64_t nstep,
                                                                            int64_t integrator, int64_t act, const OptTensor& state_in_,
                                                                            int64_t n_mix, IntList hidden, int64_t kernel_size) {
    FlowCall c(x, "x", w_all, "w_all", n_layers, n_mix, hidden, kernel_size);
    Tensor v = shaped_like(c.x, v_, "v"), u = perchain(u_, c.B, "u"), beta_b = perchain(beta_b_, c.B, "beta_b");
    Tensor state_in;
    if (state_in_.has_value()) {
        state_in = dev64(*state_in_, "state_in");
        TORCH_CHECK(state_in.numel() == 3 * (int64_t)c.B, "state_in: expected [3, ", c.B, "]");
    }
    Tensor xn = c.like_x(), dH = c.per_chain(), acc = c.per_chain(), plaq = c.per_chain(), Q = c.per_chain(),
           state = at::empty({3, c.B}, c.x.options());
    Workspace ws = c.workspace();
    ok(fthmc_ft_trajectory_pb_v(cp(c.x), cp(v), cp(u), cp(c.w), c.A.ptr(), c.nl, c.B, c.L, (int)act, cp(beta_b), dt, (int)nstep, FTHMC_MODE_MD,
                                mp(xn), mp(dH), mp(acc), nullptr, nullptr, mp(plaq), mp(Q), cp_or_null(state_in), mp(state), ws.ptr(), ws.bytes,
                                c.stream, (int)integrator, 0), "fthmc_ft_trajectory_pb_v");
    return {xn, dH, acc, plaq, Q, state};
}
Tensor3 hmc_trajectory_pb(const Tensor& x, const Tensor& v_, const Tensor& u_, const Tensor& beta_b_, double dt, int64_t nstep, int64_t integrator) {
    FieldCall c(x);
    Tensor v = shaped_like(c.x, v_, "v"), u = perchain(u_, c.B, "u"), beta_b = perchain(beta_b_, c.B, "beta_b");
    Tensor xn = c.like_x(), dH = c.per_chain(), acc = c.per_chain();
    Workspace ws = c.workspace();
    ok(fthmc_hmc_trajectory_pb(cp(c.x), cp(v), cp(u), c.B, c.L, cp(beta_b), dt, (int)nstep, (int)integrator, mp(xn), mp(dH), mp(acc), nullptr, nullptr,
                               ws.ptr(), ws.bytes, c.stream), "fthmc_hmc_trajectory_pb");
    return {xn, dH, acc};
}
// no field in this call: it runs on beta_b's device.  beta_b, rung and chain_of are updated in place (the schema says so)
Tensor2 replica_swap(const Tensor& betas_, const Tensor& C_, const Tensor& u_, Tensor& beta_b, Tensor& rung, Tensor& chain_of, int64_t parity) {
    const DeviceGuard guard(beta_b.device());
    Tensor betas = dev64(betas_, "betas").reshape({-1});
    const int64_t K = betas.numel(), B = beta_b.numel();
    TORCH_CHECK(beta_b.is_cuda() && beta_b.scalar_type() == at::kDouble && beta_b.is_contiguous(), "beta_b: expected a contiguous float64 device tensor");
    TORCH_CHECK(K >= 2 && B > 0 && B % K == 0, "replica_swap: ", B, " chains do not form whole ladders of ", K, " rungs");
    const int64_t M = B / K;
    Tensor C = perchain(C_, B, "C"), u = perchain(u_, M * (K - 1), "u");
    i32(rung, B, "rung"); i32(chain_of, B, "chain_of");
    Tensor acc = at::empty({M, K - 1}, beta_b.options()), d = at::empty({M, K - 1}, beta_b.options());
    ok(fthmc_replica_swap(cp(betas), (int)K, (int)M, (int)parity, cp(C), cp(u), mp(beta_b), rung.mutable_data_ptr<int32_t>(),
                          chain_of.mutable_data_ptr<int32_t>(), mp(acc), mp(d), c10::hip::getCurrentHIPStream(beta_b.device().index()).stream()),
       "fthmc_replica_swap");
    return {acc, d};
}

}  // namespace

// The operators, each named once: X(function, "(arguments) -> returns").  fthmc_amd/torch_ops.py carries the same schema text in its
// table (tests/test_torch_boundary.py holds the two lists to each other).
#define FTHMC_OPERATORS(X) \
    X(wilson_action_charge, "(Tensor x, float beta) -> (Tensor, Tensor, Tensor)") \
    X(wilson_force, "(Tensor x, float beta) -> Tensor") \
    X(hmc_trajectory, "(Tensor x, Tensor v, Tensor u, float beta, float dt, int nstep) -> (Tensor, Tensor, Tensor)") \
    X(flow_layer_fwd, "(Tensor x, Tensor w, int mu, int off, int n_mix, int act, int[]? hidden=None, int kernel_size=3) -> (Tensor, Tensor)") \
    X(flow_layer_bwd_x, "(Tensor x, Tensor gy, Tensor glogJ, Tensor w, int mu, int off, int n_mix, int act, int[]? hidden=None, int kernel_size=3) -> Tensor") \
    X(flow_layer_bwd_w, "(Tensor x, Tensor gy, Tensor glogJ, Tensor w, int mu, int off, int n_mix, int act, int[]? hidden=None, int kernel_size=3) -> Tensor") \
    X(flow_layer_bwd, "(Tensor x, Tensor gy, Tensor glogJ, Tensor w, int mu, int off, int n_mix, int act, int[]? hidden=None, int kernel_size=3) -> (Tensor, Tensor)") \
    X(flow_layer_rev, "(Tensor y, Tensor w, int mu, int off, int n_mix, int act, float tol, int[]? hidden=None, int kernel_size=3) -> (Tensor, Tensor)") \
    X(ft_action_force, "(Tensor x, Tensor w_all, int n_layers, float beta, int act, int n_mix=2, int[]? hidden=None, int kernel_size=3) -> (Tensor, Tensor, Tensor)") \
    X(fthmc_trajectory, "(Tensor x, Tensor v, Tensor u, Tensor w_all, int n_layers, float beta, float dt, int nstep, int mode, int act, int n_mix=2, int[]? hidden=None, int kernel_size=3) -> (Tensor, Tensor, Tensor, Tensor, Tensor)") \
    X(train_grad, "(Tensor xi, Tensor w_all, int n_layers, float beta, int act, int n_mix=2, int[]? hidden=None, int kernel_size=3) -> (Tensor, Tensor, Tensor, Tensor)") \
    X(ft_action_vjp, "(Tensor x, Tensor w_all, int n_layers, float beta, int act, Tensor gS, Tensor? glogdet=None, int n_mix=2, int[]? hidden=None, int kernel_size=3) -> (Tensor, Tensor)") \
    X(ft_force_vjp, "(Tensor x, Tensor w_all, int n_layers, float beta, int act, Tensor g, int n_mix=2, int[]? hidden=None, int kernel_size=3) -> (Tensor, Tensor)") \
    X(train_force_grad, "(Tensor x, Tensor w_all, int n_layers, float beta, int act, int n_mix=2, int[]? hidden=None, int kernel_size=3) -> (Tensor, Tensor, Tensor)") \
    X(ft_trajectory_pb, "(Tensor x, Tensor v, Tensor u, Tensor w_all, int n_layers, Tensor beta_b, float dt, int nstep, int integrator, int act, Tensor? state_in=None, int n_mix=2, int[]? hidden=None, int kernel_size=3) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)") \
    X(hmc_trajectory_pb, "(Tensor x, Tensor v, Tensor u, Tensor beta_b, float dt, int nstep, int integrator=0) -> (Tensor, Tensor, Tensor)") \
    X(replica_swap, "(Tensor betas, Tensor C, Tensor u, Tensor(a!) beta_b, Tensor(b!) rung, Tensor(c!) chain_of, int parity) -> (Tensor, Tensor)") \
    X(wilson_loops, "(Tensor x, int Rmax, int Tmax) -> Tensor") \
    X(local_update, "(Tensor x, float beta, Tensor? beta_b, Tensor? seeds, int n_hb=1, int n_or=0, int nsweep=1, int sweep0=0, int classes=15) -> Tensor") \
    X(instanton_hit, "(Tensor x, float beta, Tensor? beta_b, Tensor? seeds, int n_hit=1, int hit0=0) -> (Tensor, Tensor, Tensor)")

TORCH_LIBRARY(fthmc_hip, m) {
#define FTHMC_DEF(name, schema) m.def(#name schema);
    FTHMC_OPERATORS(FTHMC_DEF)
#undef FTHMC_DEF
}

// "CUDA" is the dispatch key of HIP devices in PyTorch-ROCm
TORCH_LIBRARY_IMPL(fthmc_hip, CUDA, m) {
#define FTHMC_IMPL(name, schema) m.impl(#name, &name);
    FTHMC_OPERATORS(FTHMC_IMPL)
#undef FTHMC_IMPL
}
