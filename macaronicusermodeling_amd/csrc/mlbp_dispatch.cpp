// What a sweep call runs: the argument checks, the choice between the kernel families, and what follows the sweep kernels of a
// call.  Each family says for itself whether it applies (its *_plan behind its launch_* entry, mlbp_internal.h): this file offers
// the call in a fixed order and reads *launched.  Host code only: no kernel and no device descriptor here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "mlbp_internal.h"

using mlbp::fail;
using mlbp::FastPass; using mlbp::FAST_NONE; using mlbp::FAST_LEAN; using mlbp::FAST_SHARED;

namespace {

// mlbp_set_sweep_variant: 1 = the fast kernels with the exact kernel as fix-up (default), 3 = the exact / per-graph
// kernels on every graph (the tests' reference on the same inputs).
int g_sweep_variant = 1;
// mlbp_set_lean_walk: the order in which a lean launch's workgroups take the graphs -- 0 forward (default), 1 backward, 2 each
// program's launches in alternate directions (measured, LAB_NOTES R32: no gain behind non-temporal table loads, so not the
// default).  Read once per public call, like the variant.
int g_lean_walk = 0;
thread_local int g_last_lean_walk = 0;     // mlbp_last_lean_walk()
thread_local int g_last_kernel = -1;       // mlbp_last_sweep_kernel()
thread_local int g_last_fused_gradient = 0; // mlbp_last_sweep_fused_gradient()

// the program a call runs: the pruned twin under MLBP_SWEEP_SKIP_UNCHANGED (a fused gradient reads the final messages and
// the resident tables only, so it follows either list)
mlbp_program* effective_program(mlbp_program* p, const mlbp_sweep_args* a) {
  const bool pruned = (a->flags & MLBP_SWEEP_SKIP_UNCHANGED) && p->pruned;
  if (!p->is_twin) p->last_was_pruned = pruned;
  return pruned ? p->pruned : p;
}

// Every argument check of a sweep call of (prog, a), prog the program the call runs, made before anything is enqueued.  A
// grouped call makes them on all its groups first: one bad group fails it with the single call's message and launches nothing.
int check_sweep_args(const mlbp_program* prog, const mlbp_sweep_args* a) {
  if (a->B <= 0 || a->X <= 0) return fail(MLBP_EINVAL, "mlbp_sweep_f64: B=%d X=%d", a->B, a->X);
  if (!a->msgs) return fail(MLBP_EINVAL, "mlbp_sweep_f64: msgs is NULL");
  const bool f32_tables = (a->flags & MLBP_SWEEP_PAIR_TABLES_F32) != 0;
  if (prog->P > 0 && (!(f32_tables ? (const void*)a->pair_tables_f32 : (const void*)a->pair_tables) || !a->pair_tab || a->n_pair_tables <= 0))
    return fail(MLBP_EINVAL, "mlbp_sweep_f64: program has %d pairwise factors but no pair tables", prog->P);
  if (prog->U > 0 && (!a->unary_tables || !a->unary_tab || a->n_unary_tables <= 0))
    return fail(MLBP_EINVAL, "mlbp_sweep_f64: program has %d unary factors but no unary tables", prog->U);
  if (a->X > 4096) return fail(MLBP_EUNSUPPORTED, "mlbp_sweep_f64: X=%d > 4096", a->X);
  const bool approx = (a->flags & MLBP_SWEEP_APPROX_INFERENCE) != 0;
  if (approx && a->X < MLBP_APPROX_K)      // np.argpartition(-vec, K - 1) in the reference: "kth(=99) out of bounds"
    return fail(MLBP_EINVAL, "mlbp_sweep_f64: approximate inference keeps the %d largest entries; kth(=%d) out of bounds (%d)",
                MLBP_APPROX_K, MLBP_APPROX_K - 1, a->X);
  if (approx && !(a->X > 64 && a->X <= 1024 && a->normalize_messages && !f32_tables))
    return fail(MLBP_EUNSUPPORTED, "mlbp_sweep_f64: batched approximate inference needs 100 <= X <= 1024, normalised messages, float64 tables");
  if (f32_tables && !(a->X == 256 || a->X == 512))
    return fail(MLBP_EUNSUPPORTED, "mlbp_sweep_f64: float32 pairwise tables need X = 256 or 512 (got %d)", a->X);
  if (f32_tables && a->gradient) return fail(MLBP_EUNSUPPORTED, "mlbp_sweep_f64: no gradient with float32 pairwise tables");
  if (int e = mlbp::check_device()) return e;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev != prog->device)
    return fail(MLBP_EINVAL, "mlbp_sweep_f64: the program was created on device %d, the calling thread's current device is %d",
                prog->device, dev);
  if (a->marginals && !prog->d_readout)
    return fail(MLBP_EINVAL, "mlbp_sweep_f64: marginals requested but mlbp_program_set_readout was not called");
  if (a->posterior && (!a->marginals || !a->posterior->labels || !a->posterior->out))
    return fail(MLBP_EINVAL, "mlbp_sweep_f64: posterior needs marginals, labels and an output array");
  const mlbp_gradient_args* ga = a->gradient;
  if (ga && (ga->B != a->B || ga->X != a->X || ga->P != prog->P || ga->U != prog->U || ga->n_msgs != prog->n_msgs || ga->msgs != a->msgs))
    return fail(MLBP_EINVAL, "mlbp_sweep_f64: gradient arguments do not describe the same batch");
  if (ga && (ga->flags & MLBP_GRADIENT_APPROX_BELIEFS) && a->X > MLBP_APPROX_BELIEFS_MAX_X)      // (mlbp_gradient_f64's own refusal, before the sweeps)
    return fail(MLBP_EUNSUPPORTED, "mlbp_sweep_f64: approximate beliefs hold both selected messages on chip; X=%d > %d", a->X,
                MLBP_APPROX_BELIEFS_MAX_X);
  return MLBP_OK;
}

// mlbp_gradient_f64 behind the sweeps of a call: a gradient that was given no workspace gets scratch the PROGRAM owns
// (grown by new blocks only), so that the call is safe on its own stream and inside a captured graph
int gradient_behind_sweeps(mlbp_program* prog, const mlbp_gradient_args* ga, void* stream) {
  mlbp_gradient_args g = *ga;
  if (!g.workspace) {
    const int64_t need = mlbp_gradient_workspace_bytes(&g);
    if (need > 0) {
      if (int e = prog->d_gwork.grow(prog, (size_t)need)) return e;
      g.workspace = prog->d_gwork;
      g.workspace_bytes = (int64_t)prog->d_gwork.bytes;
    }
  }
  return mlbp_gradient_f64(&g, stream);
}

// mlbp_sweep_args.posterior by its own launch (no fix-up pass took it)
int posterior_behind_sweeps(const mlbp_program* prog, const mlbp_sweep_args* a, void* stream) {
  const mlbp_posterior_args* pa = a->posterior;
  if (!pa) return MLBP_OK;
  return mlbp_log_posterior_sum_f64(a->marginals, pa->labels, a->B, prog->n_vars, a->X, pa->out, pa->sum_out, stream);
}

// What follows the sweep kernels of a call and was not fused into them, in this order: the marginals, the gradient (behind a
// shared-table epilogue: the flagged graphs' only), the posterior.
struct SweepTail {
  bool marginals = true;       // false: the sweep kernels wrote them
  bool grad_done = false;      // the sweep kernels ran the gradient as their epilogue
  bool grad_flagged = false;   // ... on every graph but the flagged ones
  bool post_done = false;      // the fix-up pass took the posterior
};
int sweep_tail(mlbp_program* prog, const mlbp_sweep_args* a, const SweepTail& t, void* stream) {
  if (a->marginals && t.marginals)
    if (int e = mlbp_marginals_f64(a->msgs, a->B, prog->n_msgs, a->X, prog->n_vars, prog->d_readout, prog->d_readout + prog->n_vars + 1,
                                   a->normalize_messages ? 1 : 0, a->marginals, stream)) return e;
  if (a->gradient && !t.grad_done)
    if (int e = t.grad_flagged ? mlbp::gradient_flagged_only(a->gradient, prog->d_bail, stream) : gradient_behind_sweeps(prog, a->gradient, stream))
      return e;
  return t.post_done ? MLBP_OK : posterior_behind_sweeps(prog, a, stream);
}

// X = 64 with the exact kernel applicable: the shared-table kernel, else the lean kernel (variant 1 and no fast pass run yet),
// then the exact kernel -- on the graphs the fast pass flagged, or on every graph.
int sweep_x64(mlbp_program* prog, const mlbp_sweep_args* a, FastPass pass, int variant, int walk, void* stream) {
  const bool offer_fast = pass == FAST_NONE && variant == 1;      // variant 3: the exact kernel on every graph
  bool launched = false;
  if (offer_fast) {                               // shared-table batches: 16 graphs per workgroup on the matrix cores
    if (int e = mlbp::launch_shared_sweep(prog, a, stream, &launched)) return e;
    if (launched) pass = FAST_SHARED;
  }
  // The gradient runs as the sweep kernels' epilogue when the tables are on chip in BOTH the fast and the exact kernel (a grouped
  // lean launch runs none).  Behind the shared-table kernel's epilogue the fix-up pass keeps its own for the graphs it redoes --
  // or, with more than three pairwise factors, where the exact kernel streams its tables and has no epilogue, the per-graph
  // gradient kernel follows on the flagged graphs only.
  const bool exact_grad = mlbp::exact_kernel_fuses_gradient(prog, a) && pass != FAST_LEAN;
  const bool shared_grad = pass == FAST_SHARED && mlbp::shared_gradient_fused(prog, a);
  SweepTail tail;
  tail.marginals = !a->normalize_messages;        // (normalised: the read-out is the kernels' epilogue)
  tail.grad_done = exact_grad && (pass != FAST_SHARED || shared_grad);
  tail.grad_flagged = shared_grad && !exact_grad;
  if (offer_fast && pass == FAST_NONE) {          // default path: the lean scale-free kernel (mlbp_lean.hip)
    if (int e = mlbp::launch_lean_sweep(prog, a, tail.grad_done, walk, stream, &launched, &g_last_lean_walk)) return e;
    if (launched) pass = FAST_LEAN;
  }
  g_last_kernel = pass == FAST_SHARED ? MLBP_KERNEL_SHARED_MFMA : (pass == FAST_LEAN ? MLBP_KERNEL_LEAN : MLBP_KERNEL_EXACT);
  g_last_fused_gradient = (tail.grad_done || tail.grad_flagged) ? 1 : 0;
  if (int e = mlbp::launch_exact_x64(prog, a, pass != FAST_NONE, tail.grad_done, stream, &tail.post_done)) return e;
  return sweep_tail(prog, a, tail, stream);
}

// Every other state count (and X = 64 graphs too large for the exact kernel's LDS): the lean kernel on zero-padded vectors for
// X < 64, the batched contractions for shared tables at X > 64, the wide kernel, the generic kernel.
int sweep_other_x(mlbp_program* prog, const mlbp_sweep_args* a, int variant, int walk, void* stream) {
  const bool fast = variant == 1;
  bool lean_small = false, launched = false;
  // small state spaces: the lean X = 64 kernel on zero-padded vectors and tables (it starts from uniform messages itself); the
  // graphs it flags are redone by the generic kernel in its fix-up mode
  if (fast && a->X < 64)
    if (int e = mlbp::launch_lean_sweep(prog, a, false, walk, stream, &lean_small, &g_last_lean_walk)) return e;
  if (a->init_messages && !lean_small)
    if (int e = mlbp_init_messages_f64(a->msgs, (int64_t)a->B * prog->n_msgs, a->X, stream)) return e;
  if (fast && !lean_small) {                      // shared tables at a large state space: every contraction one MFMA launch over the batch
    if (int e = mlbp::launch_gemm_sweep(prog, a, stream, &launched)) return e;
    if (launched) g_last_kernel = MLBP_KERNEL_SHARED_GEMM;
  }
  if (!launched && !lean_small) {
    if (int e = mlbp::launch_wide_sweep(prog, a, stream, &launched)) return e;
    if (launched) g_last_kernel = MLBP_KERNEL_WIDE;
  }
  if (!launched) {
    g_last_kernel = lean_small ? MLBP_KERNEL_LEAN : MLBP_KERNEL_GENERIC;
    if (int e = mlbp::launch_generic_sweep(prog, a, lean_small, stream)) return e;
  }
  return sweep_tail(prog, a, SweepTail(), stream);
}

// One sweep call of (prog, a) -- checked; prog the program it runs -- behind `pass` (FAST_NONE: the call runs its own).
// variant, walk: mlbp_set_sweep_variant's and mlbp_set_lean_walk's, read once per public call.
int run_sweep(mlbp_program* prog, const mlbp_sweep_args* a, FastPass pass, int variant, int walk, void* stream) {
  g_last_fused_gradient = 0;
  if (mlbp::exact_x64_applies(prog, a)) return sweep_x64(prog, a, pass, variant, walk, stream);
  return sweep_other_x(prog, a, variant, walk, stream);
}

// Behind launch_shared_groups: every member's fix-up pass in ONE launch (and, when the call carries gradients, one launch of
// the per-graph gradient kernel over the flagged graphs of all members), then each member's posterior by its own launch.
// *done false: some member needs the per-group path (launch_exact_x64_groups says which).
int finish_shared_groups(mlbp_program* const* progs, const mlbp_sweep_args* args, int n_groups, const std::vector<char>& member,
                         void* stream, bool* done) {
  *done = false;
  if (int e = mlbp::launch_exact_x64_groups(progs, args, n_groups, member, stream, done)) return e;
  if (!*done) return MLBP_OK;
  std::vector<mlbp_gradient_args> grads;
  std::vector<const uint8_t*> grad_flags;
  for (int k = 0; k < n_groups; ++k)
    if (member[k] && args[k].gradient) { grads.push_back(*args[k].gradient); grad_flags.push_back(progs[k]->d_bail); }
  if (!grads.empty())
    if (int e = mlbp::gradient_flagged_groups(grads.data(), grad_flags.data(), (int)grads.size(), progs[0], stream)) return e;
  SweepTail tail;                                 // (the marginals are the kernels' epilogue, the gradient is done above)
  tail.marginals = false;
  tail.grad_done = true;
  for (int k = 0; k < n_groups; ++k)
    if (member[k])
      if (int e = sweep_tail(progs[k], &args[k], tail, stream)) return e;
  g_last_kernel = MLBP_KERNEL_SHARED_MFMA;
  g_last_fused_gradient = grads.empty() ? 0 : 1;
  return MLBP_OK;
}

}  // namespace

extern "C" {

int mlbp_sweep_f64(const mlbp_program* handle, const mlbp_sweep_args* a, void* stream) {
  g_last_fused_gradient = 0;
  if (!handle || !a) return fail(MLBP_EINVAL, "mlbp_sweep_f64: NULL program or args");
  // (the handle is const in the ABI; a call updates the program's scratch and redo flags: one stream at a time per program)
  mlbp_program* prog = effective_program(const_cast<mlbp_program*>(handle), a);
  if (int e = check_sweep_args(prog, a)) return e;
  return run_sweep(prog, a, FAST_NONE, g_sweep_variant, g_lean_walk, stream);
}

int mlbp_sweep_groups_f64(const mlbp_program* const* handles, const mlbp_sweep_args* args, int32_t n_groups, void* stream) {
  if (!handles || !args || n_groups < 1) return fail(MLBP_EINVAL, "mlbp_sweep_groups_f64: bad arguments");
  std::vector<mlbp_program*> eff(n_groups);
  for (int k = 0; k < n_groups; ++k) {
    if (!handles[k]) return fail(MLBP_EINVAL, "mlbp_sweep_groups_f64: NULL program");
    eff[k] = effective_program(const_cast<mlbp_program*>(handles[k]), &args[k]);
    if (int e = check_sweep_args(eff[k], &args[k])) return e;
  }
  mlbp_program* const* progs = eff.data();
  const int variant = g_sweep_variant, walk = g_lean_walk;
  // The fast kernels take what they can, in this order: the shared-table launch sequence, then one grouped lean launch over the
  // groups left; each is followed by the fix-up pass over the graphs it flagged.  The rest run one after the other exactly as
  // separate calls would.  A program joins one grouped launch at most (with its first group): two groups would share one set of
  // redo flags and scratch -- the later one runs as a separate call behind the grouped launches.
  std::vector<char> shared(n_groups, 0), lean(n_groups, 0);
  if (variant == 1) {
    std::vector<char> first(n_groups);
    for (int k = 0; k < n_groups; ++k) first[k] = std::find(progs, progs + k, progs[k]) == progs + k;
    shared = first;
    if (int e = mlbp::launch_shared_groups(progs, args, n_groups, stream, shared)) return e;
    // the shared-table kernels have run every member, gradient included: ONE fix-up launch for the flagged graphs of all members
    // and one more for their gradients (a mixed minibatch used to pay both per group)
    if (std::find(shared.begin(), shared.end(), 1) != shared.end()) {
      bool done = false;
      if (int e = finish_shared_groups(progs, args, n_groups, shared, stream, &done)) return e;
      for (int k = 0; k < n_groups && !done; ++k)
        if (shared[k])
          if (int e = run_sweep(progs[k], &args[k], FAST_SHARED, variant, walk, stream)) return e;
    }
    for (int k = 0; k < n_groups; ++k) lean[k] = first[k] && !shared[k];      // (lean_plan takes no pairwise-free group)
    if (int e = mlbp::launch_lean_groups(progs, args, n_groups, walk, stream, lean, &g_last_lean_walk)) return e;
    for (int k = 0; k < n_groups; ++k)
      if (lean[k])
        if (int e = run_sweep(progs[k], &args[k], FAST_LEAN, variant, walk, stream)) return e;
  }
  for (int k = 0; k < n_groups; ++k)
    if (!shared[k] && !lean[k])
      if (int e = run_sweep(progs[k], &args[k], FAST_NONE, variant, walk, stream)) return e;
  return MLBP_OK;
}

int mlbp_set_sweep_variant(int32_t variant) {
  const bool known = variant == 1 || variant == 3;
  if (!known) return fail(MLBP_EINVAL, "unknown sweep variant %d", variant);
  g_sweep_variant = variant;
  return MLBP_OK;
}

int mlbp_set_lean_walk(int32_t mode) {
  if (mode < 0 || mode > 2) return fail(MLBP_EINVAL, "unknown lean walk mode %d (0 forward, 1 backward, 2 alternate)", mode);
  g_lean_walk = mode;
  return MLBP_OK;
}
int mlbp_lean_walk(void) { return g_lean_walk; }
int mlbp_last_lean_walk(void) { return g_last_lean_walk; }

int mlbp_last_sweep_kernel(void) { return g_last_kernel; }
int mlbp_last_sweep_fused_gradient(void) { return g_last_fused_gradient; }

}  // extern "C"
