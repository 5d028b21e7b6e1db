// The host side of the lean X = 64 sweep kernel (mlbp_lean_device.h): whether it applies to a call (lean_plan), the choice of
// the compiled instance (pick_lean), and the single and the grouped launch.
#include <hip/hip_runtime.h>

#include <vector>

#include "mlbp_lean_device.h"
#include "mlbp_internal.h"

using mlbp::fail;

namespace mlbp {

size_t lean_lds_bytes(const mlbp_program* prog, bool grad, bool padx) {
  const LeanProgram& lp = prog->lean;
  const int n_ext = 2 + lp.n_cprod;               // uniform, the constant products, ones
  size_t lds = ((size_t)(prog->n_msgs + n_ext) * 64 + 4 * 256) * sizeof(double) + 16 * (size_t)(lp.n_bundles + 1) * sizeof(int32_t);
  if (prog->P == 7 && !padx) lds += 32 * 1024;    // the seventh table lives in LDS
  if (grad) lds += 5 * (size_t)prog->U * sizeof(int32_t);
  return lds;
}

// Does the lean kernel apply to this (program, arguments) pair?  Fills the device-side descriptions when it does.
// grad: the call's gradient is fused into the launch (the caller has checked that it can be); a gradient request without
// it is served by the standalone kernel afterwards, from the messages in memory.
static int lean_plan(mlbp_program* prog, const mlbp_sweep_args* a, bool grad, bool* ok, SweepDev* d, LeanDev* f, size_t* lds) {
  *ok = false;
  const LeanProgram& lp = prog->lean;
  if (!lp.ok || !prog->d_limage || a->X > 64 || a->X < 2 || !a->normalize_messages || prog->P < 1 || prog->P > 8) return MLBP_OK;
  const bool padx = a->X < 64;
  if (padx && prog->P > 4) return MLBP_OK;
  if (a->gradient && padx) return MLBP_OK;
  if (grad && (prog->P > 3 || prog->U > WG)) return fail(MLBP_EINVAL, "lean kernel: fused gradient needs P <= 3 and U <= %d", WG);
  if (a->flags & MLBP_SWEEP_APPROX_INFERENCE) return MLBP_OK;
  if (a->marginals && !prog->d_lreadout && !padx) return MLBP_OK;
  const int n_ext = 2 + lp.n_cprod;               // uniform, the constant products, ones
  *lds = lean_lds_bytes(prog, grad, padx);
  if (*lds > 80 * 1024) return MLBP_OK;           // large graphs: the generic kernel's rules apply
  if (prog->P + prog->U > WG) return MLBP_OK;     // the dense-layout check is one index word per thread
  const bool dense = (a->flags & MLBP_SWEEP_DENSE_TABLES) != 0;
  if (dense && ((int64_t)a->B * prog->P > a->n_pair_tables || (int64_t)a->B * prog->U > a->n_unary_tables))
    return fail(MLBP_EINVAL, "mlbp_sweep_f64: MLBP_SWEEP_DENSE_TABLES needs B*P pair tables and B*U unary columns");
  if (prog->d_bail.bytes < (size_t)a->B)
    if (int e = mlbp_program_reserve(prog, a->B)) return e;
  d->pair_tables = a->pair_tables; d->pair_tab = a->pair_tab;
  d->unary_tables = a->unary_tables; d->unary_tab = a->unary_tab;
  d->msgs = a->msgs;
  d->ops = nullptr; d->srcs = nullptr; d->sweeps = nullptr; d->pairseq = nullptr;
  d->status = prog->d_status;
  d->n_sweeps = prog->n_sweeps; d->n_msgs = prog->n_msgs; d->P = prog->P; d->U = prog->U; d->X = a->X;
  d->n_pair_tables = a->n_pair_tables; d->n_unary_tables = a->n_unary_tables;
  d->marginals = padx ? nullptr : a->marginals; d->readout = nullptr; d->n_vars = prog->n_vars;
  d->only = nullptr; d->fill_uniform = 0; d->approx_k = 0;
  f->image = prog->d_limage; f->readout = (a->marginals && !padx) ? prog->d_lreadout : nullptr; f->bail = prog->d_bail;
  f->n_bundles = lp.n_bundles; f->HL = lp.HL; f->n_cprod = lp.n_cprod; f->WL = lp.WL;
  f->n_ext = n_ext; f->init = a->init_messages; f->dense = dense ? 1 : 0;
  // the messages go back to memory unless the caller waives them and takes the fused read-outs instead (a gradient that
  // is NOT fused reads them from memory)
  const bool waived = (a->flags & MLBP_SWEEP_NO_MESSAGE_WRITEBACK) && !padx && (a->marginals || grad) && (!a->gradient || grad);
  f->keep = waived ? 0 : 1;                       // (small X: the read-out is a separate launch over the messages)
  f->walk = -1;                                   // (the launch sets it: lean_walk_word)
  *ok = true;
  return MLBP_OK;
}

typedef void (*lean_fn)(SweepDev, LeanDev, const int32_t*, int, GradFusedDev);

// The direction of the next lean launch of `prog` (LeanDev::walk) under mlbp_set_lean_walk's mode, and -- behind the launch --
// the turn: in mode 2 consecutive launches of a program walk its batch in opposite directions, so the graphs at the turn are
// wanted again while the last-level cache still holds them.  The direction is a kernel argument: a captured launch keeps its own.
static int lean_walk_of(const mlbp_program* prog, int mode) { return mode == 2 ? prog->lean_walk_next : mode; }
static int32_t lean_walk_word(int dir, int n_graphs) { return dir ? n_graphs - 1 : -1; }      // LeanDev::walk of a launch of n_graphs
static void lean_walk_turn(mlbp_program* prog, int mode) { if (mode == 2) prog->lean_walk_next ^= 1; }

template <bool MULTI>
static lean_fn pick_lean(int P, bool padx) {
  if constexpr (!MULTI) {       // (a grouped launch is X = 64 only: launch_lean_groups never pads)
    if (padx) {
      switch (P) {
        case 1: return sweep_x64_lean_kernel<1, true, false, 0, false>;
        case 2: return sweep_x64_lean_kernel<2, true, false, 0, false>;
        case 3: return sweep_x64_lean_kernel<3, true, false, 0, false>;
        default: return sweep_x64_lean_kernel<4, true, false, 0, false>;
      }
    }
  }
  switch (P) {
    case 1: return sweep_x64_lean_kernel<1, false, MULTI, 0, false>;
    case 2: return sweep_x64_lean_kernel<2, false, MULTI, 0, false>;
    case 3: return sweep_x64_lean_kernel<3, false, MULTI, 0, false>;
    case 4: return sweep_x64_lean_kernel<4, false, MULTI, 0, false>;
    case 5: case 6: return sweep_x64_lean_kernel<6, false, MULTI, 0, false>;
    case 7: return sweep_x64_lean_kernel<6, false, MULTI, 1, false>;     // six tables in registers, the seventh in LDS: two workgroups per CU
    default: return sweep_x64_lean_kernel<8, false, MULTI, 0, false>;    // part of the tables lives in the accumulator registers
  }
}
static lean_fn pick_lean_grad(int P) {
  switch (P) {
    case 1: return sweep_x64_lean_kernel<1, false, false, 0, true>;
    case 2: return sweep_x64_lean_kernel<2, false, false, 0, true>;
    default: return sweep_x64_lean_kernel<3, false, false, 0, true>;
  }
}

int launch_lean_sweep(mlbp_program* prog, const mlbp_sweep_args* a, bool fuse_gradient, int walk_mode, void* stream, bool* launched,
                      int* walk) {
  *launched = false;
  SweepDev d;
  LeanDev f;
  size_t lds = 0;
  bool ok = false;
  if (int e = lean_plan(prog, a, fuse_gradient, &ok, &d, &f, &lds)) return e;
  if (!ok) return MLBP_OK;
  const int dir = lean_walk_of(prog, walk_mode);
  f.walk = lean_walk_word(dir, a->B);
  GradFusedDev gf = {};
  if (fuse_gradient) fill_grad_fused(a->gradient, &gf);
  // a single, non-gradient X = 64 call of a three-table program: the program's static kernel (mlbp_lean_jit.cpp) when it has
  // one -- the same kernel with the micro-ops compiled in, the same arguments, grid and LDS
  if (!fuse_gradient && a->X == 64 && prog->P == 3) {
    lean_jit_auto(prog, a->B, stream);
    if (prog->jit.state == 1) {
      void* params[] = {&d, &f};
      launch_begin();
      launch_log_record(prog->jit.function);
      HIP_TRY(hipModuleLaunchKernel((hipFunction_t)prog->jit.function, a->B, 1, 1, WG, 1, 1, (unsigned)lds, (hipStream_t)stream, params, nullptr));
      if (int e = launch_verdict("static lean sweep")) return e;
      lean_walk_turn(prog, walk_mode);
      *walk = dir;
      *launched = true;
      return MLBP_OK;
    }
  }
  lean_fn k = fuse_gradient ? pick_lean_grad(prog->P) : pick_lean<false>(prog->P, a->X < 64);
  if (int e = grant_lds((const void*)k, lds)) return e;
  launch_begin();
  MLBP_LAUNCH(k, dim3(a->B), dim3(WG), lds, (hipStream_t)stream, d, f, nullptr, 0, gf);
  if (int e = launch_verdict("lean sweep")) return e;
  lean_walk_turn(prog, walk_mode);
  *walk = dir;
  *launched = true;
  return MLBP_OK;
}

// Several (program, arguments) groups in ONE launch of the lean kernel.  member: in, the groups offered (distinct programs);
// out, the groups the launch runs -- those the kernel takes that make the same init / write-back / read-out choices as the first
// of them (none: nothing is launched).  The group table lives in a device buffer owned by the FIRST program of the call (like
// its redo flags: one stream at a time per program) and is uploaded only when its contents differ from the last call's, so a
// repeated call -- the trainer's every step -- is enqueue-only and can be captured into a HIP graph after one warm-up call.
// The launch walks in the FIRST program's direction (mlbp_set_lean_walk) and turns that program alone.  *walk: the direction
// launched, left alone when nothing is.
int launch_lean_groups(mlbp_program* const* progs, const mlbp_sweep_args* args, int n_groups, int walk_mode, void* stream,
                       std::vector<char>& member, int* walk) {
  std::vector<int32_t> table;
  size_t lds_max = 0;
  int p_max = 0, total = 0, n_in = 0;
  SweepDev d0;
  LeanDev f0;
  for (int k = 0; k < n_groups; ++k) {
    if (!member[k]) continue;
    member[k] = 0;
    if (args[k].X != 64) continue;
    SweepDev d;
    LeanDev f;
    size_t lds = 0;
    bool ok = false;
    if (int e = lean_plan(progs[k], &args[k], false, &ok, &d, &f, &lds)) return e;
    if (!ok) continue;
    if (n_in == 0) { d0 = d; f0 = f; }
    else if (f.init != f0.init || f.keep != f0.keep || (f.readout != nullptr) != (f0.readout != nullptr)) continue;
    member[k] = 1;
    ++n_in;
    lds_max = std::max(lds_max, lds + (progs[k]->P < 7 ? 32 * 1024 : 0));      // (a 7-table group may sit beside it: its LDS table)
    p_max = std::max(p_max, (int)progs[k]->P);
    table.resize(table.size() + GROUP_WORDS, 0);
    int32_t* w = &table[table.size() - GROUP_WORDS];
    auto put = [&](int at, const void* p) { const uintptr_t v = (uintptr_t)p; w[at] = (int32_t)(uint32_t)v; w[at + 1] = (int32_t)(uint32_t)(v >> 32); };
    w[0] = total; w[1] = args[k].B;
    put(2, f.image); put(4, f.readout); put(6, f.bail); put(8, d.msgs); put(10, d.marginals); put(12, d.pair_tables);
    put(14, d.pair_tab); put(16, d.unary_tables); put(18, d.unary_tab); put(20, d.status);
    w[22] = f.n_bundles; w[23] = f.HL; w[24] = f.n_cprod; w[25] = f.WL; w[26] = f.n_ext; w[27] = d.n_msgs; w[28] = d.P; w[29] = d.U;
    w[30] = d.n_vars; w[31] = d.n_pair_tables; w[32] = d.n_unary_tables; w[33] = f.dense;
    total += args[k].B;
  }
  if (n_in == 0) return MLBP_OK;
  // one device copy per distinct table (stream-ordered upload on first sight, none afterwards): a captured graph keeps its own
  int32_t* d_gtable = nullptr;
  if (int e = group_table_device(progs[0]->gtables, table, stream, &d_gtable)) return e;
  lean_fn k = pick_lean<true>(p_max, false);
  if (int e = grant_lds((const void*)k, lds_max)) return e;
  const int dir = lean_walk_of(progs[0], walk_mode);
  f0.walk = lean_walk_word(dir, total);
  launch_begin();
  MLBP_LAUNCH(k, dim3(total), dim3(WG), lds_max, (hipStream_t)stream, d0, f0, d_gtable, n_in, GradFusedDev{});
  if (int e = launch_verdict("grouped lean sweep")) return e;
  lean_walk_turn(progs[0], walk_mode);
  *walk = dir;
  return MLBP_OK;
}

}  // namespace mlbp
