// Everything of libmlbp.so that creates, owns, grows and frees device memory: the mlbp_program life cycle, the program-owned
// scratch (DeviceArray, mlbp_internal.h), the group-table cache, the process-wide fallback arena and status word, and the two
// small launch services every kernel file uses (grant_lds, launch_begin / launch_verdict).  Host code only: no kernel here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <utility>
#include <vector>

#include "mlbp_internal.h"

using mlbp::fail;

namespace mlbp {

int check_device() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    return fail(MLBP_ENODEVICE, "no HIP device visible: libmlbp.so has no CPU fallback");
  }
  return MLBP_OK;
}

// the status word of the kernels that have no program attached (mlbp_gradient_status)
static int32_t* g_status = nullptr;
int status_word(int32_t** out) {
  if (!g_status) {
    HIP_TRY(hipMalloc(&g_status, sizeof(int32_t)));
    HIP_TRY(hipMemset(g_status, 0, sizeof(int32_t)));
  }
  *out = g_status;
  return MLBP_OK;
}

int status_word_read() {
  if (!g_status) return 0;
  int32_t v = 0, zero = 0;
  HIP_TRY(hipMemcpy(&v, g_status, sizeof(v), hipMemcpyDeviceToHost));
  if (v) HIP_TRY(hipMemcpy(g_status, &zero, sizeof(zero), hipMemcpyHostToDevice));
  return v;
}

void device_release(void* p) {
  if (p) (void)hipFree(p);
}

int device_grow(mlbp_program* owner, void** p, size_t* bytes, size_t need, bool zero) {
  if (need <= *bytes && *p) return MLBP_OK;
  void* fresh = nullptr;
  if (hipMalloc(&fresh, need ? need : 1) != hipSuccess) return fail(MLBP_EHIP, "program scratch: allocation of %zu bytes failed", need);
  if (zero && hipMemset(fresh, 0, need) != hipSuccess) { (void)hipFree(fresh); return fail(MLBP_EHIP, "program scratch: memset failed"); }
  if (*p) {                                 // a captured graph may still name it: freed with the program
    owner->retired.emplace_back();
    owner->retired.back().p = static_cast<char*>(*p);
    owner->retired.back().bytes = *bytes;
  }
  *p = fresh;
  *bytes = need;
  return MLBP_OK;
}

int device_upload(const char* what, void** p, size_t* bytes, const void* src, size_t n_bytes) {
  device_release(*p);
  *p = nullptr;
  *bytes = 0;
  hipError_t e = hipMalloc(p, n_bytes ? n_bytes : 1);
  if (e == hipSuccess && n_bytes) e = hipMemcpy(*p, src, n_bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) return fail(MLBP_EHIP, "%s: device upload failed: %s", what, hipGetErrorString(e));
  *bytes = n_bytes ? n_bytes : 1;
  return MLBP_OK;
}

int grant_lds(const void* kernel, size_t bytes, bool* fresh) {
  static std::vector<std::pair<const void*, size_t>> granted;
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  if (fresh) *fresh = false;
  auto g = std::find_if(granted.begin(), granted.end(), [&](const std::pair<const void*, size_t>& e) { return e.first == kernel; });
  if (g != granted.end() && g->second >= bytes) return MLBP_OK;
  HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  if (g != granted.end()) g->second = bytes;
  else granted.push_back({kernel, bytes});
  if (fresh) *fresh = true;
  return MLBP_OK;
}

void launch_begin() { (void)hipGetLastError(); }

int launch_verdict(const char* what) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MLBP_OK : fail(MLBP_EHIP, "%s launch failed: %s", what, hipGetErrorString(e));
}

int fallback_scratch(int purpose, size_t bytes, void** out) {
  struct Block { void* p = nullptr; size_t cap = 0; };
  static std::mutex mu;
  static std::vector<std::vector<Block>> per_device;      // [device][purpose]; replaced blocks are never freed (process lifetime)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return fail(MLBP_EHIP, "hipGetDevice failed");
  std::lock_guard<std::mutex> lock(mu);
  if ((int)per_device.size() <= dev) per_device.resize(dev + 1, std::vector<Block>(SCRATCH_PURPOSES));
  Block& b = per_device[dev][purpose];
  if (bytes > b.cap) {
    void* fresh = nullptr;
    const size_t want = bytes > 2 * b.cap ? bytes : 2 * b.cap;
    if (hipMalloc(&fresh, want) != hipSuccess) return fail(MLBP_EHIP, "scratch allocation of %zu bytes failed", want);
    b.p = fresh; b.cap = want;
  }
  *out = b.p;
  return MLBP_OK;
}

int group_table_device(GroupTables& gt, const std::vector<int32_t>& table, void* stream, int32_t** out) {
  for (auto& e : gt.entries)
    if (e.words == table) { *out = e.dev; return MLBP_OK; }
  GroupTables::Entry* slot = nullptr;
  if (gt.entries.size() < (size_t)GroupTables::MAX) { gt.entries.emplace_back(); slot = &gt.entries.back(); }
  else { slot = &gt.entries[gt.next_evict]; gt.next_evict = (gt.next_evict + 1) % GroupTables::MAX; }
  const size_t bytes = table.size() * sizeof(int32_t);
  if (bytes > slot->dev.bytes) {
    int32_t* fresh = nullptr;
    if (hipMalloc(&fresh, bytes) != hipSuccess) return fail(MLBP_EHIP, "group table allocation failed");
    slot->dev.release();                    // (only a recycled slot has one: its table is being replaced anyway)
    slot->dev.p = fresh; slot->dev.bytes = bytes;
  }
  slot->words = table;
  if (hipMemcpyAsync(slot->dev, slot->words.data(), bytes, hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess)
    return fail(MLBP_EHIP, "group table upload failed");
  *out = slot->dev;
  return MLBP_OK;
}

}  // namespace mlbp

static int create_program(const int32_t* ops, int32_t n_ops, const int32_t* srcs, int32_t n_srcs, const int32_t* sweeps, int32_t n_sweeps,
                          int32_t n_msgs, int32_t P, int32_t U, mlbp_program** out, bool with_pruned);

// The device side of a validated program: the op list as given, the three compiled forms, the status word.
static int upload_program(mlbp_program* p, const int32_t* ops, const int32_t* srcs, const int32_t* sweeps, std::vector<int32_t> pairseq) {
  const char* const who = "mlbp_program_create";
  pairseq.push_back(-1);
  std::vector<int32_t> srcs_padded(srcs ? srcs : nullptr, srcs ? srcs + p->n_srcs : nullptr);
  srcs_padded.resize(((size_t)p->n_srcs + 16 + 3) / 4 * 4, 0);   // the fused kernel reads sources 16 at a time
  const int32_t zero = 0;
  const mlbp::FusedProgram& fp = p->fused;
  std::vector<int32_t> image(fp.fops);
  image.insert(image.end(), fp.psrcs.begin(), fp.psrcs.end());
  image.insert(image.end(), fp.hoist.begin(), fp.hoist.end());
  image.insert(image.end(), fp.cpw.begin(), fp.cpw.end());
  image.insert(image.end(), fp.written.begin(), fp.written.end());
  if (int e = p->d_ops.upload(who, ops, (size_t)p->n_ops * 4)) return e;
  if (int e = p->d_srcs.upload(who, srcs_padded.data(), srcs_padded.size())) return e;
  if (int e = p->d_sweeps.upload(who, sweeps, (size_t)p->n_sweeps * 2)) return e;
  if (int e = p->d_pairseq.upload(who, pairseq.data(), pairseq.size())) return e;
  if (int e = p->d_status.upload(who, &zero, 1)) return e;
  if (p->shared.ok)
    if (int e = p->d_simage.upload(who, p->shared.image.data(), p->shared.image.size())) return e;
  if (p->lean.ok)
    if (int e = p->d_limage.upload(who, p->lean.image.data(), p->lean.image.size())) return e;
  if (int e = p->d_fops.upload(who, image.data(), image.size())) return e;
  if (int e = p->d_fsweeps.upload(who, fp.fsweeps.data(), fp.fsweeps.size())) return e;
  return p->d_fpairseq.upload(who, fp.pairseq.data(), fp.pairseq.size());
}

static int create_program(const int32_t* ops, int32_t n_ops, const int32_t* srcs, int32_t n_srcs, const int32_t* sweeps, int32_t n_sweeps,
                          int32_t n_msgs, int32_t P, int32_t U, mlbp_program** out, bool with_pruned) {
  if (!out) return fail(MLBP_EINVAL, "out is NULL");
  *out = nullptr;
  int max_srcs = 0;
  if (int e = mlbp::validate_program(ops, n_ops, srcs, n_srcs, sweeps, n_sweeps, n_msgs, P, U, &max_srcs)) return e;
  std::vector<int32_t> pairseq;
  for (int s = 0; s < n_sweeps; ++s) {
    const int first = sweeps[2 * s], cnt = sweeps[2 * s + 1];
    for (int o = first; o < first + cnt; ++o)
      if (ops[4 * o] == MLBP_OP_PAIR_TM || ops[4 * o] == MLBP_OP_PAIR_MT) pairseq.push_back(ops[4 * o + 1]);
  }
  if (int e = mlbp::check_device()) return e;
  mlbp_program* p = new mlbp_program();
  p->n_ops = n_ops; p->n_srcs = n_srcs; p->n_sweeps = n_sweeps; p->n_msgs = n_msgs; p->P = P; p->U = U;
  p->n_pairseq = (int)pairseq.size();
  p->max_srcs = max_srcs;
  (void)hipGetDevice(&p->device);
  p->h_ops.assign(ops, ops + 4 * (size_t)n_ops);
  p->h_sweeps.assign(sweeps, sweeps + 2 * (size_t)n_sweeps);
  mlbp::FusedProgram& fp = p->fused;
  mlbp::build_fused_program(ops, srcs, sweeps, n_sweeps, n_msgs, fp);
  p->n_fops = (int)fp.fops.size() / 8;
  p->n_hoist = (int)fp.hoist.size() / 2;
  p->n_psrcs = (int)fp.psrcs.size();
  p->n_cprod = fp.n_cprod;
  p->n_cpw = (int)fp.cpw.size();
  p->n_written = (int)fp.written.size();
  p->sf_ok = !fp.has_unary_fops;
  mlbp::build_shared_program(fp, n_msgs, P, U, p->shared);
  mlbp::build_lean_program(fp, n_msgs, p->lean);
  int rc = upload_program(p, ops, srcs, sweeps, std::move(pairseq));
  if (rc == MLBP_OK && with_pruned) {
    std::vector<int32_t> ops2, sweeps2;
    p->n_dropped = mlbp::drop_unchanged_updates(ops, srcs, sweeps, n_sweeps, n_msgs, ops2, sweeps2);
    if (p->n_dropped > 0) {
      rc = create_program(ops2.data(), (int)ops2.size() / 4, srcs, n_srcs, sweeps2.data(), n_sweeps, n_msgs, P, U, &p->pruned, false);
      if (rc == MLBP_OK) p->pruned->is_twin = true;
    }
  }
  if (rc != MLBP_OK) {
    mlbp_program_destroy(p);
    return rc;
  }
  *out = p;
  return MLBP_OK;
}

// Uploads the shared-table read-out image and notes what the product-fused read-outs need to know about it.
static int set_shared_readout(mlbp_program* p, int32_t n_vars, const int32_t* in_off, const int32_t* in_slots) {
  p->d_sreadout.release();
  p->n_sreadout = 0;
  p->sreadout_all_based = false; p->sreadout_all_tiled = false;
  std::vector<int32_t> simg;
  if (!(p->shared.ok && mlbp::build_shared_readout(p->shared, p->n_msgs, n_vars, in_off, in_slots, simg))) return MLBP_OK;
  p->sreadout_all_based = true; p->sreadout_all_tiled = true;
  for (int v = 0; v < n_vars; ++v) {
    p->sreadout_all_based &= simg[simg[v]] >= 0;
    p->sreadout_all_tiled &= simg[simg[v] + 1] >= 1;       // (the three-source product-fused read-out stages a variable's rows in its first message tile)
    for (int u = 0; u < v; ++u) p->sreadout_all_based &= simg[simg[u]] != simg[simg[v]];      // (and its own: the read-out stages a variable's rows there)
  }
  if (int e = p->d_sreadout.upload("mlbp_program_set_readout", simg.data(), simg.size())) return e;
  p->n_sreadout = (int)simg.size();
  return MLBP_OK;
}

extern "C" {

int mlbp_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

int mlbp_program_create(const int32_t* ops, int32_t n_ops, const int32_t* srcs, int32_t n_srcs,
                        const int32_t* sweeps, int32_t n_sweeps, int32_t n_msgs, int32_t P, int32_t U,
                        mlbp_program** out) {
  return create_program(ops, n_ops, srcs, n_srcs, sweeps, n_sweeps, n_msgs, P, U, out, true);
}

int mlbp_program_destroy(mlbp_program* p) {
  if (!p) return MLBP_OK;
  if (p->pruned) (void)mlbp_program_destroy(p->pruned);
  mlbp::lean_jit_release(p);
  if (p->side_stream) (void)hipStreamDestroy((hipStream_t)p->side_stream);
  if (p->ev_fork) (void)hipEventDestroy((hipEvent_t)p->ev_fork);
  if (p->ev_join) (void)hipEventDestroy((hipEvent_t)p->ev_join);
  delete p;                                  // every device block is a DeviceArray member
  return MLBP_OK;
}

int mlbp_program_reserve(mlbp_program* p, int32_t max_graphs) {
  if (!p || max_graphs <= 0) return fail(MLBP_EINVAL, "mlbp_program_reserve: bad arguments");
  if (p->pruned)
    if (int e = mlbp_program_reserve(p->pruned, max_graphs)) return e;
  // (cleared: mlbp_program_exact_count before any fast-path launch reads 0)
  return p->d_bail.grow(p, (size_t)max_graphs, true);
}

int mlbp_program_set_readout(mlbp_program* p, int32_t n_vars, const int32_t* in_off, const int32_t* in_slots) {
  const char* const who = "mlbp_program_set_readout";
  if (!p || n_vars <= 0 || !in_off || !in_slots) return fail(MLBP_EINVAL, "mlbp_program_set_readout: bad arguments");
  if (in_off[0] != 0) return fail(MLBP_EINVAL, "in_off[0] must be 0");
  for (int v = 0; v < n_vars; ++v)
    if (in_off[v + 1] < in_off[v]) return fail(MLBP_EINVAL, "in_off must be non-decreasing");
  const int n_in = in_off[n_vars];
  for (int q = 0; q < n_in; ++q)
    if (in_slots[q] < 0 || in_slots[q] >= p->n_msgs) return fail(MLBP_EINVAL, "in_slots[%d] = %d out of [0,%d)", q, in_slots[q], p->n_msgs);
  if (p->pruned)
    if (int e = mlbp_program_set_readout(p->pruned, n_vars, in_off, in_slots)) return e;
  std::vector<int32_t> img(in_off, in_off + n_vars + 1);
  img.insert(img.end(), in_slots, in_slots + n_in);
  img.push_back(0);
  if (int e = p->d_readout.upload(who, img.data(), img.size())) return e;
  p->n_vars = n_vars;
  p->n_readout = (int)img.size();
  p->d_lreadout.release();
  std::vector<int32_t> limg;
  if (p->lean.ok && mlbp::build_lean_readout(p->lean, p->n_msgs, n_vars, in_off, in_slots, limg))
    if (int e = p->d_lreadout.upload(who, limg.data(), limg.size())) return e;
  return set_shared_readout(p, n_vars, in_off, in_slots);
}

int mlbp_program_exact_count(const mlbp_program* prog, int32_t B) {
  // Synchronising: how many of the first B graphs of the last default-variant launch were handed
  // to the exact kernel (0 when the scale-free kernel was not used).
  if (!prog || B < 0) return fail(MLBP_EINVAL, "mlbp_program_exact_count: bad arguments");
  if (prog->last_was_pruned && prog->pruned) prog = prog->pruned;
  if (!prog->d_bail || B == 0) return 0;
  if ((size_t)B > prog->d_bail.bytes) B = (int32_t)prog->d_bail.bytes;
  std::vector<unsigned char> h((size_t)B);
  HIP_TRY(hipMemcpy(h.data(), prog->d_bail, (size_t)B, hipMemcpyDeviceToHost));
  int n = 0, hist[4] = {0, 0, 0, 0};
  for (unsigned char c : h) { n += c ? 1 : 0; hist[c & 3]++; }
  fail(0, "exact-kernel graphs by reason: prologue %d, main loop %d, final pass %d (shared-table kernel: 2 = degenerate total, 4 -> counted under 0 = tables not shared)", hist[1], hist[2], hist[3]);
  return n;
}

int mlbp_program_bail_codes(const mlbp_program* prog, int32_t B, uint8_t* out) {
  // Synchronising: the flag bytes themselves, of the program the last call ran
  if (!prog || B < 0 || (B > 0 && !out)) return fail(MLBP_EINVAL, "mlbp_program_bail_codes: bad arguments");
  if (prog->last_was_pruned && prog->pruned) prog = prog->pruned;
  if ((size_t)B > prog->d_bail.bytes) B = (int32_t)prog->d_bail.bytes;
  if (!prog->d_bail || B == 0) return 0;
  HIP_TRY(hipMemcpy(out, prog->d_bail, (size_t)B, hipMemcpyDeviceToHost));
  return B;
}

int mlbp_program_status(const mlbp_program* prog) {
  // Synchronising read of the status word: 0 = clean, 1 = a kernel skipped a graph because a
  // table index was out of range.  Resets the word.
  if (!prog) return fail(MLBP_EINVAL, "NULL program");
  int32_t v = 0, zero = 0;
  HIP_TRY(hipMemcpy(&v, prog->d_status, sizeof(v), hipMemcpyDeviceToHost));
  if (v) HIP_TRY(hipMemcpy(prog->d_status, &zero, sizeof(zero), hipMemcpyHostToDevice));
  if (prog->pruned) {
    const int w = mlbp_program_status(prog->pruned);
    if (w < 0) return w;
    v |= w;
  }
  return v;
}

int mlbp_program_skippable_updates(const mlbp_program* prog) {
  if (!prog) return fail(MLBP_EINVAL, "NULL program");
  return prog->n_dropped;
}

}  // extern "C"
