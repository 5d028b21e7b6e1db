// Host helpers shared by the side libraries (libmlbp_map.so, libmlbp_logz.so, libmlbp_sample.so, libmlbp_converge.so,
// libmlbp_cutset.so, libmlbp_exactmap.so): the
// thread's last error, the index checks of a sweep program and of the read-out arrays, the argument checks every compute
// entry starts with, and the LDS grant of the X = 64 kernels.  Each library is one translation unit, so everything here is in
// the anonymous namespace: each .so has its own g_last_error.  Not part of the ABI.
// Include after the library's public header (status codes and op kinds come from there; a library that runs no sweep program
// defines MLBP_GRAPH_NO_SWEEPS first and gets everything but the program check).  The first part is plain C++ and
// compiles without HIP (a host-only program can feed the index checks malformed programs); the second needs the HIP runtime.
#ifndef MLBP_GRAPH_HOST_H
#define MLBP_GRAPH_HOST_H

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>

namespace {

thread_local std::string g_last_error = "";

int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}

// ---- index checks: plain C++ ---------------------------------------------------------------------
// The per_op / per_var of a library that adds nothing.
struct NoMoreChecks {
  template <class... A>
  int operator()(A...) const { return MLBP_OK; }
};

// The arrays and sizes of a program, as every check_program but the sampler's words them (its sizes include n_vars).
inline int check_program_sizes(const int32_t* ops, int32_t n_ops, const int32_t* srcs, int32_t n_srcs, const int32_t* sweeps,
                               int32_t n_sweeps, int32_t n_msgs, int32_t P, int32_t U) {
  if (!ops || !sweeps) return fail(MLBP_EINVAL, "program: ops or sweeps is NULL");
  if (n_ops <= 0 || n_sweeps <= 0 || n_msgs <= 0 || P < 0 || U < 0 || n_srcs < 0 || (n_srcs > 0 && !srcs))
    return fail(MLBP_EINVAL, "program: bad sizes (n_ops %d, n_sweeps %d, n_msgs %d, P %d, U %d, n_srcs %d) or srcs is NULL", n_ops,
                n_sweeps, n_msgs, P, U, n_srcs);
  return MLBP_OK;
}

#ifndef MLBP_GRAPH_NO_SWEEPS
// Every index of every op, then every sweep's op range.  per_op(o, kind, c) runs behind the checks of op o and adds the
// library's own (0: fine).  The sizes have been checked.  (The range ends are formed in 64 bits: first + count may pass INT_MAX.)
template <class PerOp>
int check_program_indices(const int32_t* ops, int32_t n_ops, const int32_t* srcs, int32_t n_srcs, const int32_t* sweeps,
                          int32_t n_sweeps, int32_t n_msgs, int32_t P, int32_t U, PerOp per_op) {
  for (int o = 0; o < n_ops; ++o) {
    const int kind = ops[4 * o], a = ops[4 * o + 1], b = ops[4 * o + 2], c = ops[4 * o + 3];
    if (c < 0 || c >= n_msgs) return fail(MLBP_EINVAL, "op %d: destination slot %d out of [0,%d)", o, c, n_msgs);
    switch (kind) {
      case MLBP_OP_UNARY:
        if (a < 0 || a >= U) return fail(MLBP_EINVAL, "op %d: unary slot %d out of [0,%d)", o, a, U);
        break;
      case MLBP_OP_PAIR_TM:
      case MLBP_OP_PAIR_MT:
        if (a < 0 || a >= P) return fail(MLBP_EINVAL, "op %d: pair slot %d out of [0,%d)", o, a, P);
        if (b < 0 || b >= n_msgs) return fail(MLBP_EINVAL, "op %d: source slot %d out of [0,%d)", o, b, n_msgs);
        if (b == c) return fail(MLBP_EINVAL, "op %d: source and destination slot coincide", o);
        break;
      case MLBP_OP_VAR:
        if (a < 0 || b < 0 || (int64_t)a + b > n_srcs) return fail(MLBP_EINVAL, "op %d: srcs range [%d,%lld) out of [0,%d)", o, a, (long long)a + b, n_srcs);
        for (int q = a; q < a + b; ++q)
          if (srcs[q] < 0 || srcs[q] >= n_msgs) return fail(MLBP_EINVAL, "op %d: source slot %d out of [0,%d)", o, srcs[q], n_msgs);
        break;
      default:
        return fail(MLBP_EINVAL, "op %d: unknown kind %d", o, kind);
    }
    if (int e = per_op(o, kind, c)) return e;
  }
  for (int s = 0; s < n_sweeps; ++s) {
    const int first = sweeps[2 * s], cnt = sweeps[2 * s + 1];
    if (first < 0 || cnt < 0 || (int64_t)first + cnt > n_ops)
      return fail(MLBP_EINVAL, "sweep %d: op range [%d,%lld) out of [0,%d)", s, first, (long long)first + cnt, n_ops);
  }
  return MLBP_OK;
}
#endif

inline int check_in_slots_present(const int32_t* in_off, const int32_t* in_slots) {
  if (!in_off || !in_slots) return fail(MLBP_EINVAL, "read-out: in_off or in_slots is NULL");
  return MLBP_OK;
}

// The walk over every variable's in-slots.  per_var(v) runs once in_off[v] <= in_off[v + 1] is known and before the slots of v
// are read (0: fine).  The arrays are there and n_vars, n_msgs positive.
template <class PerVar>
int check_in_slots(int32_t n_vars, const int32_t* in_off, const int32_t* in_slots, int32_t n_msgs, PerVar per_var) {
  if (in_off[0] != 0) return fail(MLBP_EINVAL, "read-out: in_off[0] must be 0");
  for (int v = 0; v < n_vars; ++v) {
    if (in_off[v + 1] < in_off[v]) return fail(MLBP_EINVAL, "read-out: in_off not monotone at variable %d", v);
    if (int e = per_var(v)) return e;
    for (int q = in_off[v]; q < in_off[v + 1]; ++q)
      if (in_slots[q] < 0 || in_slots[q] >= n_msgs) return fail(MLBP_EINVAL, "read-out: variable %d: slot %d out of [0,%d)", v, in_slots[q], n_msgs);
  }
  return MLBP_OK;
}

// check_readout of a library whose read-out is the in-slots alone.
inline int check_readout_in_slots(int32_t n_vars, const int32_t* in_off, const int32_t* in_slots, int32_t n_msgs) {
  if (int e = check_in_slots_present(in_off, in_slots)) return e;
  if (n_vars <= 0 || n_msgs <= 0) return fail(MLBP_EINVAL, "read-out: bad sizes (n_vars %d, n_msgs %d)", n_vars, n_msgs);
  return check_in_slots(n_vars, in_off, in_slots, n_msgs, NoMoreChecks());
}

// ---- the argument checks of a compute entry, over the library's args struct (the field names agree) --------------
// They come in the order the entries run them; an entry puts its own between them.
template <class Args>
int check_args_sizes(const Args* a) {
  if (!a) return fail(MLBP_EINVAL, "args is NULL");
  if (a->B <= 0 || a->n_msgs <= 0 || a->n_vars <= 0 || a->P < 0 || a->U < 0 || a->n_ops <= 0 || a->n_sweeps <= 0 || a->n_srcs < 0)
    return fail(MLBP_EINVAL, "bad sizes: B %d, n_msgs %d, n_vars %d, P %d, U %d, n_ops %d, n_sweeps %d, n_srcs %d", a->B, a->n_msgs,
                a->n_vars, a->P, a->U, a->n_ops, a->n_sweeps, a->n_srcs);
  return MLBP_OK;
}

inline int check_states(int32_t X) {
  if (X < 2) return fail(MLBP_EINVAL, "X = %d: a variable needs at least two states", X);
  return MLBP_OK;
}

template <class Args>
int check_args_in_slots(const Args* a) {
  if (!a->in_off || !a->in_slots) return fail(MLBP_EINVAL, "in_off or in_slots is NULL");
  return MLBP_OK;
}

template <class Args>
int check_args_program(const Args* a) {
  if (!a->ops || !a->sweeps || (a->n_srcs > 0 && !a->srcs)) return fail(MLBP_EINVAL, "ops, srcs or sweeps is NULL");
  return check_args_in_slots(a);
}

// The table arrays of the factors there are.  more_pair / more_unary: a per-factor array of the library's own is missing;
// pair_names / unary_names: the arrays the message lists.
template <class Args>
int check_args_tables(const Args* a, bool more_pair, const char* pair_names, bool more_unary, const char* unary_names) {
  if (a->P > 0 && (!a->pair_tables || !a->pair_tab || more_pair || a->n_pair_tables <= 0))
    return fail(MLBP_EINVAL, "P = %d but %s is NULL (or n_pair_tables <= 0)", a->P, pair_names);
  if (a->U > 0 && (!a->unary_tables || !a->unary_tab || more_unary || a->n_unary_tables <= 0))
    return fail(MLBP_EINVAL, "U = %d but %s is NULL (or n_unary_tables <= 0)", a->U, unary_names);
  return MLBP_OK;
}

template <class Args>
int check_args_tables(const Args* a) {
  return check_args_tables(a, false, "pair_tables or pair_tab", false, "unary_tables or unary_tab");
}

template <class Args>
int check_args_extent(const Args* a) {
  if ((int64_t)a->n_msgs * a->X > 0x7fffffff / 2) return fail(MLBP_EUNSUPPORTED, "n_msgs * X = %lld too large", (long long)a->n_msgs * a->X);
  return MLBP_OK;
}

}  // namespace

// ---- what needs the HIP runtime ------------------------------------------------------------------
#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>

namespace {

// `library`: the file name the message gives.
inline int check_device(const char* library) {
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
    (void)hipGetLastError();
    return fail(MLBP_ENODEVICE, "no HIP device visible: %s has no CPU fallback", library);
  }
  return MLBP_OK;
}

// An X = 64 kernel asks for more than the default 64 KiB of dynamic LDS: its limit is raised to `bytes` once per device and
// instance (0 or 1) -- a host-side attribute call, on the first -- eager -- call.
inline int grant_x64_lds(const void* kernel, int instance, int bytes) {
  enum { MAX_DEVICES = 64 };
  static std::atomic<bool> granted[MAX_DEVICES][2];
  static std::mutex mu;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return fail(MLBP_EHIP, "hipGetDevice failed");
  if (dev < 0 || dev >= MAX_DEVICES) return fail(MLBP_EUNSUPPORTED, "device index %d beyond %d", dev, (int)MAX_DEVICES);
  if (granted[dev][instance].load(std::memory_order_acquire)) return MLBP_OK;
  std::lock_guard<std::mutex> lock(mu);
  if (granted[dev][instance].load(std::memory_order_relaxed)) return MLBP_OK;
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e != hipSuccess) return fail(MLBP_EHIP, "raising the X = 64 kernel's LDS limit failed: %s", hipGetErrorString(e));
  granted[dev][instance].store(true, std::memory_order_release);
  return MLBP_OK;
}

}  // namespace
#endif

#endif
