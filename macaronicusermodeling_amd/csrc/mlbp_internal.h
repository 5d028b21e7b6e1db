// Internal declarations shared by the host (mlbp_host.cpp, mlbp_compile*.cpp; with HIP runtime calls: mlbp_program.cpp,
// mlbp_dispatch.cpp) and device (mlbp_*.hip) translation units of libmlbp.so.  Not part of the ABI.  Includes no device header itself: the host-only units compile without one.
#ifndef MLBP_INTERNAL_H
#define MLBP_INTERNAL_H

#include <string>
#include <vector>

#include "../../include/mlbp.h"
#include "mlbp_uop.h"

namespace mlbp_dev { struct GradFusedDev; }

struct mlbp_program;

namespace mlbp {
// Device memory owned by a program (or by a cache entry): a pointer and its capacity IN BYTES.  grow() never frees: it allocates
// a new block and retires the old one to `owner`, which keeps it alive until mlbp_program_destroy -- a HIP graph captured
// earlier may still name it (a free on growth was a use-after-free on replay).  The block is freed with its holder.
// device_release / device_grow / device_upload (mlbp_program.cpp) are the only places that allocate or free for it.
void device_release(void* p);
int device_grow(mlbp_program* owner, void** p, size_t* bytes, size_t need, bool zero);
int device_upload(const char* what, void** p, size_t* bytes, const void* src, size_t n_bytes);
template <class T>
struct DeviceArray {
  T* p = nullptr;
  size_t bytes = 0;
  DeviceArray() = default;
  DeviceArray(DeviceArray&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
  DeviceArray(const DeviceArray&) = delete;
  DeviceArray& operator=(const DeviceArray&) = delete;
  ~DeviceArray() { release(); }
  operator T*() const { return p; }
  void release() { device_release(p); p = nullptr; bytes = 0; }
  // at least `need` bytes (zero: a new block is cleared); MLBP_OK or MLBP_EHIP
  int grow(mlbp_program* owner, size_t need, bool zero = false) { return device_grow(owner, reinterpret_cast<void**>(&p), &bytes, need, zero); }
  // replaces the contents by a synchronous copy of n host elements (the old block is freed: nothing enqueued may still read
  // it); `what` names the caller in the error message
  int upload(const char* what, const T* src, size_t n) { return device_upload(what, reinterpret_cast<void**>(&p), &bytes, src, n * sizeof(T)); }
};

// Records a printf-style message for mlbp_last_error() and returns `code`.
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// Returns MLBP_EHIP with the runtime's message when a HIP call fails.
#define HIP_TRY(expr)                                                                      \
  do {                                                                                     \
    hipError_t _e = (expr);                                                                \
    if (_e != hipSuccess) return mlbp::fail(MLBP_EHIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
  } while (0)

// MLBP_ENODEVICE unless a HIP device is visible: in front of every entry that launches or allocates.
int check_device();
// The device status word of the kernels that have no program attached (allocated on first use), and its synchronising
// read-and-reset (mlbp_gradient_status).
int status_word(int32_t** out);
int status_word_read();

// Raises `kernel`'s dynamic-LDS limit to `bytes`.  hipFuncSetAttribute is a slow host call (~0.1 ms): the largest size granted
// per kernel is remembered and the call repeated only when a launch needs more.  *fresh (optional): this call raised it.
int grant_lds(const void* kernel, size_t bytes, bool* fresh = nullptr);
// The verdict on the launches issued since launch_begin(), and only on them: launch_begin() drops what an earlier runtime call
// of this thread -- the caller's, another library's -- may have left in the thread's last-error slot.  `what` names the launch
// in the message, which carries the runtime's own words.
void launch_begin();
int launch_verdict(const char* what);

// Every kernel launch of the library goes through MLBP_LAUNCH: it appends the kernel's handle to the calling thread's launch
// log (mlbp_launch_log) and then launches.  The log is host-side bookkeeping only, like mlbp_last_sweep_kernel().
void launch_log_record(const void* kernel);
#define MLBP_LAUNCH(kernel, ...)                                                           \
  do {                                                                                     \
    mlbp::launch_log_record((const void*)(kernel));                                        \
    hipLaunchKernelGGL(kernel, __VA_ARGS__);                                               \
  } while (0)

// The program compilers (mlbp_compile.cpp, mlbp_compile_shared.cpp): pure host code.  mlbp_program_create runs the chain
// validate_program -> build_fused_program -> build_shared_program / build_lean_program (and drop_unchanged_updates for the
// pruned twin); mlbp_program_plan and mlbp_program_image run the same chain without a device.
int validate_program(const int32_t* ops, int32_t n_ops, const int32_t* srcs, int32_t n_srcs, const int32_t* sweeps,
                     int32_t n_sweeps, int32_t n_msgs, int32_t P, int32_t U, int* max_srcs_out);
int drop_unchanged_updates(const int32_t* ops, const int32_t* srcs, const int32_t* sweeps, int n_sweeps, int n_msgs,
                           std::vector<int32_t>& ops_out, std::vector<int32_t>& sweeps_out);
// Index of the constant product whose hoisted message slots are exactly `consts`, or -1.
int find_cprod(const std::vector<std::vector<int32_t>>& cprods, const std::vector<int32_t>& consts);

// Fused program form of the X = 64 kernels (build_fused_program): 8-word op headers.
enum { FOP_UNARY = 0, FOP_PAIR_TM = 1, FOP_PAIR_MT = 2, FOP_VAR = 3, FOP_VAR_PAIR_TM = 4, FOP_VAR_PAIR_MT = 5,
       FOP_BUNDLED = 0x100 /* flag: the next update touches disjoint slots and may share this one's barrier */ };
struct FusedProgram {
  std::vector<int32_t> fops, psrcs, fsweeps, hoist, cpw, pairseq, written;
  int n_cprod = 0;
  bool has_unary_fops = false;
};
void build_fused_program(const int32_t* ops, const int32_t* srcs, const int32_t* sweeps, int n_sweeps, int n_msgs, FusedProgram& out);

// Micro-op form of the lean X = 64 kernel (mlbp_lean_device.h): operands are LDS byte offsets.  The words and the UOP_* bits
// of word 0: mlbp_uop.h.
struct LeanProgram {
  bool ok = false;
  const char* why = "";
  int n_bundles = 0, HL = 0, n_cprod = 0, WL = 0;
  std::vector<int32_t> image;          // bundles [n_bundles][16] | hoist [4][HL][2] | cprod lists [n_cprod][16] | written [4][WL] | padding
  std::vector<char> hoisted;           // [n_msgs] the slot holds a hoisted (constant) unary message
  std::vector<std::vector<int32_t>> cprods;   // hoisted message slots of constant product k
};
void build_lean_program(const FusedProgram& fp, int n_msgs, LeanProgram& out);
bool build_lean_readout(const LeanProgram& lp, int n_msgs, int n_vars, const int32_t* in_off, const int32_t* in_slots,
                        std::vector<int32_t>& image);
// Enqueues the lean scale-free kernel when it applies (sets *launched); flagged graphs are left in prog->d_bail.
// fuse_gradient: the call's gradient runs as the kernel's epilogue (P <= 3, every unary message hoisted, F = (3, 6): the caller
// has asked exact_kernel_fuses_gradient).
// walk_mode: mlbp_set_lean_walk's, read once per public call; *walk: the direction of the launch (0 forward, 1 backward), written
// when one is enqueued.
int launch_lean_sweep(mlbp_program* prog, const mlbp_sweep_args* a, bool fuse_gradient, int walk_mode, void* stream, bool* launched,
                      int* walk);
// The same for several (program, arguments) groups in one launch.  member: in, the groups offered; out, the groups launched
// (a group that does not qualify is left out, not the call).
int launch_lean_groups(mlbp_program* const* progs, const mlbp_sweep_args* args, int n_groups, int walk_mode, void* stream,
                       std::vector<char>& member, int* walk);

// Run-time specialisation of the lean kernel (mlbp_lean_jit.cpp): the static kernel of ONE program -- its bundle words compiled
// in -- as a loaded module.  state: 0 not tried, 1 in use, -1 tried and fell back (why); there is one attempt per program.
struct LeanJit {
  void* module = nullptr;      // hipModule_t, unloaded with the program
  void* function = nullptr;    // hipFunction_t of sweep_x64_lean_static_kernel
  int state = 0;
  double seconds = 0.0;        // what the attempt that succeeded took: compile and load
  std::string why;
};
// The automatic policy: the first single X = 64 call of a P = 3 program with at least this many graphs, on a stream that is
// not capturing, compiles (synchronously, once).  Below it a launch is under 0.1 ms and the saving a microsecond or two.
constexpr int LEAN_JIT_MIN_BATCH = 4096;
// Dynamic LDS of one lean launch of `prog` (mlbp_lean.hip): messages and ext slots, the reduction buffers, the micro-ops, the
// seventh table of an X = 64 launch, the fused gradient's per-factor words.  The one statement of it: lean_plan asks for it and
// lean_jit_specialize holds it against the 64 KB the static kernel's immediates can address.
size_t lean_lds_bytes(const mlbp_program* prog, bool grad, bool padx);
int lean_jit_specialize(mlbp_program* prog);                    // compiles unless tried before; returns the state
void lean_jit_auto(mlbp_program* prog, int B, void* stream);    // the policy; MLBP_LEAN_SPECIALIZE=0 in the environment disables it
void lean_jit_release(mlbp_program* prog);

// Shared-table (MFMA) form, mlbp_shared.hip: 16 graphs per workgroup, messages kept as [state][graph]
// tiles in LDS, only the "live" slots (read or written inside the sweeps) resident.
struct SharedProgram {
  bool ok = false;
  const char* why = "";               // when !ok: what rules the program out
  int n_ops = 0, n_live = 0, n_cpw = 0, n_back = 0, n_fill = 0, n_init = 0, n_bundles = 0;
  int off_ent = 0, off_back = 0, off_fill = 0, off_init = 0, off_ptile = 0, off_written = 0;
  int max_sources = 1;                 // most tiles any variable update multiplies
  // product-fused form (degree <= 2 variables: K2, K3, chains, rings): the producer of a factor->variable message stores it
  // already multiplied by the destination variable's constant product, so a contraction reads ONE tile and multiplies nothing
  bool pf_ok = false;
  int off_pfb = 0, off_stash = 0, off_pinit = 0, n_stash = 0, n_pinit = 0, off_vftile = 0;
  bool vf_direct = false;             // the gradient epilogue may read the final variable->factor messages from the message tiles
  // ... its three-source variant (K4 cliques: messages stored as sqrt(c) (.) m, constant products in memory; mlbp_compile_shared.cpp)
  bool p3_ok = false;
  int n_lds = 0, sqrt_mask = 0, off_map3 = 0, off_kind3 = 0, off_back3 = 0;
  std::vector<int32_t> sweeps;         // {first op, count} of the transformed op list (one sequence: sweep boundaries mean nothing here)
  // bundles [n_bundles + 1][2][4] | cprod entries [n_cpw] | write-back pairs [n_back][2] | fill slots [n_fill] | uniform tiles [n_init] |
  // product tiles [n_cprod] | written bits | 16 zeros | the sections of the product-fused form in use (mlbp_compile_shared.cpp) | 16 zeros
  std::vector<int32_t> image;
  std::vector<int32_t> live_of_slot;   // [n_msgs + 1 + n_cprod] LDS tile of a slot (ext slots included) or -1
  std::vector<int32_t> hoisted;        // [n_msgs] unary factor whose constant message the slot holds, or -1
  std::vector<char> written;           // [n_msgs] some update of the program writes the slot
  std::vector<std::vector<int32_t>> cprods;   // hoisted message slots of constant product k
};
void build_shared_program(const FusedProgram& fp, int n_msgs, int P, int U, SharedProgram& out);
// Builds the device read-out image of the shared form from the per-variable incoming-slot lists;
// false when some variable's constant part matches no constant product.
bool build_shared_readout(const SharedProgram& sp, int n_msgs, int n_vars, const int32_t* in_off, const int32_t* in_slots,
                          std::vector<int32_t>& image);
// Enqueues the shared-table kernel when it applies (sets *launched); flagged graphs are left in
// prog->d_bail for the exact kernel.
int launch_shared_sweep(mlbp_program* prog, const mlbp_sweep_args* a, void* stream, bool* launched);
// Whether that launch also runs a->gradient (as the sweep kernel's epilogue); and whether the exact X = 64 kernel can (it
// redoes flagged graphs, gradient included).  Both are functions of the arguments alone.
bool shared_gradient_fused(const mlbp_program* prog, const mlbp_sweep_args* a);
bool exact_kernel_fuses_gradient(const mlbp_program* prog, const mlbp_sweep_args* a);
// mlbp_grad.hip: the per-graph gradient kernel on the graphs whose flag byte is set (fix-up behind a fused gradient the exact
// kernel cannot redo: more than three pairwise factors)
int gradient_flagged_only(const mlbp_gradient_args* a, const uint8_t* flags, void* stream);
// The same for n_groups groups in ONE launch (table cached with `owner`'s group tables).
int gradient_flagged_groups(const mlbp_gradient_args* args, const uint8_t* const* flags, int n_groups, mlbp_program* owner, void* stream);
// The same for several (program, arguments) groups in one launch sequence.  member: in, the groups offered; out, the groups
// launched (a group that does not qualify is left out, not the call).
int launch_shared_groups(mlbp_program* const* progs, const mlbp_sweep_args* args, int n_groups, void* stream, std::vector<char>& member);
// Pairwise part of the gradient for shared tables (X = 64, F_ee = 3), ADDED to a->grad_en_en.
int launch_shared_pair_gradient(const mlbp_gradient_args* a, int32_t* status, void* stream);
// Shared tables at X = 128 .. 512: the sweeps update by update over the whole batch, every contraction one launch of the
// hand-written MFMA kernel of mlbp_gemm.hip (float64 tables, or float32 with MLBP_SWEEP_PAIR_TABLES_F32).  Sets *launched;
// a call it does not take (tables not stated shared, no host row, approximate inference, more than 16 pairwise factors, a
// shape the contraction does not support) is left to the per-graph kernels.
int launch_gemm_sweep(mlbp_program* prog, const mlbp_sweep_args* a, void* stream, bool* launched);
bool gemm_path_supports(int X);
// Pairwise part of the gradient for shared tables at X >= 128 (F_ee = 3), ADDED to a->grad_en_en.
int launch_gemm_pair_gradient(const mlbp_gradient_args* a, int32_t* status, void* stream);
// Bytes of mlbp_gradient_args.workspace that call needs (0: none): the weighted table fragments and the per-graph sums.
size_t gemm_gradient_workspace_bytes(const mlbp_gradient_args* a);
size_t shared_gradient_workspace_bytes(const mlbp_gradient_args* a);

// ---- the per-graph kernels of mlbp_sweep.hip --------------------------------------------------------------------------
// The fast pass that has already run over a call's graphs, leaving the flagged ones (prog->d_bail) to the exact kernel.
enum FastPass { FAST_NONE, FAST_LEAN, FAST_SHARED };
// The exact X = 64 kernel applies to (prog, a): X = 64 and the graph's messages and program image fit its LDS.
bool exact_x64_applies(const mlbp_program* prog, const mlbp_sweep_args* a);
// The device form of a fused gradient request (the exact and the lean kernel's epilogue read the same one).
void fill_grad_fused(const mlbp_gradient_args* ga, mlbp_dev::GradFusedDev* gf);
// Enqueues the exact X = 64 kernel (the caller has asked exact_x64_applies): on every graph, or -- flagged_only, the fix-up
// pass behind a fast kernel -- on the graphs flagged in prog->d_bail.  fuse_gradient: a->gradient runs as its epilogue.  The
// marginals are its epilogue when the messages are normalised.  *post_done: the launch took a->posterior (the fix-up pass
// visits every graph's flag anyway; without one the posterior is a launch of its own behind the sweeps).
int launch_exact_x64(mlbp_program* prog, const mlbp_sweep_args* a, bool flagged_only, bool fuse_gradient, void* stream, bool* post_done);
// Behind launch_shared_groups: the fix-up pass of every member in ONE launch (table cached with progs[0]).  *launched false,
// nothing enqueued: some member needs the per-group path (marginals without normalisation, an LDS image too large, a gradient
// the shared-table kernel did not produce, gradients on some members only).
int launch_exact_x64_groups(mlbp_program* const* progs, const mlbp_sweep_args* args, int n_groups, const std::vector<char>& member,
                            void* stream, bool* launched);
// The wide kernel when it applies (sets *launched): X = 128 / 256 / 512 exactly, and (normalised messages, float64 tables) any
// X in (64, 1024] with the last pieces of each row masked.
int launch_wide_sweep(mlbp_program* prog, const mlbp_sweep_args* a, void* stream, bool* launched);
// The generic kernel: any X.  flagged_only: its fix-up mode behind the lean kernel on padded vectors (X < 64).
int launch_generic_sweep(mlbp_program* prog, const mlbp_sweep_args* a, bool flagged_only, void* stream);

// A process-wide arena for the calls that carry no program and were given no workspace (mlbp_gradient_f64 with shared tables):
// one block per (device, purpose), grown the same way and never freed.  Calls that use it on different streams must not overlap.
int fallback_scratch(int purpose, size_t bytes, void** out);
enum { SCRATCH_GEMM_GRADIENT = 0, SCRATCH_SHARED_GRADIENT = 1, SCRATCH_PURPOSES = 2 };
}  // namespace mlbp

namespace mlbp {
// Device copies of the group tables of mlbp_sweep_groups_f64, ONE PER DISTINCT CONTENTS: a call whose table equals an earlier
// one reuses that copy without an upload, a call with other buffers or groups gets its own -- so a HIP graph captured on one
// table keeps replaying against it.  At most MAX tables per program; beyond that the oldest copy is overwritten
// (a graph captured on it must be re-captured: include/mlbp.h says so).
struct GroupTables {
  enum { MAX = 64 };
  struct Entry { std::vector<int32_t> words; DeviceArray<int32_t> dev; };
  std::vector<Entry> entries;
  size_t next_evict = 0;
};
int group_table_device(GroupTables& gt, const std::vector<int32_t>& table, void* stream, int32_t** out);
}  // namespace mlbp

// Device-resident, validated op list (see mlbp_program_create).  Every device block is a DeviceArray: freed with the program.
struct mlbp_program {
  int32_t n_ops = 0, n_srcs = 0, n_sweeps = 0, n_msgs = 0, P = 0, U = 0;
  int32_t n_pairseq = 0;  // pair ops over all sweeps, in execution order
  int32_t max_srcs = 0;   // largest MLBP_OP_VAR fan-in
  int device = 0;
  mlbp::DeviceArray<int32_t> d_ops;      // [n_ops][4]
  mlbp::DeviceArray<int32_t> d_srcs;     // [n_srcs], padded: the fused kernel reads sources 16 at a time
  mlbp::DeviceArray<int32_t> d_sweeps;   // [n_sweeps][2]
  mlbp::DeviceArray<int32_t> d_pairseq;  // [n_pairseq + 1] pair slot of the k-th executed pair op (-1 terminated)
  mlbp::DeviceArray<int32_t> d_status;   // [1] set non-zero by a kernel that met an out-of-range table index
  std::vector<int32_t> h_ops, h_sweeps;  // host copies of the validated op list (the op-by-op GEMM path walks them)
  // fused form used by the X = 64 kernel (build_fused_program)
  int32_t n_fops = 0, n_hoist = 0, n_psrcs = 0, n_cprod = 0, n_cpw = 0, n_written = 0;
  bool sf_ok = false;                    // the scale-free kernel applies (no in-loop unary ops)
  mlbp::DeviceArray<int32_t> d_fops;     // one block: op headers [n_fops][8], source lists [n_psrcs], hoist list
                                         // [n_hoist][2], constant-product lists [n_cpw], written slots [n_written]
  mlbp::DeviceArray<int32_t> d_fsweeps;  // [n_sweeps][2]
  mlbp::DeviceArray<int32_t> d_fpairseq; // pair slot of the k-th executed pairwise update of the fused form (-1 terminated)
  mlbp::FusedProgram fused;              // host copy (the update-by-update contraction path walks it)
  mlbp::DeviceArray<unsigned char> d_bail;   // per-graph "redo with the exact kernel" flags, one byte per graph (mlbp_program_reserve)
  mlbp::DeviceArray<int32_t> d_readout;  // in_off [n_vars+1] then in_slots (mlbp_program_set_readout), or NULL
  int32_t n_vars = 0, n_readout = 0;
  // the pruned twin
  mlbp_program* pruned = nullptr;   // the same program without the updates MLBP_SWEEP_SKIP_UNCHANGED drops, or NULL (none to drop)
  int32_t n_dropped = 0;
  bool is_twin = false;             // this IS some program's pruned twin
  bool last_was_pruned = false;     // the last sweep call ran the twin (mlbp_program_exact_count reads its flags)
  // lean form (mlbp_lean.hip)
  mlbp::LeanProgram lean;
  mlbp::DeviceArray<int32_t> d_limage;   // LeanProgram::image
  mlbp::DeviceArray<int32_t> d_lreadout; // build_lean_readout
  mlbp::LeanJit jit;             // the program's static kernel, when it has one (mlbp_lean_jit.cpp)
  int lean_walk_next = 0;        // the direction of the program's next lean launch under mlbp_set_lean_walk(2): turned by each one
  mlbp::GroupTables gtables;     // group tables of mlbp_sweep_groups_f64 calls that name this program first (launch_lean_groups)
  mlbp::GroupTables stables;     // the same for the shared-table kernels (launch_shared_groups)
  // shared-table form (mlbp_shared.hip); the scratch below is allocated on first use
  mlbp::SharedProgram shared;
  mlbp::DeviceArray<int32_t> d_simage;   // SharedProgram::image
  mlbp::DeviceArray<int32_t> d_sreadout; // per variable: base tile, count, live tiles (4-word aligned lists) or NULL
  int32_t n_sreadout = 0;
  bool sreadout_all_tiled = false;   // ... and at least one message tile
  bool sreadout_all_based = false;   // every variable of the read-out has a constant product (the product-fused read-out needs it)
  mlbp::DeviceArray<double> d_tfrag;     // [32][2][4096] table fragments in MFMA operand order
  mlbp::DeviceArray<double> d_spill;     // message tiles of the shared-table kernel that do not fit LDS
  mlbp::DeviceArray<double> d_wfrag;     // the gradient epilogue's weighted table fragments [n_pair_tables][2][4][4096]
  mlbp::DeviceArray<int32_t> d_header;   // the prepare launch's per-group headers for the sweep kernel [groups][8]
  mlbp::DeviceArray<double> d_ptiles;    // constant-product tiles of the shared-table kernel [groups][n_cprod][1024]
  // grouped launches (mlbp_sweep_groups_f64) with more than one form of the shared-table kernel: the product-fused groups' sweep
  // launch runs on a side stream beside the others' (fork / join by events behind the prepare launch); created on first use
  void* side_stream = nullptr; void* ev_fork = nullptr; void* ev_join = nullptr;
  // large-state shared-table path (mlbp_gemm.hip): fragment-ordered table copies [P][2][XA^2], the formed input messages of
  // the chunked contraction [B][X], and the gradient's workspace when the caller gave none
  mlbp::DeviceArray<char> d_gfrag, d_gxbuf, d_gwork;
  std::vector<mlbp::DeviceArray<char>> retired;   // blocks a DeviceArray outgrew: freed with the program
};

#endif
