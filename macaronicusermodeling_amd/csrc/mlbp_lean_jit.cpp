// Run-time specialisation of the lean X = 64 sweep kernel: the micro-op program of ONE mlbp_program compiled into the kernel.
//
// The lean kernel (mlbp_lean_device.h) interprets the program's bundle words; they are fixed when mlbp_program_create returns
// and the same for every graph of every launch.  Here the library compiles the kernel's own source text -- embedded at build
// time (mlbp_lean_embed.inc, written by build.py from the three device headers) -- once more for one program, with the words
// as compile-time constants (MLBP_LEAN_STATIC), through hiprtc, loads the code object as a module and keeps module and function
// with the program.  Only the single, non-gradient X = 64 launch of a P = 3 program takes it (launch_lean_sweep); every other
// launch, and every failure on the way (no libhiprtc.so, a compile error, a load error), leaves the compiled-in interpreter in
// charge: same results either way, bit for bit.  libhiprtc.so is opened on first use: the library loads without it.
// Host code only: no kernel here.
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "mlbp_internal.h"
#include "mlbp_lean_embed.inc"      // MLBP_EMBED_N, MLBP_EMBED_NAMES[], MLBP_EMBED_TEXTS[]: the device headers' text

using mlbp::fail;

namespace {

// hiprtc by hand (its header is not needed to build the library, nor its presence to load it)
typedef void* rtc_program;
struct Rtc {
  void* lib = nullptr;         // set last: non-NULL means every entry below resolved
  int (*create)(rtc_program*, const char*, const char*, int, const char* const*, const char* const*) = nullptr;
  int (*compile)(rtc_program, int, const char* const*) = nullptr;
  int (*log_size)(rtc_program, size_t*) = nullptr;
  int (*log)(rtc_program, char*) = nullptr;
  int (*code_size)(rtc_program, size_t*) = nullptr;
  int (*code)(rtc_program, char*) = nullptr;
  int (*destroy)(rtc_program*) = nullptr;
};
Rtc g_rtc;
std::once_flag g_rtc_once;
std::atomic<int> g_compiles{0};

// Opens libhiprtc.so once per process, whichever thread comes first; the others wait for it (std::call_once) and read g_rtc
// only afterwards.  The table is filled into a local and published whole, and only when every entry resolved.
bool rtc_open(std::string& why) {
  std::call_once(g_rtc_once, [] {
    Rtc r;
    void* lib = nullptr;
    const char* names[] = {"libhiprtc.so", "libhiprtc.so.7", "libhiprtc.so.6", "/opt/rocm/lib/libhiprtc.so"};
    for (const char* n : names)
      if ((lib = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
    if (!lib) return;
    auto sym = [&](const char* n) { return dlsym(lib, n); };
    r.create = (decltype(r.create))sym("hiprtcCreateProgram");
    r.compile = (decltype(r.compile))sym("hiprtcCompileProgram");
    r.log_size = (decltype(r.log_size))sym("hiprtcGetProgramLogSize");
    r.log = (decltype(r.log))sym("hiprtcGetProgramLog");
    r.code_size = (decltype(r.code_size))sym("hiprtcGetCodeSize");
    r.code = (decltype(r.code))sym("hiprtcGetCode");
    r.destroy = (decltype(r.destroy))sym("hiprtcDestroyProgram");
    if (!r.create || !r.compile || !r.log_size || !r.log || !r.code_size || !r.code || !r.destroy) return;
    r.lib = lib;
    g_rtc = r;
  });
  if (!g_rtc.lib) why = "libhiprtc.so could not be opened, or lacks an entry point";
  return g_rtc.lib != nullptr;
}

// The translation unit handed to hiprtc: what the device headers take from host headers, the program's words, the kernel.
std::string static_source(const int32_t* bundles, int n_bundles) {
  std::string s =
      "typedef __INT32_TYPE__ int32_t;\ntypedef __UINT32_TYPE__ uint32_t;\ntypedef __UINT8_TYPE__ uint8_t;\n"
      "typedef __UINTPTR_TYPE__ uintptr_t;\n#define DBL_MAX __DBL_MAX__\n#define MLBP_LEAN_STATIC 1\n"
      // the kernel's declarator (mlbp_lean_device.h puts the body behind it): three workgroups of 256 threads per CU
      "#define MLBP_LEAN_STATIC_ENTRY extern \"C\" __global__ __launch_bounds__(256, 3) void sweep_x64_lean_static_kernel(SweepDev d, LeanDev f)\n";
  s += "#define MLBP_LEAN_STATIC_BUNDLES " + std::to_string(n_bundles) + "\n#define MLBP_LEAN_STATIC_IMAGE ";
  for (int i = 0; i < 16 * n_bundles; ++i) {
    if (i) s += ',';
    s += std::to_string(bundles[i]);
  }
  s += "\n#include \"mlbp_lean_device.h\"\n";
  return s;
}

// arch NULL: the current device's.  The flags are build.py's.
bool rtc_compile(const std::string& src, const char* arch, std::vector<char>& code, std::string& why) {
  if (!rtc_open(why)) return false;
  const Rtc& r = g_rtc;
  rtc_program p = nullptr;
  if (r.create(&p, src.c_str(), "mlbp_lean_static.hip", MLBP_EMBED_N, MLBP_EMBED_TEXTS, MLBP_EMBED_NAMES) != 0) {
    why = "hiprtcCreateProgram failed";
    return false;
  }
  std::string arch_opt = std::string("--offload-arch=") + (arch ? arch : "");
  std::vector<const char*> opts = {"-O3", "-std=c++17", "-fno-fast-math"};
  if (arch) opts.push_back(arch_opt.c_str());
  ++g_compiles;
  const int rc = r.compile(p, (int)opts.size(), opts.data());
  bool ok = rc == 0;
  if (!ok) {
    size_t n = 0;
    std::string log;
    if (r.log_size(p, &n) == 0 && n > 1) { log.resize(n); r.log(p, &log[0]); }
    why = "hiprtc compilation failed (" + std::to_string(rc) + "): " + log.substr(0, 2000);
  } else {
    size_t n = 0;
    ok = r.code_size(p, &n) == 0 && n > 0;
    if (ok) { code.resize(n); ok = r.code(p, code.data()) == 0; }
    if (!ok) why = "hiprtc returned no code object";
  }
  r.destroy(&p);
  return ok;
}

bool env_disabled() {
  const char* e = getenv("MLBP_LEAN_SPECIALIZE");
  return e && e[0] == '0' && e[1] == 0;
}

}  // namespace

namespace mlbp {

int lean_jit_specialize(mlbp_program* prog) {
  LeanJit& j = prog->jit;
  if (j.state != 0) return j.state;          // in use, or tried once and never again
  j.state = -1;
  const LeanProgram& lp = prog->lean;
  // (every slot offset must fit the 16-bit immediate of an LDS instruction: the workgroup's LDS stays under 64 KB)
  if (!lp.ok || !prog->d_limage || prog->P != 3 || lp.n_bundles < 1 || lean_lds_bytes(prog, false, false) > 64 * 1024) {
    j.why = "only X = 64 programs with three pairwise factors and under 64 KB of LDS are specialised";
    return j.state;
  }
  // (a product of more than four sources is a chain of carry links; a variable of a three-table graph never multiplies that
  // many, the static step has no arm for them, and StaticBundle asserts it)
  for (int k = 0; k < lp.n_bundles; ++k)
    if (lp.image[16 * (size_t)k] & (UOP_CARRY_IN | UOP_CARRY_OUT)) {
      j.why = "the program holds carry links";
      return j.state;
    }
  // (measured, LAB_NOTES R27: the twin's launch runs at the rate the tables arrive, and its static form is 5 % SLOWER)
  if (prog->is_twin) {
    j.why = "the pruned twin of MLBP_SWEEP_SKIP_UNCHANGED keeps the interpreting kernel";
    return j.state;
  }
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<char> code;
  if (!rtc_compile(static_source(lp.image.data(), lp.n_bundles), nullptr, code, j.why)) return j.state;
  hipModule_t mod = nullptr;
  hipFunction_t fn = nullptr;
  if (hipModuleLoadData(&mod, code.data()) != hipSuccess || hipModuleGetFunction(&fn, mod, "sweep_x64_lean_static_kernel") != hipSuccess) {
    (void)hipGetLastError();
    if (mod) (void)hipModuleUnload(mod);
    j.why = "the compiled module could not be loaded";
    return j.state;
  }
  j.module = mod;
  j.function = fn;
  j.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  j.state = 1;
  return j.state;
}

void lean_jit_auto(mlbp_program* prog, int B, void* stream) {
  if (prog->jit.state != 0 || B < LEAN_JIT_MIN_BATCH || prog->P != 3 || prog->is_twin) return;
  if (env_disabled()) return;                          // (read at every call that could compile: an A/B switch of one process too)
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  // (a query that fails -- the legacy stream while another stream captures in global mode -- counts as "capturing": not now.  It
  // is asked again at the next such call on purpose; it costs a host call of well under a microsecond beside a 0.2 ms launch)
  if (hipStreamIsCapturing((hipStream_t)stream, &cs) != hipSuccess) { (void)hipGetLastError(); return; }
  if (cs != hipStreamCaptureStatusNone) return;        // (not now: a later call outside a capture may)
  (void)lean_jit_specialize(prog);
}

void lean_jit_release(mlbp_program* prog) {
  if (prog->jit.module) (void)hipModuleUnload((hipModule_t)prog->jit.module);
  prog->jit = LeanJit();
}

}  // namespace mlbp

extern "C" {

int mlbp_program_specialize(mlbp_program* prog) {
  if (!prog) return fail(MLBP_EINVAL, "mlbp_program_specialize: NULL program");
  if (int e = mlbp::check_device()) return e;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev != prog->device)
    return fail(MLBP_EINVAL, "mlbp_program_specialize: the program was created on device %d, the calling thread's current device is %d",
                prog->device, dev);
  if (mlbp::lean_jit_specialize(prog) != 1) return fail(MLBP_EUNSUPPORTED, "mlbp_program_specialize: %s", prog->jit.why.c_str());
  fail(0, "specialised: compiled and loaded in %.0f ms", prog->jit.seconds * 1e3);
  return MLBP_OK;
}

int mlbp_program_specialized(const mlbp_program* prog) {
  if (!prog) { fail(MLBP_EINVAL, "mlbp_program_specialized: NULL program"); return 0; }      // (the answer is 1, 0 or -1: no program, nothing in use)
  if (prog->jit.state < 0) fail(0, "not specialised: %s", prog->jit.why.c_str());
  else if (prog->jit.state > 0) fail(0, "specialised: compiled and loaded in %.0f ms", prog->jit.seconds * 1e3);
  return prog->jit.state;
}

int mlbp_lean_compile_count(void) { return g_compiles.load(); }

int mlbp_lean_static_code(const int32_t* bundles, int32_t n_bundles, const char* arch, char* out, int32_t cap) {
  if (!bundles || n_bundles < 1 || !arch || cap < 0 || (cap > 0 && !out)) return fail(MLBP_EINVAL, "mlbp_lean_static_code: bad arguments");
  std::vector<char> code;
  std::string why;
  if (!rtc_compile(static_source(bundles, n_bundles), arch, code, why)) return fail(MLBP_EUNSUPPORTED, "mlbp_lean_static_code: %s", why.c_str());
  if (code.size() > (size_t)INT32_MAX) return fail(MLBP_EINVAL, "mlbp_lean_static_code: the code object does not fit the return value");
  if (cap > 0) memcpy(out, code.data(), std::min(code.size(), (size_t)cap));
  return (int)code.size();
}

}  // extern "C"
