// Stand-alone driver for the sweep-program compilers (csrc/mlbp_compile.cpp, mlbp_compile_shared.cpp), for runs under a host
// sanitizer -- the library itself is only ever loaded uninstrumented.  Reads the op lists `tests/golden/make_program_images.py
// --dump FILE` writes and calls every builder, both read-outs, mlbp_program_plan and every mlbp_program_image on each shape.
//
//   python tests/golden/make_program_images.py --dump shapes.txt
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o compile_check tools/compile_check.cpp
//       macaronicusermodeling_amd/csrc/mlbp_compile.cpp macaronicusermodeling_amd/csrc/mlbp_compile_shared.cpp
//       macaronicusermodeling_amd/csrc/mlbp_host.cpp                                              (one command line)
//   ./compile_check shapes.txt
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../macaronicusermodeling_amd/csrc/mlbp_internal.h"

static std::vector<int32_t> read_words(std::istream& in, size_t n) {
  std::vector<int32_t> v(n);
  for (auto& w : v) in >> w;
  v.reserve(n + 1);          // (data() of an empty vector may be NULL: the library wants an array)
  return v;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s SHAPES.txt\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  std::string name;
  int n_shapes = 0, n_shared = 0, n_lean = 0;
  long long words = 0;
  int n_ops, n_srcs, n_sweeps, n_msgs, P, U, n_vars, n_in;
  while (in >> name >> n_ops >> n_srcs >> n_sweeps >> n_msgs >> P >> U >> n_vars >> n_in) {
    const std::vector<int32_t> ops = read_words(in, 4 * (size_t)n_ops), srcs = read_words(in, n_srcs), sweeps = read_words(in, 2 * (size_t)n_sweeps),
                               in_off = read_words(in, n_vars + 1), in_slots = read_words(in, n_in);
    if (!in) { fprintf(stderr, "%s: truncated\n", name.c_str()); return 1; }
    if (int e = mlbp::validate_program(ops.data(), n_ops, srcs.data(), n_srcs, sweeps.data(), n_sweeps, n_msgs, P, U, nullptr)) {
      fprintf(stderr, "%s: %d %s\n", name.c_str(), e, mlbp_last_error());
      return 1;
    }
    mlbp::FusedProgram fp;
    mlbp::build_fused_program(ops.data(), srcs.data(), sweeps.data(), n_sweeps, n_msgs, fp);
    mlbp::LeanProgram lp;
    mlbp::build_lean_program(fp, n_msgs, lp);
    std::vector<int32_t> img;
    if (lp.ok) { mlbp::build_lean_readout(lp, n_msgs, n_vars, in_off.data(), in_slots.data(), img); ++n_lean; }
    mlbp::SharedProgram sp;
    mlbp::build_shared_program(fp, n_msgs, P, U, sp);
    if (sp.ok) { mlbp::build_shared_readout(sp, n_msgs, n_vars, in_off.data(), in_slots.data(), img); ++n_shared; }
    std::vector<int32_t> ops2, sweeps2;
    mlbp::drop_unchanged_updates(ops.data(), srcs.data(), sweeps.data(), n_sweeps, n_msgs, ops2, sweeps2);
    int32_t plan[8];
    if (mlbp_program_plan(ops.data(), n_ops, srcs.data(), n_srcs, sweeps.data(), n_sweeps, n_msgs, P, U, plan)) return 1;
    for (int which = MLBP_IMAGE_FUSED; which <= MLBP_IMAGE_PRUNED; ++which) {
      const int n = mlbp_program_image(ops.data(), n_ops, srcs.data(), n_srcs, sweeps.data(), n_sweeps, n_msgs, P, U, n_vars, in_off.data(),
                                       in_slots.data(), which, nullptr, 0);
      if (n < 0) { fprintf(stderr, "%s image %d: %s\n", name.c_str(), which, mlbp_last_error()); return 1; }
      std::vector<int32_t> out(n);
      if (mlbp_program_image(ops.data(), n_ops, srcs.data(), n_srcs, sweeps.data(), n_sweeps, n_msgs, P, U, n_vars, in_off.data(),
                             in_slots.data(), which, out.data(), n) != n) return 1;
      words += n;
    }
    ++n_shapes;
  }
  printf("%d shapes: shared form for %d, lean form for %d, %lld image words\n", n_shapes, n_shared, n_lean, words);
  return n_shapes ? 0 : 1;
}
