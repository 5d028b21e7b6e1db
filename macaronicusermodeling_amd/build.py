"""Builds libmlbp.so, libmlbp_map.so, libmlbp_logz.so, libmlbp_sample.so, libmlbp_converge.so, libmlbp_cutset.so, libmlbp_exactmap.so, libmlbp_exactgrad.so, libmlbp_exactsample.so, libmlbp_exactmbest.so, libmlbp_cutsetis.so and libmlbp_cutdraw.so (gfx950 only) in-tree with hipcc.  `python -m macaronicusermodeling_amd.build`.

hipcc cross-compiles without a GPU, so this runs in the build container; the resulting .so is
git-ignored but travels to the GPU box with the working-tree snapshot.
"""
import os
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
INCLUDE = os.path.join(PKG, '..', 'include')
CSRC = os.path.join(PKG, 'csrc')
CSRC_MAP = os.path.join(PKG, 'csrc_map')
CSRC_LOGZ = os.path.join(PKG, 'csrc_logz')
CSRC_SAMPLE = os.path.join(PKG, 'csrc_sample')
CSRC_CONVERGE = os.path.join(PKG, 'csrc_converge')
CSRC_CUTSET = os.path.join(PKG, 'csrc_cutset')
CSRC_EXACTMAP = os.path.join(PKG, 'csrc_exactmap')
CSRC_EXACTGRAD = os.path.join(PKG, 'csrc_exactgrad')
CSRC_EXACTSAMPLE = os.path.join(PKG, 'csrc_exactsample')
CSRC_EXACTMBEST = os.path.join(PKG, 'csrc_exactmbest')
CSRC_CUTSETIS = os.path.join(PKG, 'csrc_cutsetis')
CSRC_CUTDRAW = os.path.join(PKG, 'csrc_cutdraw')
LIB = os.path.join(PKG, 'libmlbp.so')
LIB_MAP = os.path.join(PKG, 'libmlbp_map.so')
LIB_LOGZ = os.path.join(PKG, 'libmlbp_logz.so')
LIB_SAMPLE = os.path.join(PKG, 'libmlbp_sample.so')
LIB_CONVERGE = os.path.join(PKG, 'libmlbp_converge.so')
LIB_CUTSET = os.path.join(PKG, 'libmlbp_cutset.so')
LIB_EXACTMAP = os.path.join(PKG, 'libmlbp_exactmap.so')
LIB_EXACTGRAD = os.path.join(PKG, 'libmlbp_exactgrad.so')
LIB_EXACTSAMPLE = os.path.join(PKG, 'libmlbp_exactsample.so')
LIB_EXACTMBEST = os.path.join(PKG, 'libmlbp_exactmbest.so')
LIB_CUTSETIS = os.path.join(PKG, 'libmlbp_cutsetis.so')
LIB_CUTDRAW = os.path.join(PKG, 'libmlbp_cutdraw.so')
SOURCES = ['mlbp_host.cpp', 'mlbp_compile.cpp', 'mlbp_compile_shared.cpp', 'mlbp_program.cpp', 'mlbp_dispatch.cpp', 'mlbp_lean_jit.cpp', 'mlbp_sweep.hip', 'mlbp_lean.hip', 'mlbp_shared.hip', 'mlbp_gemm.hip', 'mlbp_prims.hip', 'mlbp_grad.hip']
SOURCES_MAP = ['mlbp_map.hip']
SOURCES_LOGZ = ['mlbp_logz.hip']
SOURCES_SAMPLE = ['mlbp_sample.hip']
SOURCES_CONVERGE = ['mlbp_converge.hip']
SOURCES_CUTSET = ['mlbp_cutset.hip']
SOURCES_EXACTMAP = ['mlbp_exactmap.hip']
SOURCES_EXACTGRAD = ['mlbp_exactgrad.hip']
SOURCES_EXACTSAMPLE = ['mlbp_exactsample.hip']
SOURCES_EXACTMBEST = ['mlbp_exactmbest.hip']
SOURCES_CUTSETIS = ['mlbp_cutsetis.hip']
SOURCES_CUTDRAW = ['mlbp_cutdraw.hip']
# csrc/ headers: the core library's, and what the side libraries share (mlbp_graph_device.h includes mlbp_device.h)
HEADERS = ['mlbp_internal.h', 'mlbp_device.h', 'mlbp_uop.h', 'mlbp_lean_device.h']
# The lean kernel's device headers, whose TEXT the library carries (mlbp_lean_jit.cpp compiles it at run time with one program's
# micro-ops as constants): written into EMBED, a generated and git-ignored include file, before the core library is compiled
EMBEDDED = ['mlbp_device.h', 'mlbp_uop.h', 'mlbp_lean_device.h']
EMBED = os.path.join(CSRC, 'mlbp_lean_embed.inc')
HEADERS_SIDE = ['mlbp_device.h', 'mlbp_graph_device.h', 'mlbp_graph_host.h', 'mlbp_cutset_plan.h', 'mlbp_cutset_walk.h', 'mlbp_draw_device.h']
# (source dir, sources, csrc/ headers, public header, output): every library has its own sources and its own kernel
# inventory; the flags are the same
LIBRARIES = [
    (CSRC, SOURCES, HEADERS, 'mlbp.h', LIB),
    (CSRC_MAP, SOURCES_MAP, HEADERS_SIDE, 'mlbp_map.h', LIB_MAP),                        # max-product / MAP
    (CSRC_LOGZ, SOURCES_LOGZ, HEADERS_SIDE, 'mlbp_logz.h', LIB_LOGZ),                    # log-partition / joint likelihood
    (CSRC_SAMPLE, SOURCES_SAMPLE, HEADERS_SIDE, 'mlbp_sample.h', LIB_SAMPLE),            # posterior sampling
    (CSRC_CONVERGE, SOURCES_CONVERGE, HEADERS_SIDE, 'mlbp_converge.h', LIB_CONVERGE),    # sweeps to convergence
    (CSRC_CUTSET, SOURCES_CUTSET, HEADERS_SIDE, 'mlbp_cutset.h', LIB_CUTSET),            # exact inference by cutset conditioning
    (CSRC_EXACTMAP, SOURCES_EXACTMAP, HEADERS_SIDE + ['../../include/mlbp_cutset.h'], 'mlbp_exactmap.h', LIB_EXACTMAP),   # exact MAP by cutset conditioning
    (CSRC_EXACTGRAD, SOURCES_EXACTGRAD, HEADERS_SIDE + ['../../include/mlbp_cutset.h'], 'mlbp_exactgrad.h', LIB_EXACTGRAD),   # exact pair marginals and gradient
    (CSRC_EXACTSAMPLE, SOURCES_EXACTSAMPLE, HEADERS_SIDE + ['../../include/mlbp_cutset.h'], 'mlbp_exactsample.h', LIB_EXACTSAMPLE),   # exact posterior sampling
]
# libraries added since: the same tuple shape, built after LIBRARIES
LATER_LIBRARIES = [
    (CSRC_EXACTMBEST, SOURCES_EXACTMBEST, HEADERS_SIDE + ['../../include/mlbp_cutset.h'], 'mlbp_exactmbest.h', LIB_EXACTMBEST),   # exact M-best decoding
    (CSRC_CUTSETIS, SOURCES_CUTSETIS, HEADERS_SIDE + ['../../include/mlbp_cutset.h'], 'mlbp_cutsetis.h', LIB_CUTSETIS),   # cutset importance sampling: log Z and marginals beyond the exact limit
]
# and since those: a third list, because the tests of the earlier libraries pin len(LIBRARIES) == 9 and
# len(LIBRARIES) + len(LATER_LIBRARIES) == 11
MORE_LIBRARIES = [
    (CSRC_CUTDRAW, SOURCES_CUTDRAW, HEADERS_SIDE, 'mlbp_cutdraw.h', LIB_CUTDRAW),   # the cutset proposal drawn from held messages
]
FLAGS = ['-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-fno-fast-math', '-Wall',
         '-Wno-unused-function']


def _stale(obj, deps):
    if not os.path.exists(obj):
        return True
    t = os.path.getmtime(obj)
    return any(os.path.getmtime(d) > t for d in deps)


def _write_embed():
    """EMBED: the EMBEDDED headers as raw string literals (rewritten only when its text would change: it is a dependency)."""
    delim = 'MLBPEMBED'
    out = ['// generated by build.py from %s: do not edit\n' % ', '.join(EMBEDDED), 'enum { MLBP_EMBED_N = %d };\n' % len(EMBEDDED),
           'static const char* const MLBP_EMBED_NAMES[] = {%s};\n' % ', '.join('"%s"' % h for h in EMBEDDED),
           'static const char* const MLBP_EMBED_TEXTS[] = {\n']
    for h in EMBEDDED:
        with open(os.path.join(CSRC, h)) as f:
            text = f.read()
        assert ')' + delim not in text
        # (pieces of at most ~12 KB, concatenated by the compiler: no single literal near a compiler's length limit)
        lines = text.splitlines(True)
        pieces = [''.join(lines[i:i + 100]) for i in range(0, len(lines), 100)]
        out.append(''.join('R"%s(%s)%s"\n' % (delim, p, delim) for p in pieces) + ',\n')
    out.append('};\n')
    new = ''.join(out)
    old = None
    if os.path.exists(EMBED):
        with open(EMBED) as f:
            old = f.read()
    if new != old:
        with open(EMBED, 'w') as f:
            f.write(new)


def _build_one(hipcc, csrc, sources, headers, lib, force, verbose):
    objs = []
    for src in sources:
        path = os.path.join(csrc, src)
        obj = os.path.join(csrc, os.path.splitext(src)[0] + '.o')
        if force or _stale(obj, [path] + headers):
            cmd = [hipcc] + FLAGS + ['-x', 'hip', '-c', path, '-o', obj]
            if verbose:
                cmd.insert(1, '-Rpass-analysis=kernel-resource-usage')
                print(' '.join(cmd))
            subprocess.check_call(cmd)
        objs.append(obj)
    if force or _stale(lib, objs):
        subprocess.check_call([hipcc, '-shared', '-fPIC', '--offload-arch=gfx950', '-o', lib] + objs)
    return lib


def build(force=False, verbose=False):
    """Builds the twelve libraries; returns the path of libmlbp.so (the others lie beside it: LIB_MAP, LIB_LOGZ, LIB_SAMPLE,
    LIB_CONVERGE, LIB_CUTSET, LIB_EXACTMAP, LIB_EXACTGRAD, LIB_EXACTSAMPLE, LIB_EXACTMBEST, LIB_CUTSETIS, LIB_CUTDRAW)."""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    _write_embed()
    for csrc, sources, headers, public, lib in LIBRARIES + LATER_LIBRARIES + MORE_LIBRARIES:
        deps = [os.path.join(CSRC, h) for h in headers] + [os.path.join(INCLUDE, public)]
        _build_one(hipcc, csrc, sources, deps, lib, force, verbose)
    return LIB


if __name__ == '__main__':
    print(build(force='--force' in sys.argv, verbose='-v' in sys.argv))
