"""Builds libmlbp.so, libmlbp_map.so, libmlbp_logz.so, libmlbp_sample.so and libmlbp_converge.so (gfx950 only) in-tree with hipcc.  `python -m macaronicusermodeling_amd.build`.

hipcc cross-compiles without a GPU, so this runs in the build container; the resulting .so is
git-ignored but travels to the GPU box with the working-tree snapshot.
"""
import os
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, 'csrc')
LIB = os.path.join(PKG, 'libmlbp.so')
SOURCES = ['mlbp_host.cpp', 'mlbp_compile.cpp', 'mlbp_compile_shared.cpp', 'mlbp_program.cpp', 'mlbp_dispatch.cpp', 'mlbp_sweep.hip', 'mlbp_lean.hip', 'mlbp_shared.hip', 'mlbp_gemm.hip', 'mlbp_prims.hip', 'mlbp_grad.hip']
# the max-product / MAP library (include/mlbp_map.h): its own sources, its own kernel inventory, the same flags
CSRC_MAP = os.path.join(PKG, 'csrc_map')
LIB_MAP = os.path.join(PKG, 'libmlbp_map.so')
SOURCES_MAP = ['mlbp_map.hip']
# the log-partition / joint-likelihood library (include/mlbp_logz.h): again its own sources and inventory, the same flags
CSRC_LOGZ = os.path.join(PKG, 'csrc_logz')
LIB_LOGZ = os.path.join(PKG, 'libmlbp_logz.so')
SOURCES_LOGZ = ['mlbp_logz.hip']
# the posterior-sampling library (include/mlbp_sample.h): its own sources and inventory, the same flags
CSRC_SAMPLE = os.path.join(PKG, 'csrc_sample')
LIB_SAMPLE = os.path.join(PKG, 'libmlbp_sample.so')
SOURCES_SAMPLE = ['mlbp_sample.hip']
# the sweeps-to-convergence library (include/mlbp_converge.h): its own sources and inventory, the same flags
CSRC_CONVERGE = os.path.join(PKG, 'csrc_converge')
LIB_CONVERGE = os.path.join(PKG, 'libmlbp_converge.so')
SOURCES_CONVERGE = ['mlbp_converge.hip']
FLAGS = ['-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-fno-fast-math', '-Wall',
         '-Wno-unused-function']


def _stale(obj, deps):
    if not os.path.exists(obj):
        return True
    t = os.path.getmtime(obj)
    return any(os.path.getmtime(d) > t for d in deps)


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
    """Builds the five libraries; returns the path of libmlbp.so (the others lie beside it: LIB_MAP, LIB_LOGZ, LIB_SAMPLE,
    LIB_CONVERGE)."""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    headers = [os.path.join(CSRC, 'mlbp_internal.h'), os.path.join(CSRC, 'mlbp_device.h'), os.path.join(PKG, '..', 'include', 'mlbp.h')]
    lib = _build_one(hipcc, CSRC, SOURCES, headers, LIB, force, verbose)
    headers_map = [os.path.join(CSRC, 'mlbp_device.h'), os.path.join(PKG, '..', 'include', 'mlbp_map.h')]
    _build_one(hipcc, CSRC_MAP, SOURCES_MAP, headers_map, LIB_MAP, force, verbose)
    headers_logz = [os.path.join(CSRC, 'mlbp_device.h'), os.path.join(PKG, '..', 'include', 'mlbp_logz.h')]
    _build_one(hipcc, CSRC_LOGZ, SOURCES_LOGZ, headers_logz, LIB_LOGZ, force, verbose)
    headers_sample = [os.path.join(CSRC, 'mlbp_device.h'), os.path.join(PKG, '..', 'include', 'mlbp_sample.h')]
    _build_one(hipcc, CSRC_SAMPLE, SOURCES_SAMPLE, headers_sample, LIB_SAMPLE, force, verbose)
    headers_converge = [os.path.join(CSRC, 'mlbp_device.h'), os.path.join(PKG, '..', 'include', 'mlbp_converge.h')]
    _build_one(hipcc, CSRC_CONVERGE, SOURCES_CONVERGE, headers_converge, LIB_CONVERGE, force, verbose)
    return lib


if __name__ == '__main__':
    print(build(force='--force' in sys.argv, verbose='-v' in sys.argv))
