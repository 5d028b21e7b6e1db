"""The contract every side library keeps, checked without a GPU for each entry of build.SIDE_LIBRARIES.

A side library <name> is csrc_<name>/mlbp_<name>.hip, include/mlbp_<name>.h, libmlbp_<name>.so and one binding module.  The
binding's SIGNATURES, constants and args struct mirror the header; the library's kernels are its sources' kernels, all named
<name>_*, and every compiled instance has a case in each of the library's GPU modules; no two of the twelve libraries (the
core library, _ffi and csrc/, included) share a function or a kernel.  What only one library promises -- its bad-argument
table, the kernel-choice, chunk and workspace rules of its header, the header's wording -- is in tests/test_<name>_cpu.py.
"""
import ctypes
import functools
import importlib
import itertools
import os
import re

import pytest

import kernel_inventory as K
from conftest import ROOT
from macaronicusermodeling_amd import _ffi, _sidelib
from macaronicusermodeling_amd import build as B

NAMES = ['map', 'logz', 'sample', 'converge', 'cutset', 'exactmap', 'exactgrad', 'exactsample', 'exactmbest', 'cutsetis', 'cutdraw']
# which of them compile against include/mlbp_cutset.h (they take its packed plan)
TAKE_THE_PLAN = {'exactmap', 'exactgrad', 'exactsample', 'exactmbest', 'cutsetis'}
HEADERS_SIDE = ['mlbp_device.h', 'mlbp_graph_device.h', 'mlbp_graph_host.h', 'mlbp_cutset_plan.h', 'mlbp_cutset_walk.h', 'mlbp_draw_device.h']
# name -> (how many functions the header declares, the compute entry among them)
FUNCTIONS = {
    'map': (7, 'mlbp_map_sweep_f64'), 'logz': (6, 'mlbp_logz_f64'), 'sample': (9, 'mlbp_sample_f64'), 'converge': (7, 'mlbp_converge_f64'),
    'cutset': (8, 'mlbp_cutset_f64'), 'exactmap': (8, 'mlbp_exactmap_f64'), 'exactgrad': (8, 'mlbp_exactgrad_f64'),
    'exactsample': (8, 'mlbp_exactsample_f64'), 'exactmbest': (9, 'mlbp_exactmbest_f64'), 'cutsetis': (8, 'mlbp_cutsetis_f64'),
    'cutdraw': (7, 'mlbp_cutdraw_f64'),
}


def _plain(*names):
    return {(name, ()) for name in names}


# name -> every kernel instance its .so holds, as kernel_inventory names them
INSTANCES = {
    'map': {('map_sweep_x64_kernel', (True,)), ('map_sweep_x64_kernel', (False,)), ('map_sweep_generic_kernel', ())},
    'logz': _plain('logz_x64_kernel', 'logz_x64_shared_kernel', 'logz_generic_kernel', 'logz_sum_kernel'),
    'sample': {('sample_x64_kernel', (True,)), ('sample_x64_kernel', (False,)), ('sample_generic_kernel', ())},
    'converge': {('converge_x64_kernel', (True,)), ('converge_x64_kernel', (False,)), ('converge_generic_kernel', ())},
    'cutset': _plain('cutset_x64_kernel', 'cutset_generic_kernel', 'cutset_combine_kernel'),
    'exactmap': {('exactmap_x64_kernel', (False,)), ('exactmap_x64_kernel', (True,)), ('exactmap_generic_kernel', (False,)),
                 ('exactmap_generic_kernel', (True,)), ('exactmap_final_kernel', ())},
    'exactgrad': {('exactgrad_x64_kernel', (1,)), ('exactgrad_x64_kernel', (2,)), ('exactgrad_generic_kernel', ()),
                  ('exactgrad_combine_kernel', ())},
    'exactsample': _plain('exactsample_weights_x64_kernel', 'exactsample_weights_generic_kernel', 'exactsample_scan_kernel',
                          'exactsample_draw_x64_kernel', 'exactsample_draw_generic_kernel'),
    'exactmbest': _plain('exactmbest_values_x64_kernel', 'exactmbest_values_generic_kernel', 'exactmbest_select_kernel',
                         'exactmbest_lists_x64_kernel', 'exactmbest_lists_generic_kernel', 'exactmbest_merge_kernel'),
    'cutsetis': _plain('cutsetis_x64_kernel', 'cutsetis_generic_kernel', 'cutsetis_combine_kernel'),
    'cutdraw': _plain('cutdraw_x64_kernel', 'cutdraw_generic_kernel'),
}
# the GPU modules whose CASES must name every instance, beside test_gpu_<name>
MORE_GPU_MODULES = {'map': ['test_gpu_map_edges'], 'logz': ['test_gpu_logz_edges'], 'sample': ['test_gpu_sample_edges']}
C_TYPES = {'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'double': ctypes.c_double}

RECORDS = pytest.mark.parametrize('name,module,takes_plan', B.SIDE_LIBRARIES, ids=[r[0] for r in B.SIDE_LIBRARIES])


def _binding(module):
    return importlib.import_module('macaronicusermodeling_amd.' + module)


def _header(name):
    """The text of include/mlbp_<name>.h without its comments."""
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mlbp_%s.h' % name)).read(), flags=re.S)


def _csrc(name):
    return os.path.join(ROOT, 'macaronicusermodeling_amd', 'csrc_' + name)


kernels_of = functools.lru_cache(maxsize=None)(K.kernels_of)
kernel_names = functools.lru_cache(maxsize=None)(K.kernel_names)


def _classes(mod, base):
    return [v for v in vars(mod).values() if isinstance(v, type) and issubclass(v, base) and v.__module__ == mod.__name__]


# ------------------------------------------------------------------------------------------------
# per library
# ------------------------------------------------------------------------------------------------
@RECORDS
def test_declared_exported_and_bound_functions_are_equal(name, module, takes_plan):
    M = _binding(module)
    names = sorted(set(re.findall(r'\b(mlbp_%s_[a-z0-9_]+)\s*\(' % name, _header(name))))
    count, entry = FUNCTIONS[name]
    assert len(names) == count and entry in names
    exported = K.exported_functions(M.LIB_PATH)
    assert exported == names, set(exported) ^ set(names)
    assert sorted(M.SIGNATURES) == names, set(M.SIGNATURES) ^ set(names)
    raw = ctypes.CDLL(M.LIB_PATH)
    for n in names:
        assert hasattr(raw, n)


@RECORDS
def test_args_struct_and_error_class_mirror_the_header(name, module, takes_plan):
    M = _binding(module)
    (args,), (error,) = _classes(M, ctypes.Structure), _classes(M, _sidelib.SideError)
    assert error.LIB == 'libmlbp_' + name
    body = re.search(r'typedef struct mlbp_%s_args \{(.*?)\} mlbp_%s_args;' % (name, name), _header(name), flags=re.S).group(1)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            base, rest = re.match(r'(?:const\s+)?(\w+)\b(.*)', decl, flags=re.S).groups()
            fields += [(d.strip().lstrip('* '), ctypes.c_void_p if '*' in d else C_TYPES[base]) for d in rest.split(',')]
    assert fields == list(args._fields_), fields


@RECORDS
def test_integer_constants_mirror_the_defines(name, module, takes_plan):
    M = _binding(module)
    text = _header(name)
    constants = {k: v for k, v in vars(M).items() if re.fullmatch(r'[A-Z][A-Z0-9_]*', k) and type(v) is int}
    assert {'KERNEL_NONE', 'KERNEL_X64', 'KERNEL_GENERIC'} <= set(constants)
    for k, v in constants.items():
        found = re.search(r'#define MLBP_%s_%s (\d+)\s' % (name.upper(), k), text)
        assert found and int(found.group(1)) == v, k


@RECORDS
def test_kernels_are_the_sources_kernels_and_each_instance_has_a_case(name, module, takes_plan):
    M = _binding(module)
    src = kernel_names(_csrc(name))
    compiled = kernels_of(M.LIB_PATH)
    assert compiled == INSTANCES[name], compiled ^ INSTANCES[name]
    assert {kern for kern, _ in compiled} == src
    assert all(kern.startswith(name + '_') for kern in src)
    for gpu in ['test_gpu_' + name] + MORE_GPU_MODULES.get(name, []):
        G = importlib.import_module(gpu)
        assert set(G.CASES) == compiled, (gpu, set(G.CASES) ^ compiled)
        for kern, tests in G.CASES.items():
            assert tests, (gpu, kern)
            for t in tests:
                assert callable(getattr(G, t, None)), (gpu, kern, t)
    for f in os.listdir(_csrc(name)):
        assert f.endswith(('.hip', '.h', '.o')), f


@RECORDS
def test_build_entry_is_the_layout_of_the_name(name, module, takes_plan):
    mine = [e for e in B.LIBRARIES if os.path.basename(e[4]) == 'libmlbp_%s.so' % name]
    assert len(mine) == 1 and len(mine[0]) == 5
    csrc, sources, headers, public, lib = mine[0]
    assert (os.path.basename(csrc), sources, public) == ('csrc_' + name, ['mlbp_%s.hip' % name], 'mlbp_%s.h' % name)
    assert os.path.samefile(csrc, _csrc(name)) and os.path.dirname(lib) == os.path.dirname(B.LIB)
    assert headers == HEADERS_SIDE + (['../../include/mlbp_cutset.h'] if name in TAKE_THE_PLAN else [])
    assert takes_plan == (name in TAKE_THE_PLAN)
    assert all(os.path.exists(os.path.join(csrc, s)) for s in sources) and os.path.exists(os.path.join(B.INCLUDE, public))
    assert all(os.path.exists(os.path.join(B.CSRC, h)) for h in headers)
    assert lib == _binding(module).LIB_PATH


# ------------------------------------------------------------------------------------------------
# across libraries: every pair among the twelve
# ------------------------------------------------------------------------------------------------
def _twelve():
    """[(name, signatures, .so path, source dir, kernel prefix or None)], the core library first."""
    out = [('core', _ffi.SIGNATURES, _ffi.LIB_PATH, K.CSRC, None)]
    for name, module, _ in B.SIDE_LIBRARIES:
        M = _binding(module)
        out.append((name, M.SIGNATURES, M.LIB_PATH, _csrc(name), name + '_'))
    return out


@pytest.mark.parametrize('name', ['core'] + [r[0] for r in B.SIDE_LIBRARIES])
def test_no_other_library_holds_a_function_or_a_kernel_of_this_one(name):
    libs = _twelve()
    (_, signatures, path, csrc, prefix), = [e for e in libs if e[0] == name]
    for other, other_signatures, other_path, other_csrc, other_prefix in libs:
        if other == name:
            continue
        assert not set(signatures) & set(other_signatures), other
        assert not kernel_names(csrc) & kernel_names(other_csrc), other
        assert not {k for k, _ in kernels_of(path)} & {k for k, _ in kernels_of(other_path)}, other
        if prefix:                                              # (the core library's kernels share no prefix)
            assert not [k for k in kernels_of(other_path) if k[0].startswith(prefix)], other
            assert not [k for k in kernel_names(other_csrc) if k.startswith(prefix)], other


# ------------------------------------------------------------------------------------------------
# the build table
# ------------------------------------------------------------------------------------------------
def test_the_table_lists_the_eleven_side_libraries_once_each_after_the_core_library():
    assert [r[0] for r in B.SIDE_LIBRARIES] == NAMES
    assert [r[1] for r in B.SIDE_LIBRARIES] == ['mapdecode'] + NAMES[1:]
    assert B.HEADERS_SIDE == HEADERS_SIDE
    assert B.LIBRARIES[0] == (B.CSRC, B.SOURCES, B.HEADERS, 'mlbp.h', B.LIB) and B.LIB == _ffi.LIB_PATH
    outputs = [e[4] for e in B.LIBRARIES]
    assert [os.path.basename(o) for o in outputs] == ['libmlbp.so'] + ['libmlbp_%s.so' % n for n in NAMES]
    assert len(set(outputs)) == len(outputs) == 12
    assert not hasattr(B, 'LATER_LIBRARIES') and not hasattr(B, 'MORE_LIBRARIES')
    for a, b in itertools.combinations(B.LIBRARIES, 2):
        assert a[0] != b[0] and not set(a[1]) & set(b[1])        # own directory, own sources
