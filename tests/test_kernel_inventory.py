"""The built library's kernels are all accounted for (no GPU needed).  Each instance of the sweep and contraction families is
COVERED by a GPU parity case in tests/test_gpu_instances.py or UNREACHABLE with the dispatch condition that excludes it; every
other kernel has a case in tests/test_gpu_kernels.py (CASES), or -- when it runs only inside a sweep or gradient call -- a
workload of tests/test_gpu_instances.py that launches it (COMPOUND).  A new kernel or instance without a case, or a case for one
that is no longer compiled, fails here; so does a __global__ function of the sources the symbol reader does not find."""
import ctypes
import os
import shutil

import pytest

import kernel_inventory as K
import test_gpu_instances as G
import test_gpu_kernels as GK
from macaronicusermodeling_amd import _ffi

# instance -> the dispatch condition that keeps every call off it.  (The instances found unreachable when this list was made --
# padded grouped lean kernels, float32 contractions at X = 128 / 384, one-table shared-table kernels that spill, take wide updates
# or the three-source form -- are no longer compiled: pick_lean, launch_contract_rt and pick_sweep_kernel say why.)
UNREACHABLE = {}


def test_every_compiled_instance_is_covered_or_unreachable():
    compiled = K.compiled()
    covered, unreachable = set(G.COVERED), set(UNREACHABLE)
    assert not covered & unreachable, sorted(covered & unreachable, key=repr)
    assert compiled - covered - unreachable == set(), 'instances without a GPU parity case: %s' % sorted(compiled - covered - unreachable, key=repr)
    assert covered - compiled == set(), 'cases for instances the library no longer holds: %s' % sorted(covered - compiled, key=repr)
    assert unreachable - compiled == set(), 'stale UNREACHABLE entries: %s' % sorted(unreachable - compiled, key=repr)
    for fam in K.FAMILIES:
        assert any(i[0] == fam for i in compiled), 'no instance of %s found: the symbol table reader missed it' % fam


# kernel -> why no call reaches it (none today)
UNREACHABLE_KERNELS = {}


def _kernel_cases():
    """kernel -> [(module, case)] over the two GPU modules."""
    cases = {}
    for inst in G.COVERED:
        cases.setdefault(inst, []).extend(('test_gpu_instances', w) for w in G.COVERED[inst])
    for kern, ws in G.COMPOUND.items():
        cases.setdefault(kern, []).extend(('test_gpu_instances', w) for w in ws)
    for kern, tests in GK.CASES.items():
        cases.setdefault(kern, []).extend(('test_gpu_kernels', t) for t in tests)
    return cases


def test_every_kernel_is_covered_or_unreachable():
    everything = K.all_compiled()
    assert len(everything) > len(K.compiled())
    assert {k for k in everything if k[0] in K.FAMILIES} == K.compiled()
    cases, unreachable = set(_kernel_cases()), set(UNREACHABLE) | set(UNREACHABLE_KERNELS)
    assert not cases & unreachable, sorted(cases & unreachable, key=repr)
    missing = sorted(everything - cases - unreachable, key=repr)
    assert not missing, 'kernels without a GPU parity case: %s' % missing
    assert cases - everything == set(), 'cases for kernels the library no longer holds: %s' % sorted(cases - everything, key=repr)
    assert unreachable - everything == set(), 'stale unreachable entries: %s' % sorted(unreachable - everything, key=repr)
    assert not set(G.COMPOUND) & set(GK.CASES) and not set(G.COMPOUND) & set(G.COVERED)


def test_every_kernel_case_exists():
    for kern, cases in _kernel_cases().items():
        assert cases, kern
        for module, name in cases:
            if module == 'test_gpu_kernels':
                assert callable(getattr(GK, name, None)), (kern, name)
            else:
                assert name in G.WORKLOADS, (kern, name)
    for kern, why in UNREACHABLE_KERNELS.items():
        assert why.strip(), kern


def test_symbol_reader_finds_every_kernel_of_the_sources():
    """The __global__ functions of csrc/ are exactly the kernels the symbol table holds: a kernel the reader cannot decode (or
    a new one) is named here, and then needs a case above."""
    src = K.kernel_names()
    assert len(src) >= 45
    lib = {name for name, _ in K.all_compiled()}
    assert src - lib == set(), 'kernels in the sources the symbol reader does not find: %s' % sorted(src - lib)
    assert lib - src == set(), 'kernels in the library not defined in the sources: %s' % sorted(lib - src)


def test_a_new_kernel_in_the_sources_is_named(tmp_path):
    """kernel_names() on a copy of the sources with one more (templated, launch-bounded) kernel finds it."""
    for f in os.listdir(K.CSRC):
        if f.endswith(('.hip', '.h')):
            shutil.copy(os.path.join(K.CSRC, f), str(tmp_path))
    with open(str(tmp_path / 'mlbp_prims.hip'), 'a') as f:
        f.write('\ntemplate <int N>\n__global__ __launch_bounds__(256, (N > 2 ? 1 : 2))\nvoid extra_probe_kernel(double* p) { p[0] = N; }\n'
                '// __global__ void commented_out_kernel(double* p);\n')
    assert K.kernel_names(str(tmp_path)) - K.kernel_names() == {'extra_probe_kernel'}


@pytest.mark.parametrize('mangled,want', [
    ('_ZN12_GLOBAL__N_122step_statistics_kernelILi3ELi6EEEvNS_6SumCatElPd', ('step_statistics_kernel', (3, 6))),
    ('_ZN12_GLOBAL__N_111zero_kernelEPdl', ('zero_kernel', ())),
    ('_ZN4mlbp12_GLOBAL__N_119fill_uniform_kernelEPdmd', ('fill_uniform_kernel', ())),
    ('_ZN12_GLOBAL__N_121sweep_x64_lean_kernelILi3ELb0ELb0ELi0ELb1EEEvN8mlbp_dev8SweepDevENS_7LeanDevEPKiiNS1_12GradFusedDevE',
     ('sweep_x64_lean_kernel', (3, False, False, 0, True))),
    ('_Z18extra_probe_kernelPd', ('extra_probe_kernel', ())),                  # at namespace scope
    ('_Z18extra_probe_kernelILi4EEvPd', ('extra_probe_kernel', (4,))),
    ('_ZN12_GLOBAL__N_114g_sum_partialsE', None),             # a device variable's shadow, not a kernel
    ('_Z14g_probe_kernel', None),
    ('_ZN12_GLOBAL__N_18g_statusE', None),
    ('mlbp_sweep_f64', None),
])
def test_any_kernel_symbol_decodes(mangled, want):
    assert K.decode_kernel(mangled) == want


def test_every_case_names_existing_workloads():
    for inst, names in G.COVERED.items():
        assert names, inst
        for n in names:
            assert n in G.WORKLOADS, (inst, n)
    for inst, why in UNREACHABLE.items():
        assert why.strip(), inst
    for name, w in G.WORKLOADS.items():          # every workload builds its graphs, and its roots name their variables
        for g in (w['groups'] if w['kind'] == 'groups' else [w]):
            spec, roots = G.SPECS[g['spec']](g['X']), G.ROOTS[g['spec']]
            assert set(roots) <= set(spec['var_ids']), name
            assert len(roots) >= 3 and len(set(roots)) < len(roots), name    # three sweeps or more, a root repeated


def test_every_wide_instance_that_can_select_has_an_approximate_case():
    """The top-100 selection is fused into sweep_wide_kernel and approximate calls are normalised float64 ones: every
    compiled sweep_wide_kernel<true, Q, double, 2, PAD> has a case of tests/test_gpu_approx.py that runs it with approx_k > 0.
    A new padded instance without one fails here, without a GPU."""
    import test_gpu_approx as GA
    selecting = {i for i in K.compiled() if i[0] == 'sweep_wide_kernel' and i[1][0] is True and i[1][2:4] == ('double', 2)}
    assert len(selecting) >= 15
    assert selecting - set(GA.APPROX_CASES) == set(), 'wide instances without an approximate case: %s' % sorted(selecting - set(GA.APPROX_CASES), key=repr)
    assert set(GA.APPROX_CASES) - selecting == set(), 'approximate cases for instances the library does not hold: %s' % sorted(set(GA.APPROX_CASES) - selecting, key=repr)
    for inst, names in GA.APPROX_CASES.items():
        assert names, inst
        for n in names:
            assert n in GA.CASES and GA.wide_instance(GA.CASES[n]['X']) == inst, (inst, n)


@pytest.mark.parametrize('mangled,want', [
    ('_ZN12_GLOBAL__N_121sweep_x64_lean_kernelILi3ELb0ELb0ELi0ELb1EEEvN8mlbp_dev8SweepDevENS_7LeanDevEPKiiNS1_12GradFusedDevE',
     ('sweep_x64_lean_kernel', (3, False, False, 0, True))),
    ('_ZN4mlbp12_GLOBAL__N_115contract_kernelIdLi2ELi2ELi4ELi4ELb0EEEvNS0_11ContractDevE',
     ('contract_kernel', ('double', 2, 2, 4, 4, False))),
    ('_ZN4mlbp12_GLOBAL__N_117table_frag_kernelIfLi4EEEvPKT_PKdiiiiPS2_', ('table_frag_kernel', ('float', 4))),
    ('_ZN12_GLOBAL__N_117sweep_wide_kernelILb1ELi6EdLi2ELi2EEEvN8mlbp_dev8SweepDevE', ('sweep_wide_kernel', (True, 6, 'double', 2, 2))),
    ('_ZN12_GLOBAL__N_115gradient_kernelILin1ELi6EEEvNS_7GradDevE', ('gradient_kernel', (-1, 6))),
    ('_ZN12_GLOBAL__N_111zero_kernelEPdl', None),
])
def test_template_arguments_decode(mangled, want):
    assert K.decode(mangled) == want


def test_launch_log_is_host_side_and_resets():
    K.reset()
    assert _ffi.lib.mlbp_launch_log(None, 0) == 0 and K.launched() == []
    buf = (ctypes.c_void_p * 4)()
    assert _ffi.lib.mlbp_launch_log(buf, 4) == 0
    # a call refused before it enqueues anything (bad arguments, or no device) logs nothing
    assert _ffi.lib.mlbp_init_messages_f64(None, 1, 4, None) != _ffi.MLBP_OK
    assert _ffi.lib.mlbp_launch_log(None, 0) == 0
