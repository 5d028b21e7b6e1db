"""The built library's sweep and contraction kernel instances are all accounted for (no GPU needed): each one is COVERED by a
GPU parity case in tests/test_gpu_instances.py or UNREACHABLE with the dispatch condition that excludes it.  A new instance
without a case, or a case for an instance that is no longer compiled, fails here."""
import ctypes

import pytest

import kernel_inventory as K
import test_gpu_instances as G
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
