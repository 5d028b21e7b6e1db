"""The sweep-program compilers (csrc/mlbp_compile.cpp) against tests/golden/program_images.npz: every word the X = 64 launchers
and kernels read from them, as the compilers gave it before they were moved and restructured (make_program_images.py).  CPU only."""
import numpy as np
import pytest

from conftest import load_golden
from macaronicusermodeling_amd import _ffi
from macaronicusermodeling_amd.topology import program_images
import make_program_images as M


@pytest.fixture(scope='module')
def shapes():
    return M.shapes()


def test_every_listed_shape_is_in_the_fixture_and_nothing_else(shapes):
    gold = load_golden('program_images')
    assert sorted(gold.files) == sorted('%s/%s' % (n, w) for n in shapes for w in _ffi.IMAGES)
    assert len(shapes) == 55
    M.check_coverage({k: gold[k] for k in gold.files})


def test_images_equal_the_fixture_word_for_word(shapes):
    gold = load_golden('program_images')
    bad = []
    for name, s in shapes.items():
        for which, got in program_images(**s).items():
            want = gold['%s/%s' % (name, which)]
            if want.dtype != np.int32 or got.dtype != np.int32 or got.shape != want.shape or not np.array_equal(got, want):
                bad.append('%s/%s' % (name, which))
    assert not bad, bad


def _call(s, which, buf, cap, readout=True):
    ops, srcs, sweeps = (np.ascontiguousarray(np.asarray(s[k], dtype=np.int32).reshape(-1)) for k in ('ops', 'srcs', 'sweeps'))
    srcs_p = srcs if len(srcs) else np.zeros(1, dtype=np.int32)
    in_off, in_slots = (np.ascontiguousarray(s[k], dtype=np.int32) for k in ('in_off', 'in_slots'))
    return _ffi.lib.mlbp_program_image(_ffi.i32ptr(ops), len(ops) // 4, _ffi.i32ptr(srcs_p), len(srcs), _ffi.i32ptr(sweeps), len(sweeps) // 2,
                                       s['n_msgs'], s['P'], s['U'], s['n_vars'] if readout else 0, _ffi.i32ptr(in_off) if readout else None,
                                       _ffi.i32ptr(in_slots) if readout else None, which, _ffi.i32ptr(buf), cap)


def test_a_short_buffer_gets_the_full_count_and_only_cap_words(shapes):
    s = shapes['plan_k3_roots_1_4_7']
    gold = load_golden('program_images')
    for which, name in enumerate(_ffi.IMAGES):
        want = gold['plan_k3_roots_1_4_7/' + name]
        cap = len(want) // 2
        buf = np.full(len(want) + 4, -77, dtype=np.int32)
        assert _call(s, which, buf, cap) == len(want)
        assert np.array_equal(buf[:cap], want[:cap]) and (buf[cap:] == -77).all()
        assert _call(s, which, buf, len(buf)) == len(want)
        assert np.array_equal(buf[:len(want)], want) and (buf[len(want):] == -77).all()


def test_bad_requests_are_invalid_arguments(shapes):
    s = shapes['plan_k3_roots_1_4_7']
    buf = np.zeros(8, dtype=np.int32)
    for which in (-1, len(_ffi.IMAGES)):
        assert _call(s, which, buf, len(buf)) == _ffi.MLBP_EINVAL and 'unknown image' in _ffi.last_error()
    for name in ('lean_readout', 'shared_readout'):
        assert _call(s, _ffi.IMAGES.index(name), buf, len(buf), readout=False) == _ffi.MLBP_EINVAL and 'read-out' in _ffi.last_error()
    # the other images need no read-out table, and the validation is mlbp_program_plan's
    assert _call(s, _ffi.IMAGES.index('shared'), buf, len(buf), readout=False) > 0
    broken = dict(s, n_msgs=3)
    assert _call(broken, 0, buf, len(buf)) == _ffi.MLBP_EINVAL and 'out of' in _ffi.last_error()
