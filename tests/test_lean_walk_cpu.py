"""mlbp_set_lean_walk / mlbp_lean_walk (include/mlbp.h): the process-wide order in which a launch of the default X <= 64
kernel takes its graphs.  The default is forward: the alternating walk measured no gain on the MI355X (LAB_NOTES R32) and is
shipped switched off.  Host-side state only: no device needed.  (What the order does on the device: tests/test_gpu_lean_walk.py.)"""
from macaronicusermodeling_amd import _ffi


DEFAULT = 0


def test_the_default_is_forward():
    assert _ffi.lib.mlbp_lean_walk() == DEFAULT


def test_set_and_get_round_trip():
    try:
        for mode in (0, 1, 2, 1, 0):
            assert _ffi.lib.mlbp_set_lean_walk(mode) == _ffi.MLBP_OK
            assert _ffi.lib.mlbp_lean_walk() == mode
    finally:
        assert _ffi.lib.mlbp_set_lean_walk(DEFAULT) == _ffi.MLBP_OK


def test_an_unknown_mode_is_refused_with_a_message_and_changes_nothing():
    for mode in (3, -1):
        assert _ffi.lib.mlbp_set_lean_walk(mode) == _ffi.MLBP_EINVAL
        assert ('%d' % mode) in _ffi.last_error() and 'walk' in _ffi.last_error()
        assert _ffi.lib.mlbp_lean_walk() == DEFAULT
