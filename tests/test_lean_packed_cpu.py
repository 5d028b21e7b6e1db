"""The argument behind the packed wave reductions of the lean X = 64 kernel (csrc/mlbp_lean.hip, PACKED_NORM and PACKED_HOIST;
LAB_NOTES R20), on the CPU: wave_sum (csrc/mlbp_device.h) adds, level by level, lane ^ 1, lane ^ 2, row_half_mirror, row_mirror
and then (S0 + S16) + (S32 + S48) -- with floating-point addition commutative bit for bit, the balanced pairwise tree over the
entries 0 .. 63 in index order.  A layout that holds 2 or 4 CONSECUTIVE entries in a lane forms the tree's lowest levels as
in-lane adds and its next four as the same four DPP steps inside a row of 16 lanes, so one pass of those steps serves two rows
(plus one exchange between rows of 16) or four slots.  Every function below moves values between lanes exactly as the
instructions do; a total's bits must be wave_sum's, and every lane of a group must hold it.  The running maximum of the keys
(the verdict) is pinned the same way.

This pins the argument, not the kernel: tests/test_gpu_lean_packed.py runs the kernel.
"""
import numpy as np
import pytest

LANES = np.arange(64)
XOR1 = LANES ^ 1                                     # quad_perm [1,0,3,2]
XOR2 = LANES ^ 2                                     # quad_perm [2,3,0,1]
HALF_MIRROR = (LANES & ~7) | (7 - (LANES & 7))       # row_half_mirror
MIRROR = (LANES & ~15) | (15 - (LANES & 15))         # row_mirror
STEPS = (XOR1, XOR2, HALF_MIRROR, MIRROR)


def _row16(v, op):
    """The four DPP steps on [N][64] lane values: every lane of a row of 16 ends with the row's total."""
    for perm in STEPS:
        v = op(v, v[:, perm])
    return v


def wave_sum(v):
    """mlbp_device.h wave_sum on [N][64], lane = entry: [N][64], the total in every lane."""
    v = _row16(v, np.add)
    total = (v[:, 0] + v[:, 16]) + (v[:, 32] + v[:, 48])
    return np.repeat(total[:, None], 64, axis=1)


def wave_max_u32(k):
    k = _row16(k, np.maximum)
    total = np.maximum(np.maximum(k[:, 0], k[:, 16]), np.maximum(k[:, 32], k[:, 48]))
    return np.repeat(total[:, None], 64, axis=1)


def tree_sum(rows):
    """The balanced pairwise tree over the last axis (64 entries) in index order."""
    v = np.asarray(rows, dtype=np.float64)
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def keys(v):
    """mag_key: the high word of the double."""
    return (np.ascontiguousarray(v).view(np.uint64) >> np.uint64(32)).astype(np.uint32)


def packed4_sum(slots):
    """PACKED_NORM on [N][4][64]: lane 16 s + c holds entries 4c .. 4c + 3 of slot s -> [N][64] lane values."""
    e = slots.reshape(-1, 4, 16, 4)
    q = (e[..., 0] + e[..., 1]) + (e[..., 2] + e[..., 3])
    return _row16(q.reshape(-1, 64), np.add)


def packed4_max(slots):
    k = keys(slots).reshape(-1, 4, 16, 4)
    q = np.maximum(np.maximum(k[..., 0], k[..., 1]), np.maximum(k[..., 2], k[..., 3]))
    return _row16(q.reshape(-1, 64), np.maximum)


def packed2_sum(rows):
    """PACKED_HOIST on [N][2][64]: lane 32 half + h holds entries 2h and 2h + 1 of row `half`; behind the DPP steps
    swapadd16(v, v) adds the two rows of 16 lanes inside each half -> [N][64] lane values."""
    e = rows.reshape(-1, 2, 32, 2)
    q = _row16((e[..., 0] + e[..., 1]).reshape(-1, 64), np.add)
    return q[:, LANES & ~16] + q[:, LANES | 16]


def packed8_sum(rows):
    """The eight-entries-per-lane layout of the issue's optional variant, on [N][8][64]: lane 8 r + c holds entries 8c .. 8c + 7 of
    row r; three in-lane levels, then lane ^ 1, lane ^ 2 and row_half_mirror inside groups of 8 lanes.  (Not used by the kernel.)"""
    e = rows.reshape(-1, 8, 8, 8)
    q = ((e[..., 0] + e[..., 1]) + (e[..., 2] + e[..., 3])) + ((e[..., 4] + e[..., 5]) + (e[..., 6] + e[..., 7]))
    v = q.reshape(-1, 64)
    for perm in (XOR1, XOR2, HALF_MIRROR):
        v = v + v[:, perm]
    return v


def _inputs():
    rs = np.random.RandomState(2001)
    n = 4000
    out = {
        'uniform': rs.rand(n, 64),
        'wide': rs.rand(n, 64) * np.exp2(rs.randint(-300, 301, size=(n, 64)).astype(np.float64)),
        'zero': np.zeros((8, 64)),
        'overflow': np.full((8, 64), 1e308) * (0.5 + rs.rand(8, 64)),
    }
    neg = rs.rand(n, 64)
    neg[np.arange(n), rs.randint(0, 64, size=n)] *= -1.0
    out['one_negative'] = neg
    nan = rs.rand(64, 64)
    nan[np.arange(64), np.arange(64)] = np.nan          # the NaN in every position once
    out['nan'] = nan
    return out


INPUTS = _inputs()


def _same(got, want, name):
    """got, want: [N][lanes] -- the same bits (NaN rows: NaN in both)."""
    if name == 'nan':
        assert np.isnan(got).all() and np.isnan(want).all()
        return
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(want).view(np.uint64)), name


@pytest.mark.parametrize('name', sorted(INPUTS))
def test_wave_sum_is_the_pairwise_tree(name):
    rows = INPUTS[name]
    with np.errstate(all='ignore'):
        got, want = wave_sum(rows), tree_sum(rows)
    _same(got, np.repeat(want[:, None], 64, axis=1), name)
    if name == 'overflow':
        assert np.isposinf(want).all()
    if name == 'zero':
        assert (want == 0.0).all()


@pytest.mark.parametrize('name', sorted(INPUTS))
def test_four_entries_per_lane_four_slots_per_pass(name):
    rows = INPUTS[name]
    n = len(rows) // 4 * 4
    slots = rows[:n].reshape(-1, 4, 64)
    with np.errstate(all='ignore'):
        got = packed4_sum(slots)                                     # [N][64], lane group s = the s-th slot
        want = np.stack([wave_sum(slots[:, s])[:, :16] for s in range(4)], axis=1).reshape(-1, 64)
    _same(got, want, name)
    if name != 'nan':       # (a NaN's high word is a key >= KEY_BAD either way; its payload is not pinned)
        kgot = packed4_max(slots)
        kwant = np.stack([wave_max_u32(keys(slots[:, s]))[:, :16] for s in range(4)], axis=1).reshape(-1, 64)
        assert np.array_equal(kgot, kwant)


def test_a_padding_slot_of_ones_leaves_the_other_groups_alone():
    """One to three listed slots and the rest padding (1.0 throughout): the real groups' totals are wave_sum's."""
    rows = INPUTS['wide'][:400].reshape(-1, 4, 64).copy()
    for real in (1, 2, 3):
        slots = rows.copy()
        slots[:, real:] = 1.0
        got = packed4_sum(slots)
        for s in range(4):
            _same(got[:, 16 * s:16 * s + 16], wave_sum(slots[:, s])[:, :16], 'wide')
        assert (got[:, 16 * real:] == 64.0).all()


@pytest.mark.parametrize('name', sorted(INPUTS))
def test_two_entries_per_lane_two_rows_per_pass(name):
    rows = INPUTS[name]
    n = len(rows) // 2 * 2
    pairs = rows[:n].reshape(-1, 2, 64)
    with np.errstate(all='ignore'):
        got = packed2_sum(pairs)                                     # [N][64], half-wave h = row h
        want = np.concatenate([wave_sum(pairs[:, 0])[:, :32], wave_sum(pairs[:, 1])[:, :32]], axis=1)
    _same(got, want, name)


def test_an_empty_upper_half_leaves_the_lower_row_alone():
    """An odd number of rows: the upper half-wave reads words nobody uses (here NaN); the lower row's total is wave_sum's."""
    rows = INPUTS['wide'][:500]
    pairs = np.stack([rows, np.full_like(rows, np.nan)], axis=1)
    got = packed2_sum(pairs)
    _same(got[:, :32], wave_sum(rows)[:, :32], 'wide')


@pytest.mark.parametrize('name', sorted(INPUTS))
def test_eight_entries_per_lane_eight_rows_per_pass(name):
    rows = INPUTS[name]
    n = len(rows) // 8 * 8
    octets = rows[:n].reshape(-1, 8, 64)
    with np.errstate(all='ignore'):
        got = packed8_sum(octets)
        want = np.stack([wave_sum(octets[:, r])[:, :8] for r in range(8)], axis=1).reshape(-1, 64)
    _same(got, want, name)


def test_the_quotients_are_per_entry():
    """row / total with the packed total: the same bits as with wave_sum's, entry by entry (the layout does not enter a division)."""
    rows = INPUTS['uniform'][:512]
    pairs = rows.reshape(-1, 2, 64)
    tot = packed2_sum(pairs)
    got = np.stack([pairs[:, 0] / tot[:, :1], pairs[:, 1] / tot[:, 32:33]], axis=1).reshape(-1, 64)
    want = rows / wave_sum(rows)
    _same(got, want, 'uniform')
