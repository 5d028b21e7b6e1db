"""M-best decoding beyond the exact limit without a GPU: the listed mode of libmlbp_exactmbest.so (include/mlbp_exactmbest.h) --
the ranked m best over LISTED cutset states -- stated in NumPy and pinned on enumeration, every input of
tests/test_gpu_searchmbest.py with its gaps, and the C ABI of the mode.

listed_mbest() states the header on the exact statement of tests/test_exactmbest_cpu.py (Statement): an entry's states are its row
of the list where the exact call decodes c, the select runs over the entries by index and passes over an entry whose row equals
the row of an entry of lower index, and the merge breaks ties by entry index.  Everything else -- the max walk, the list form,
the decode -- is that statement's.

The reference is enumeration RESTRICTED to the listed cutset states (restricted_top): for every distinct listed row the
log-potential of every completion of the free variables, the n largest overall by a stable sort.  Nothing of the algorithm under
test is in it.

The gaps.  A ranked list is compared exactly only where ranks 0 .. m of the reference -- the (m + 1)-th included -- are GAP =
1e-6 nats apart.  INPUTS lists every input the GPU module compares and test_every_gpu_input_has_its_gaps asserts the gaps for
every graph of every input by the restricted enumeration, to which the statement is held there too: none is left out; the seeds
were chosen so that it holds."""
import ctypes
import functools
import os

import numpy as np
import pytest

import cases as C
import test_cutset_cpu as R
import test_cutsetis_cpu as IS
import test_exactmbest_cpu as MB
import test_map_cpu as W
import test_searchmap_cpu as SM
from conftest import ROOT
from oracle import lbp_oracle as O

GAP = MB.GAP


# ------------------------------------------------------------------------------------------------
# the statement
# ------------------------------------------------------------------------------------------------
class ListedStatement(MB.Statement):
    """The listed mode on the exact statement: configuration number c reads entry c of `configs` ([N][n_cut] integers;
    column q is the state of cut[q])."""

    def __init__(self, g, inputs, cut, configs, prune=True):
        MB.Statement.__init__(self, g, inputs, cut, prune=prune)
        self.configs = np.asarray(configs).reshape(len(configs), len(self.cut))
        self.n_configs = len(self.configs)

    def states(self, c):
        return {v: int(self.configs[c][q]) for q, v in enumerate(self.cut)}

    def select(self, M):
        """The at most M entries of positive V, by V descending, ties to the lower index; the first occurrence of a row counts."""
        V = self.values()
        first = {}
        mine = [i for i, row in enumerate(self.configs) if first.setdefault(tuple(int(s) for s in row), i) == i]
        with np.errstate(invalid='ignore'):
            return [i for i in sorted(mine, key=lambda i: (-V[i], i))[:M] if V[i] > 0]


def listed_mbest(spec, inputs, cut, configs, M, **kw):
    """include/mlbp_exactmbest.h's listed mode in NumPy (spec: a spec or an oracle Graph): dict(rows [[state] in var_order],
    scores, entries, n_found) of the at most M rows."""
    g = spec if isinstance(spec, O.Graph) else O.Graph(spec)
    configs = np.asarray(configs)
    assert len(configs) >= 1
    if ((configs < 0) | (configs >= g.X)).any():
        return dict(rows=[], scores=[], entries=[], n_found=-1)
    st = ListedStatement(g, inputs, cut, configs, **kw)
    ranked = sorted(st.candidates(M), key=lambda t: (-t[0], t[1], t[2]))[:M]
    return dict(rows=MB.as_rows(g, [t[3] for t in ranked]), scores=[W.score_of(g, inputs, t[3]) for t in ranked],
                entries=[t[1] for t in ranked], n_found=len(ranked))


# ------------------------------------------------------------------------------------------------
# enumeration restricted to the listed cutset states
# ------------------------------------------------------------------------------------------------
def restricted_top(g, inputs, cut, configs, n):
    """[(score, entry, [state] in var_order)] of the at most n assignments of largest finite score among those whose cutset
    state is listed, best first; entry: the lowest index of the row.  Ties by entry, then in row-major order of the free
    variables."""
    order, X = list(g.var_order), g.X
    free = [v for v in order if v not in cut]
    configs = np.asarray(configs).reshape(len(configs), len(cut))
    with np.errstate(divide='ignore'):
        logs = [(vs, np.log(T)) for vs, T in R._factor_arrays(g, inputs)]

    def along(arr, vs):
        """arr over the free variables vs (one or two, in vs order) broadcast into the grid of all free variables."""
        axes = [free.index(v) for v in vs]
        if len(axes) == 2 and axes[0] > axes[1]:
            arr, axes = arr.T, axes[::-1]
        shape = [1] * len(free)
        for a in axes:
            shape[a] = X
        return arr.reshape(shape)
    found, seen = [], set()
    for i, row in enumerate(configs):
        key = tuple(int(s) for s in row)
        if key in seen:
            continue
        seen.add(key)
        s = dict(zip(cut, key))
        grid = np.zeros((X,) * len(free))
        for vs, L in logs:
            if len(vs) == 1:
                grid = grid + (L[s[vs[0]]] if vs[0] in s else along(L, vs))
            elif vs[0] in s and vs[1] in s:
                grid = grid + L[s[vs[0]], s[vs[1]]]
            elif vs[0] in s:
                grid = grid + along(L[s[vs[0]], :], vs[1:])
            elif vs[1] in s:
                grid = grid + along(L[:, s[vs[1]]], vs[:1])
            else:
                grid = grid + along(L, vs)
        flat = np.asarray(grid, dtype=np.float64).reshape(-1)
        k = min(n, flat.size)
        bar = np.partition(flat, flat.size - k)[flat.size - k]
        keep = np.nonzero((flat >= bar) & np.isfinite(flat))[0]
        found += [(float(flat[j]), i, int(j)) for j in keep]
        found = sorted(found, key=lambda t: (-t[0], t[1], t[2]))[:n]
    out = []
    for score, i, j in found:
        x = dict(zip(cut, (int(v) for v in configs[i])))
        x.update(zip(free, (int(v) for v in np.unravel_index(j, (X,) * len(free)))) if free else ())
        out.append((score, i, [x[v] for v in order]))
    return out


SMALL = SM.SMALL                # K3, K4, K5, a ring, a tree, two components


def _lists(X, n_cut, rs):
    """(name, configs) of a sub-list, the shuffled full list and a list with repeats."""
    full = IS.full_list(X, n_cut)
    if not n_cut:
        return [('empty', np.zeros((3, 0), dtype=np.int32))]    # a forest: the one empty configuration, three times
    return [('sub', full[rs.permutation(len(full))[:max(1, len(full) // 2)]]), ('shuffled', full[rs.permutation(len(full))]),
            ('repeats', full[rs.randint(0, len(full), size=len(full) + 3)])]


@pytest.mark.parametrize('X', [2, 3, 4])
@pytest.mark.parametrize('name,make', SMALL, ids=[n for n, _ in SMALL])
def test_statement_equals_restricted_enumeration(name, make, X):
    """Rows, entries and order equal and scores at 1e-12 for m = 1, 3, 16 on sub-lists, shuffled full lists and lists with
    repeats; the list ends at n_found where fewer assignments are admitted."""
    spec = make(X)
    g = O.Graph(spec)
    cut = R.chosen_ids(spec)
    rs = np.random.RandomState(7 * X + len(name))
    compared = 0
    for seed in (1, 2):
        inputs = C.make_inputs(spec, seed, 'lognormal')
        for kind, configs in _lists(X, len(cut), rs):
            want = restricted_top(g, inputs, cut, configs, MB.MAX_M + 1)
            admitted = len({tuple(r) for r in configs.tolist()}) * X ** (len(g.var_order) - len(cut))
            assert len(want) == min(MB.MAX_M + 1, admitted)
            assert len(want) < 2 or min(MB.gaps_of([s for s, _, _ in want])) >= GAP, (name, X, seed, kind)
            for M in (1, 3, 16):
                got = listed_mbest(g, inputs, cut, configs, M)
                assert got['n_found'] == min(M, admitted), (name, X, M, kind)
                assert got['rows'] == [x for _, _, x in want[:M]], (name, X, M, seed, kind)
                assert got['entries'] == [i for _, i, _ in want[:M]], (name, X, M, seed, kind)
                np.testing.assert_allclose(got['scores'], [s for s, _, _ in want[:M]], rtol=1e-12)
                assert listed_mbest(g, inputs, cut, configs, M, prune=False)['rows'] == got['rows']
                compared += 1
    assert compared >= 6


@pytest.mark.parametrize('name,make', MB.SMALL, ids=[n for n, _ in MB.SMALL])
def test_the_full_list_in_index_order_is_the_exact_statement(name, make):
    """Rows and order, and the configuration numbers as entries."""
    for X in (2, 3, 4):
        spec = make(X)
        g = O.Graph(spec)
        cut = R.chosen_ids(spec)
        full = IS.full_list(X, len(cut))
        inputs = C.make_inputs(spec, 4, 'lognormal')
        for M in (1, 3, 16):
            xs, scores = MB.statement(g, inputs, cut, M)
            got = listed_mbest(g, inputs, cut, full, M)
            assert got['rows'] == MB.as_rows(g, xs) and got['scores'] == scores, (name, X, M)
            assert got['entries'] == [sum(x[v] * X ** q for q, v in enumerate(cut)) for x in xs]


def test_the_duplicate_rule():
    """An entry whose row equals the row of an entry of lower index is ignored: the rows stay distinct, entries name the first
    occurrence, and the answer is the one on the list with the later repeats removed."""
    spec = R.kn_spec(4, 3)
    g, cut = O.Graph(spec), R.chosen_ids(spec)
    inputs = C.make_inputs(spec, 6, 'lognormal')
    configs = np.array([[2, 1], [0, 0], [2, 1], [1, 2], [0, 0], [2, 1], [2, 2]], dtype=np.int32)
    kept = [0, 1, 3, 6]
    for M in (1, 5, 16):
        got = listed_mbest(g, inputs, cut, configs, M)
        clean = listed_mbest(g, inputs, cut, configs[kept], M)
        assert len({tuple(r) for r in got['rows']}) == len(got['rows']) == min(M, 4 * 9)
        assert got['rows'] == clean['rows'] and got['scores'] == clean['scores']
        assert got['entries'] == [kept[e] for e in clean['entries']] and set(got['entries']) <= set(kept)
    every = listed_mbest(g, inputs, cut, np.array([[1, 1]] * 5, dtype=np.int32), 16)
    assert every['entries'] == [0] * 9 and every['n_found'] == 9 and len({tuple(r) for r in every['rows']}) == 9


def test_short_lists_end_at_n_found():
    """Zero rows, and a one-entry list at X = 2: fewer than m admitted assignments of positive potential."""
    spec, inputs = MB.zero_inputs()
    g = O.Graph(spec)
    full = IS.full_list(2, 1)
    for i, count in zip(inputs, (8, 4, 2, 0)):
        want = restricted_top(g, i, [0], full, 17)
        assert len(want) == count
        got = listed_mbest(g, i, [0], full, 16)
        assert got['n_found'] == count and got['rows'] == [x for _, _, x in want]
    one = listed_mbest(g, inputs[0], [0], [[1]], 16)
    assert one['n_found'] == 4 and one['entries'] == [0] * 4 and all(r[g.var_order.index(0)] == 1 for r in one['rows'])
    assert one['rows'] == [x for _, _, x in restricted_top(g, inputs[0], [0], [[1]], 17)]
    none = listed_mbest(g, inputs[1], [0], [[1]], 16)             # variable 0 cannot take state 1
    assert none == dict(rows=[], scores=[], entries=[], n_found=0)
    for bad in (2, -1):
        assert listed_mbest(g, inputs[0], [0], [[0], [bad]], 4)['n_found'] == -1


# ------------------------------------------------------------------------------------------------
# every input of the GPU module: name -> (spec, [inputs], cut, [configs [N][n_cut]], m)
# ------------------------------------------------------------------------------------------------
def _family(spec, seeds, lists, m=16, kind='lognormal'):
    cut = R.chosen_ids(spec)
    inputs = [C.make_inputs(spec, s, kind) for s in seeds]
    return spec, inputs, cut, lists(spec['X'], len(cut), len(inputs)), m


def _full(X, q, B):
    return [IS.full_list(X, q)] * B


INPUTS = {
    'k3_x64_full': lambda: _family(R.kn_spec(3, 64), (0, 1, 2), _full),
    'k4_x4_full': lambda: _family(R.kn_spec(4, 4), (0, 1, 2), _full),
    'k3_x64_shuffled': lambda: _family(R.kn_spec(3, 64), (0, 1, 2), lambda X, q, B: SM.shuffled_lists(X, q, B, 11)),
    'k4_x4_shuffled': lambda: _family(R.kn_spec(4, 4), (0, 1, 2), lambda X, q, B: SM.shuffled_lists(X, q, B, 12)),
    'k5_x64_n1': lambda: _family(R.kn_spec(5, 64), (0, 1, 2), lambda X, q, B: SM.random_lists(X, q, 1, B, 21)),
    'k5_x64_n7': lambda: _family(R.kn_spec(5, 64), (0, 1, 2), lambda X, q, B: SM.random_lists(X, q, 7, B, 22)),
    'k5_x64_n64': lambda: _family(R.kn_spec(5, 64), (0, 1, 2), lambda X, q, B: SM.random_lists(X, q, 64, B, 23)),
    'k5_x64_n7_m4': lambda: _family(R.kn_spec(5, 64), (0, 1, 2), lambda X, q, B: SM.random_lists(X, q, 7, B, 22), m=4),
    'k9_x64': lambda: _family(R.kn_spec(9, 64), (0, 1, 2), lambda X, q, B: SM.random_lists(X, q, 6, B, 24)),
    'k10_x64': lambda: _family(R.kn_spec(10, 64), (0, 1, 2), lambda X, q, B: SM.random_lists(X, q, 6, B, 25), m=4),
    'k5_x7': lambda: _family(R.kn_spec(5, 7), (0, 1, 2), lambda X, q, B: SM.random_lists(X, q, 9, B, 26)),
    'k5_x7_m4': lambda: _family(R.kn_spec(5, 7), (0, 1, 2), lambda X, q, B: SM.random_lists(X, q, 9, B, 26), m=4),
    'k3_x257': lambda: _family(R.kn_spec(3, 257), (0, 1, 2), lambda X, q, B: SM.random_lists(X, q, 5, B, 27), m=4),
    'chain3_x64': lambda: _family(C.chain_spec(3, 64), (0, 1, 2), lambda X, q, B: [np.zeros((2, 0), dtype=np.int32)] * B, m=6),
}


@functools.lru_cache(maxsize=None)
def family(name):
    """(spec, [inputs], cut, [configs], m, [listed_mbest(..., m + 1)]) of INPUTS[name]: computed once per process and shared."""
    spec, inputs, cut, lists, m = INPUTS[name]()
    g = O.Graph(spec)
    return spec, inputs, cut, lists, m, [listed_mbest(g, i, cut, c, m + 1) for i, c in zip(inputs, lists)]


@pytest.mark.parametrize('name', sorted(INPUTS))
def test_every_gpu_input_has_its_gaps(name):
    """No graph is left out: in every graph the GPU module ranks, ranks 0 .. m among the admitted assignments are GAP apart by
    the restricted enumeration, and the statement equals it in rows, entries and scores."""
    spec, inputs, cut, lists, m, refs = family(name)
    g = O.Graph(spec)
    smallest = np.inf
    for b, (i, c, r) in enumerate(zip(inputs, lists, refs)):
        want = restricted_top(g, i, cut, c, m + 1)
        assert len(want) == m + 1, (name, b)
        smallest = min([smallest] + MB.gaps_of([s for s, _, _ in want]))
        assert r['rows'] == [x for _, _, x in want] and r['entries'] == [e for _, e, _ in want], (name, b)
        np.testing.assert_allclose(r['scores'], [s for s, _, _ in want], rtol=1e-12)
    print('%s: smallest of the %d gaps over %d graphs %.1e nats' % (name, m, len(refs), smallest))
    assert smallest >= GAP, (name, smallest)


# ------------------------------------------------------------------------------------------------
# C ABI of the listed mode
# ------------------------------------------------------------------------------------------------
HEADER = os.path.join(ROOT, 'include', 'mlbp_exactmbest.h')


def _M():
    from macaronicusermodeling_amd import exactmbest
    return exactmbest


def _ffi():
    from macaronicusermodeling_amd import _ffi
    return _ffi


def _valid_args(M, X=64, n=3, n_cut=None, N=16, m=16):
    """Arguments of K_n with a list of N entries that pass every host-side check (the pointers are never dereferenced on the host)."""
    from macaronicusermodeling_amd import cutset
    words = cutset.plan_words(R._topo(R.kn_spec(n, 4)), list(range(n - 2 if n_cut is None else n_cut)))
    a = M.ExactMbestArgs()
    a.B, a.X, a.n_vars, a.P, a.U, a.N, a.M = 2, X, n, n * (n - 1) // 2, n, N, m
    a.n_cut, a.n_free, a.n_items, a.n_consts, a.n_forest = (int(w) for w in words[3:8])
    a.n_pair_tables, a.n_unary_tables, a.plan_words = 2 * a.P, 2 * a.U, len(words)
    for name, typ in M.ExactMbestArgs._fields_:
        if typ is ctypes.c_void_p:
            setattr(a, name, 4096)
    a.workspace_bytes = 1 << 40
    return a


def test_the_binding_mirrors_the_new_fields_and_constants():
    M = _M()
    names = [n for n, _ in M.ExactMbestArgs._fields_]
    assert names.index('N') == names.index('M') + 1 and names[-2:] == ['configs', 'entries']
    assert (M.MAX_LISTED, M.MAX_CUT) == (65536, 16)
    text = open(HEADER).read()
    for word in ('MLBP_EXACTMBEST_MAX_LISTED', 'MLBP_EXACTMBEST_MAX_CUT', 'the first occurrence counts', 'stays at M rounds',
                 'lower entry index', 'Workspace of a listed call', 'mlbp_cutsetis_check_plan', 'BEFORE it forms an'):
        assert word in text, word


def test_bad_arguments_of_the_listed_mode():
    M, F = _M(), _ffi()
    for field, value, word in (('N', -1, 'list'), ('N', 65537, 'list'), ('configs', None, 'configs')):
        a = _valid_args(M)
        setattr(a, field, value)
        assert M.lib.mlbp_exactmbest_f64(ctypes.byref(a), None) == F.MLBP_EINVAL, field
        assert word in M.last_error(), (field, M.last_error())
        assert M.lib.mlbp_exactmbest_last_kernel() == M.KERNEL_NONE
    a = _valid_args(M, n=19, n_cut=17)
    assert M.lib.mlbp_exactmbest_f64(ctypes.byref(a), None) == F.MLBP_EUNSUPPORTED and 'at most 16' in M.last_error()
    for field, value, word in (('assignments', None, 'assignments'), ('plan', None, 'plan'), ('workspace_bytes', 8, 'workspace'),
                               ('M', 17, 'rows')):
        a = _valid_args(M, n=5)
        setattr(a, field, value)
        assert M.lib.mlbp_exactmbest_f64(ctypes.byref(a), None) == F.MLBP_EINVAL and word in M.last_error(), field


def test_shapes_beyond_the_exact_limit_reach_the_device_check():
    """K5, K8 and K12 at X = 64 and K5 at X = 7 with a list get as far as the device; the same arguments without one are refused
    for their configurations, as before; an exact call with every pointer set and N = 0 is still accepted."""
    import torch
    M, F = _M(), _ffi()
    for X, n in ((64, 5), (64, 8), (64, 12), (7, 5)):
        a = _valid_args(M, X=X, n=n, N=0)
        if X ** (n - 2) > 65536:
            assert M.lib.mlbp_exactmbest_f64(ctypes.byref(a), None) == F.MLBP_EUNSUPPORTED and 'configurations' in M.last_error(), (X, n)
        if torch.cuda.is_available():
            continue                                            # (the GPU module runs the entry for real)
        for N in (1, 7, 65536):
            a = _valid_args(M, X=X, n=n, N=N)
            a.entries = None                                    # optional
            assert M.lib.mlbp_exactmbest_f64(ctypes.byref(a), None) == F.MLBP_ENODEVICE, (X, n, N, M.last_error())
            assert 'no CPU fallback' in M.last_error() and M.lib.mlbp_exactmbest_last_kernel() == M.KERNEL_NONE
    if not torch.cuda.is_available():
        a = _valid_args(M, n=3, n_cut=0)                        # n_cut = 0 needs no configs (a cyclic remainder is the plan check's)
        a.configs = None
        assert M.lib.mlbp_exactmbest_f64(ctypes.byref(a), None) == F.MLBP_ENODEVICE
        a = MB._valid_args(M)                                   # the exact call's arguments, the new integers 0
        assert a.N == 0 and a.configs == 4096 and a.entries == 4096
        assert M.lib.mlbp_exactmbest_f64(ctypes.byref(a), None) == F.MLBP_ENODEVICE


def test_listed_workspace_bytes_is_the_formula_and_what_the_entry_checks():
    import torch
    from macaronicusermodeling_amd import cutset as S
    M, F = _M(), _ffi()

    def want(B, shape, N, m):
        X, n_vars, P, U, n_forest = shape
        words = B * N * 2 + B * (m + 1) + B * m * m * 2 + (B * m * m * n_vars + 1) // 2
        if MB.values_rule(*shape) == M.KERNEL_GENERIC and (5 * n_vars + 2) * ((X + 1) // 2 * 2) * 8 + 64 + MB.ints(P, U) > S.GENERIC_LDS_BYTES:
            words += B * min(N, -(-S.MIN_WORKGROUPS // B)) * (5 * n_vars + 2) * ((X + 1) // 2 * 2)
        if MB.lists_in_workspace(X, n_vars, P, U, m, n_forest):
            words += B * m * MB.lists_bytes(X, n_vars, m) // 8
        return words * 8
    shapes = ((64, 3, 3, 3, 1), (64, 4, 6, 4, 1), (64, 3, 2, 3, 2), (64, 4, 3, 4, 3), (64, 3, 3, 12, 1), (63, 3, 3, 3, 1), (2, 260, 259, 260, 259),
              (257, 3, 3, 3, 1), (301, 3, 3, 3, 1), (1024, 3, 3, 3, 1), (7, 5, 5, 5, 3), (64, 5, 4, 5, 2), (64, 6, 5, 6, 2), (64, 9, 8, 9, 1), (64, 10, 9, 10, 1))
    for shape in shapes:                                        # the shapes of the exact call's workspace test
        X, n_vars, P, U, n_forest = shape
        for B in (1, 3, 8192):
            for N in (1, 7, 64, 65536):
                for m in (1, 3, 16):
                    assert M.listed_workspace_bytes(B, X, n_vars, P, U, n_forest, N, m) == want(B, shape, N, m), (B, shape, N, m)
        for n_cut in (0, 1, 2):                                 # N = X^|C|: the exact call's bytes
            if X ** n_cut <= S.MAX_CONFIGS and n_cut <= n_vars:
                assert M.listed_workspace_bytes(3, X, n_vars, P, U, n_forest, X ** n_cut, 16) == M.workspace_bytes(3, X, n_vars, P, U, n_forest, n_cut, 16)
    for X, n, N, m in ((64, 3, 64, 16), (64, 5, 1, 1), (64, 5, 7, 16), (64, 9, 256, 4), (64, 10, 256, 16), (64, 12, 65536, 16), (7, 5, 9, 16),
                       (257, 3, 5, 4), (1024, 4, 3, 2)):
        a = _valid_args(M, X=X, n=n, N=N, m=m)
        need = M.listed_workspace_bytes(a.B, X, n, a.P, a.U, a.n_forest, N, m)
        a.workspace_bytes = need - 1                            # one byte short
        assert M.lib.mlbp_exactmbest_f64(ctypes.byref(a), None) == F.MLBP_EINVAL and 'workspace' in M.last_error(), (X, n, N)
        a.workspace_bytes = need
        rc = M.lib.mlbp_exactmbest_f64(ctypes.byref(a), None)
        if not torch.cuda.is_available():
            assert rc == F.MLBP_ENODEVICE, (X, n, N, M.last_error())
    # K5 keeps four waves' 4-lists on chip behind its tables and not their 16-lists; K9 neither
    assert M.kernels(M.pick_kernel(64, 5, 10, 5, 1, 4)) == (M.KERNEL_X64, M.KERNEL_X64)
    assert M.kernels(M.pick_kernel(64, 5, 10, 5, 1, 16)) == M.kernels(M.pick_kernel(64, 9, 36, 9, 1, 4)) == (M.KERNEL_X64, M.KERNEL_GENERIC)
    assert M.kernels(M.pick_kernel(64, 10, 45, 10, 1, 4)) == (M.KERNEL_GENERIC, M.KERNEL_GENERIC)
    assert M.kernels(M.pick_kernel(64, 3, 2, 3, 2, 6)) == (M.KERNEL_X64, M.KERNEL_GENERIC)      # the chain of three at m = 6


def test_a_listed_plan_is_validated_by_the_listed_check():
    """mlbp_exactmbest_check_plan keeps the exact call's bound; cutsetis.plan's check admits K5 at X = 64."""
    from macaronicusermodeling_amd import cutsetis
    M = _M()
    topo = R._topo(R.kn_spec(5, 4))
    with pytest.raises(M.ExactMbestError, match='configurations'):
        M.Plan(topo, [0, 1, 2], 64, None)
    assert cutsetis.Plan(topo, [0, 1, 2], 64, None).n_cut == 3


def test_the_python_layers_exist():
    from macaronicusermodeling_amd import batch, train
    for owner, names in ((batch.FactorGraphBatch, ('cutset_mbest', 'search_mbest')), (train.UserGraphTrainer, ('search_nbest',)),
                         (train.TiDirTrainer, ('search_nbest',))):
        for name in names:
            assert callable(getattr(owner, name, None)), name
    assert 'no unbiased log Z' in train.TiDirTrainer.search_nbest.__doc__


def test_the_gpu_module_names_the_six_kernels_of_a_listed_call_and_its_inputs():
    import test_gpu_searchmbest as G
    import test_side_libraries_cpu as L
    assert set(G.CASES) == L.INSTANCES['exactmbest'] and len(G.CASES) == 6
    for kern, tests in G.CASES.items():
        assert tests, kern
        for t in tests:
            assert callable(getattr(G, t, None)), (kern, t)
    assert set(G.INPUTS_USED) == set(INPUTS), set(G.INPUTS_USED) ^ set(INPUTS)
