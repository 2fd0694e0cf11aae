"""Post-filtration of the approximate inverse by value (rlh_fsfilter_create*, rlh_fsfilter_info,
ApproximateInverse(drop=...)): cases shared by the CPU tier (tests/fake_fsai.py) and the GPU tier.  Matrices,
helpers and the bound of the defining property (`check_row`, `beta`) come from tests/_fsai_cases.py (`base`), the level
and adaptive patterns of the unfiltered build from the oracles of tests/_fsai_levels_cases.py (`lv`) and
tests/_fsai_adaptive_cases.py (`ad`).

THE ORACLE (`Oracle`) is written from the rule in include/rlhip.h and shares nothing with the library or the stand-in.
The unfiltered pattern of row i is that of `lv.oracle` (steps = 0) or `ad.oracle`; on it S y = e_last is solved densely
in float64 / complex128, g = conj(y) / sqrt(y_last), and for every column j < i of the row
    r_ij = |g_ij| sqrt(a_jj) / (g_ii sqrt(a_ii)),
formed with the division and the square roots (the library forms |g_ij|^2 a_jj >= drop^2 g_ii^2 a_ii).  The row keeps the
columns with r_ij >= drop and its diagonal.  Per row the oracle also returns the smallest |r_ij / drop - 1|.

WHAT IS COMPARED EXACTLY.  The library decides on the G it stored: float32 storage moves r by about 4e-7 (relative; two
roundings of 2^-24 in g_ij and g_ii), the double solves by far less.  A row whose smallest |r_ij / drop - 1| is below
GAP = 1e-5 is left out of the exact pattern comparison (its own pattern must still pass `check_row`); at most 1 % of a
case's rows may be left out, which every case asserts.  A row the adaptive oracle leaves out (nearly equal scores, its
own GAP of 1e-9) is left out here too and counts towards the same 1 %.

LAUNCH GEOMETRY the loop case relies on: fsai_filter takes 8 lanes per row, 256 threads per workgroup -- 32 rows per
workgroup -- on at most 8 workgroups per CU, in a grid-stride loop: one pass covers CU * 8 * 32 rows.  The 8-lane set-up
that follows takes the same 32 rows per workgroup on the same grid (tests/_fsai_cases.py).
"""

import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import _fsai_cases as base
import _fsai_levels_cases as lv
import _fsai_adaptive_cases as ad
import _fsai_work_cases as wk
from _fsai_cases import TYPES, _L, _check, check_row, csr_tensor, destroy, get, hermitian_from_upper, info, kaporin, last_error, same_bits

GAP = 1e-5
BLOCKS_PER_CU = 8
FILTER_ROWS_PER_BLOCK = 32
DROPS = (0.03, 0.1, 0.3)
LEVEL_1, LEVEL_2, ADAPTIVE, SHORT_ROWS = (1, 0, 1, 64), (2, 0, 1, 64), (1, 4, 2, 64), (1, 0, 1, 12)    # levels, steps, step_size, max_row
PATTERN_CASES = ([(which, config) for which in ('profile-d', 'banded-d') for config in (LEVEL_1, LEVEL_2, ADAPTIVE, SHORT_ROWS)]
                 + [(which, LEVEL_1) for which in ('profile-s', 'profile-c', 'profile-z', 'cut-d', 'lap')]
                 + [('profile-z', LEVEL_2), ('cut-d', SHORT_ROWS)])


def matrix(which):
    if which.startswith('profile-'):
        return base.matrix(which[-1])
    return ad.matrix(which)


@functools.lru_cache(maxsize=None)
def _wide_dense(A_id):
    A = _KEPT[A_id]
    d = hermitian_from_upper(A).toarray().astype(np.clongdouble if A.dtype.kind == 'c' else np.longdouble)
    d.setflags(write=False)
    return d


_KEPT = {}


def wide_dense(A):
    """The operator the upper triangle defines, dense, in longdouble / clongdouble (once per matrix object, never written)."""
    _KEPT[id(A)] = A
    return _wide_dense(id(A))


# ---------------------------------------------------------------- the raw entry points
def create_filtered(A, levels=1, steps=0, step_size=1, drop=0.03, host=False, bits=64, max_row=64):
    """(rc, handle) of rlh_fsfilter_create on A's arrays (host=True) or rlh_fsfilter_create_device on device
    copies of them."""
    from raleigh_amd import _lib
    it = {32: np.int32, 64: np.int64}.get(bits, np.int64)
    arrays = (A.indptr.astype(np.int64 if host else it), A.indices.astype(np.int32 if host else it), np.ascontiguousarray(A.data))
    h = ctypes.c_void_p(12345)
    head = (ctypes.byref(h), _lib.DTYPE_CODE[A.dtype.type], A.shape[0])
    tail = (max_row, levels, steps, step_size, drop)
    if host:
        return _L().rlh_fsfilter_create(*head, *[_lib.host_ptr(a) for a in arrays], *tail), h
    bufs = [base.dev(a) for a in arrays]
    return _L().rlh_fsfilter_create_device(*head, bits, *[b.ptr for b in bufs], *tail), h


def filtered_of(h):
    drop, removed = ctypes.c_double(-1.0), ctypes.c_int64(-1)
    _check(_L().rlh_fsfilter_info(h, ctypes.byref(drop), ctypes.byref(removed)))
    return drop.value, removed.value


def built_filtered(A, levels=1, steps=0, step_size=1, drop=0.03, **kw):
    """G (SciPy) and the info record, with the removed entries under 'removed', of a filtered build that must succeed."""
    rc, h = create_filtered(A, levels, steps, step_size, drop, **kw)
    _check(rc)
    try:
        assert base.levels_of(h) == levels and base.adaptive_of(h) == ((steps, step_size) if steps else (0, 0))
        f = info(h)
        got, f['removed'] = filtered_of(h)
        assert got == drop
        return get(h, A.dtype.type), f
    finally:
        destroy(h)


def built_plain(A, levels=1, steps=0, step_size=1, **kw):
    """The unfiltered build of the same pattern arguments, through the entry point it always had."""
    if steps:
        return base.built(A, '_adaptive', levels, steps, step_size, **kw)
    return base.built(A, '_levels', levels, **kw) if levels > 1 else base.built(A, **kw)


def row_of(G, i):
    return G.indices[G.indptr[i]:G.indptr[i + 1]]


# ---------------------------------------------------------------- the oracle
def oracle_row(M, P, drop):
    """Row i = P[-1] on its unfiltered pattern P: the kept columns and the smallest |r / drop - 1|."""
    P = np.asarray(P, dtype=np.int64)
    if P.size == 1:
        return P, np.inf
    S = M.block(P, P)
    e = np.zeros(P.size, dtype=S.dtype)
    e[-1] = 1.0
    y = np.linalg.solve(S, e)
    g = np.conj(y) / np.sqrt(y[-1].real)
    r = np.abs(g[:-1]) * np.sqrt(M.diag[P[:-1]]) / (g[-1].real * np.sqrt(M.diag[P[-1]]))
    return np.concatenate([P[:-1][r >= drop], P[-1:]]), float(np.min(np.abs(r / drop - 1.0)))


class Oracle:
    def __init__(self, A, levels, steps, step_size, max_row, drop):
        n = A.shape[0]
        M = ad.Dense(A)
        if steps:
            o = ad.oracle(A, levels, steps, step_size, max_row)
            ip0, ix0, sure, self.truncated = o.indptr, o.indices, o.compared, o.truncated
        else:
            ip0, ix0, self.truncated, _ = lv.oracle(A, levels, max_row)
            sure = np.ones(n, dtype=bool)
        rows, gaps = [], []
        for i in range(n):
            p, gap = oracle_row(M, ix0[ip0[i]:ip0[i + 1]], drop)
            rows.append(p)
            gaps.append(gap)
        self.rows, self.gaps = rows, np.array(gaps)
        self.compared = sure & (self.gaps >= GAP)
        lens = np.array([len(p) for p in rows])
        self.before = int(ip0[-1])
        self.nnz, self.longest, self.removed = int(lens.sum()), int(lens.max()), int(ip0[-1] - lens.sum())
        self.lens0, self.lens = np.diff(ip0), lens


@functools.lru_cache(maxsize=None)
def _oracle(A_id, levels, steps, step_size, max_row, drop):
    return Oracle(_KEPT[A_id], levels, steps, step_size, max_row, drop)


def oracle(A, levels, steps, step_size, max_row, drop):
    """Computed once per matrix object and configuration, never written."""
    _KEPT[id(A)] = A
    return _oracle(id(A), levels, steps, step_size, max_row, drop)


# ---------------------------------------------------------------- 1. pattern and values
def pattern(which, config, drop):
    levels, steps, step_size, max_row = config
    A = matrix(which)
    n = A.shape[0]
    o = oracle(A, levels, steps, step_size, max_row, drop)
    left_out = int(np.sum(~o.compared))
    print('%s %s drop %g: %d of %d entries kept, %d rows left out, smallest gap %.3g'
          % (which, config, drop, o.nnz, o.before, left_out, float(o.gaps.min())))
    assert left_out <= n // 100
    G, f = built_filtered(A, levels, steps, step_size, drop, bits=32, max_row=max_row)
    assert f['nnz'] == G.nnz == int(G.indptr[-1]) and G.shape == (n, n)
    assert f['longest'] == int(np.diff(G.indptr).max())
    D = wide_dense(A)
    worst = 0.0
    for i in range(n):
        p = row_of(G, i)
        if o.compared[i]:
            assert np.array_equal(p, o.rows[i]), (which, config, drop, i)
        else:
            assert p[-1] == i and np.all(np.diff(p) > 0)
        worst = max(worst, check_row(G, i, p, D[np.ix_(p, p)], A.dtype.type))
    print('largest residual / bound: %.3g' % worst)
    if left_out == 0:
        assert (f['removed'], f['nnz'], f['longest']) == (o.removed, o.nnz, o.longest), (f, o.removed, o.nnz, o.longest)
        assert f['truncated'] == o.truncated


# ---------------------------------------------------------------- 2. the rule against the library itself
def rule(which, config, drop):
    """The removed entries are those with r < drop, r from the unfiltered G as the library stored it and A's diagonal.
    The test forms r with a division and square roots, the library without: an entry within 1e-12 of the threshold (a
    few roundings of 2^-53 on either side) is not judged."""
    levels, steps, step_size, max_row = config
    A = matrix(which)
    n = A.shape[0]
    G0, f0 = built_plain(A, levels, steps, step_size, bits=32, max_row=max_row)
    G, f = built_filtered(A, levels, steps, step_size, drop, bits=32, max_row=max_row)
    assert f['truncated'] == f0['truncated'] and f['removed'] == G0.nnz - G.nnz and f['nnz'] == G.nnz
    diag = hermitian_from_upper(A).diagonal().real.astype(np.float64)
    judged = 0
    for i in range(n):
        p0, p = row_of(G0, i), row_of(G, i)
        assert np.all(np.isin(p, p0)) and p[-1] == i, i
        g = G0.data[G0.indptr[i]:G0.indptr[i + 1]].astype(np.complex128 if A.dtype.kind == 'c' else np.float64)
        r = np.abs(g[:-1]) * np.sqrt(diag[p0[:-1]]) / (g[-1].real * np.sqrt(diag[i]))
        sure = np.abs(r / drop - 1.0) > 1e-12
        assert np.array_equal(np.isin(p0[:-1], p)[sure], (r >= drop)[sure]), i
        judged += int(sure.sum())
    assert judged >= (G0.nnz - n) - n // 100
    assert 0 < f['removed'] < G0.nnz - n or drop == 0.3


# ---------------------------------------------------------------- 3. nothing to remove, everything removed
def nothing_to_remove():
    A = lv.lap('d')
    assert oracle(A, 1, 0, 1, 64, 0.03).removed == 0
    for host in (False, True):
        G, f = built_filtered(A, drop=0.03, host=host)
        G0, f0 = built_plain(A, host=host)
        assert same_bits(G, G0) and f['removed'] == 0
        assert (f['nnz'], f['longest'], f['truncated']) == (f0['nnz'], f0['longest'], f0['truncated'])


def everything_removed():
    A = base.matrix('d')
    n = A.shape[0]
    G, f = built_filtered(A, drop=0.3, bits=32)
    G0, _ = built_plain(A, bits=32)
    assert np.array_equal(G.indptr, np.arange(n + 1)) and np.array_equal(G.indices, np.arange(n))
    want = np.array([base.rsqrt_rounded(float(d)) for d in A.diagonal().real]).astype(A.dtype)
    assert np.array_equal(G.data, want)
    assert f['longest'] == 1 <= base.SHORT and f['nnz'] == n and f['removed'] == G0.nnz - n > 0      # every row in the 8-lane bin


# ---------------------------------------------------------------- 4. diagonal scaling by powers of two
def scaling(which, config, drop, exact=True):
    """exact: G' = G D^-1 bit for bit (the library: every operation of its build commutes with a scaling by powers of
    two).  The stand-in solves by LAPACK's pivoted LU, whose pivots a scaling moves: there the rows the oracle compares
    have equal patterns and every row has the defining property on the scaled matrix."""
    levels, steps, step_size, max_row = config
    A = matrix(which)
    n = A.shape[0]
    rng = np.random.default_rng(51)
    d = 2.0 ** rng.integers(-20, 21, n)
    B = sp.csr_matrix(sp.diags(d) @ A.astype(np.complex128 if A.dtype.kind == 'c' else np.float64) @ sp.diags(d)).astype(A.dtype)
    B.sort_indices()
    assert np.array_equal(B.indptr, A.indptr) and np.array_equal(B.indices, A.indices)
    assert np.array_equal(B.data, A.data * (d[np.repeat(np.arange(n), np.diff(A.indptr))] * d[A.indices]).astype(A.real.dtype))
    G, f = built_filtered(A, levels, steps, step_size, drop, bits=32, max_row=max_row)
    Gs, fs = built_filtered(B, levels, steps, step_size, drop, bits=32, max_row=max_row)
    assert 0 < f['removed']
    if exact:
        want = sp.csr_matrix((G.data / d[G.indices].astype(G.real.dtype), G.indices, G.indptr), shape=G.shape)
        assert same_bits(Gs, want)
        assert (fs['removed'], fs['nnz'], fs['longest'], fs['truncated']) == (f['removed'], f['nnz'], f['longest'], f['truncated'])
        return
    o = oracle(A, levels, steps, step_size, max_row, drop)
    D = wide_dense(B)
    for i in range(n):
        p = row_of(Gs, i)
        if o.compared[i]:
            assert np.array_equal(p, row_of(G, i)), i
        check_row(Gs, i, p, D[np.ix_(p, p)], A.dtype.type)


# ---------------------------------------------------------------- 5. quality lies between the unfiltered and the diagonal G
def kaporin_order():
    out = []
    for A, levels in ((lv.lap('d', 8, 8, 8), 3), (lv.banded('d', narrow=True), 2)):
        n = A.shape[0]
        d = hermitian_from_upper(A).toarray()
        s = 1 / np.sqrt(np.diag(d))
        G0, f0 = built_plain(A, levels, bits=32)
        assert f0['truncated'] == 0
        ks = [kaporin(G0.toarray() @ d @ G0.toarray().T)]
        for drop in (0.02, 0.1):
            G, f = built_filtered(A, levels, drop=drop, bits=32)
            assert 0 < f['removed'] < G0.nnz - n, drop
            ks.append(kaporin(G.toarray() @ d @ G.toarray().T))
        ks.append(kaporin(d * s[:, None] * s[None, :]))
        print('Kaporin numbers (n = %d, level %d): unfiltered %.6f, drop 0.02 %.6f, drop 0.1 %.6f, diagonal %.6f' % ((n, levels) + tuple(ks)))
        slack = 1 + 100 * n * base.unit(np.float64)
        assert ks[0] <= ks[1] * slack and ks[1] <= ks[3] * slack and ks[0] <= ks[2] * slack and ks[2] <= ks[3] * slack
        out.append(ks)
    return out


# ---------------------------------------------------------------- 6. the bins
def bins(code, monkeypatch):
    A = lv.banded(code)
    monkeypatch.setenv('RLH_FSAI_BINS', '0')
    two, f2 = built_filtered(A, 2, drop=0.03, bits=32)
    monkeypatch.delenv('RLH_FSAI_BINS')
    four, f4 = built_filtered(A, 2, drop=0.03, bits=32)
    assert same_bits(two, four) and f2 == dict(f4, seconds=f2['seconds'])
    before, _ = built_plain(A, 2, bits=32)
    lens0, lens = np.diff(before.indptr), np.diff(four.indptr)
    for lo, hi in lv.CLASSES[:4]:
        assert np.any((lens0 >= lo) & (lens0 <= hi)), (lo, hi)
    after = sum(bool(np.any((lens >= lo) & (lens <= hi))) for lo, hi in lv.CLASSES[:4])
    moved = int(np.sum((lens0 > 8) & (lens <= 8)))
    print('rows per class after filtering: %s; %d rows moved to the 8-lane bin'
          % ([int(np.sum((lens >= lo) & (lens <= hi))) for lo, hi in lv.CLASSES[:4]], moved))
    assert after >= 2 and moved > 0


# ---------------------------------------------------------------- 7. past one pass of the filter's grid (GPU tier)
def loops(cu):
    """A band of w = 4 with random values at level 1: rows of 5 entries, all on the 8-lane path before and after
    filtering (the pass boundary of the second set-up is that of the filter), more of them than one pass holds."""
    w, drop = 4, 0.1
    per_pass = cu * BLOCKS_PER_CU * FILTER_ROWS_PER_BLOCK
    n = per_pass + 300
    A = lv.band(np.full(n, w), np.float64, 52)
    G, f = built_filtered(A, drop=drop, bits=32)
    assert 0 < f['removed'] < 4 * n - 10 and f['nnz'] == G.nnz == 5 * n - 10 - f['removed'] and f['longest'] <= 5
    M = ad.Dense(A)
    assert M.D is None
    rows = [0, 1, w, per_pass - 1, per_pass, per_pass + 1, n - 1]
    dropped = 0
    for i in rows:
        P = np.arange(max(i - w, 0), i + 1)
        p, gap = oracle_row(M, P, drop)
        assert gap >= GAP, (i, gap)
        dropped += P.size - p.size
        check_row(G, i, p, M.block(p, p).astype(np.longdouble), np.float64)           # (asserts the pattern too)
    assert dropped > 0


# ---------------------------------------------------------------- 8. with a plan
def with_plan(work):
    from raleigh_amd.algebra.hip import Vectors
    from raleigh_amd.algebra.hip.precond import ApproximateInverse
    A = base.matrix('d')
    n, m = A.shape[0], 9
    plain = ApproximateInverse(A, drop=0.03)
    T = ApproximateInverse(A, drop=0.03, work=work)
    G = plain.csr()
    assert same_bits(T.csr(), G) and T.nnz == plain.nnz == G.nnz and T.dropped_entries == plain.dropped_entries > 0
    f = wk.plan_info(T._plan)
    sliced = 2 * T.nnz - f['tail']                          # entries of the filtered G and G^H outside the tails
    assert f['work'] == wk.WORKS[work] and 0 <= f['tail'] and sliced <= f['slots'] <= 2 * sliced
    full = ApproximateInverse(A, work=work)
    g = wk.plan_info(full._plan)
    assert f['slots'] + f['tail'] < g['slots'] + g['tail'] and T.algorithmic_bytes(m) < full.algorithmic_bytes(m)
    x = wk.random_block(np.random.default_rng(53), m, n, np.float64)
    y, y0 = Vectors(np.zeros((m, n))), Vectors(np.zeros((m, n)))
    T.apply(Vectors(x.copy()), y)
    plain.apply(Vectors(x.copy()), y0)
    wk.Reference(G, np.float64, work).check(x, y.data())
    wk.Reference(G, np.float64, 'native').check(x, y0.data())


# ---------------------------------------------------------------- 9. the class: kinds of input, and no drop
def class_inputs(device):
    from raleigh_amd.algebra.hip.precond import ApproximateInverse
    A = lv.banded('d')
    want, f = built_filtered(A, 2, drop=0.03, bits=64)
    wh, fh = built_filtered(A, 2, drop=0.03, host=True)
    w32, _ = built_filtered(A, 2, drop=0.03, bits=32)
    assert same_bits(wh, want) and same_bits(w32, want) and fh == dict(f, seconds=fh['seconds'])
    before, _ = built_plain(A, 2)
    made = [ApproximateInverse(A, levels=2, drop=0.03), ApproximateInverse(csr_tensor(A, device, np.int32), levels=2, drop=0.03),
            ApproximateInverse(csr_tensor(A, device, np.int64), levels=2, drop=0.03),
            ApproximateInverse(csr_tensor(A, 'cpu'), levels=2, drop=0.03)]
    for T in made:
        assert (T.levels, T.steps, T.drop) == (2, 0, 0.03) and same_bits(T.csr(), want)
        assert filtered_of(T._h) == (0.03, f['removed']) and T.dropped_entries == f['removed'] == before.nnz - want.nnz > 0
        assert T.truncated_rows == f['truncated'] > 0 and T.longest_row == f['longest'] and T.nnz == want.nnz
        assert abs(T.fill - want.nnz / A.nnz) < 1e-15
        assert T.algorithmic_bytes(4) == 2 * want.nnz * 12 + 4 * A.shape[0] * 4 * 8
    return made


def unchanged_without_drop(code, device):
    from raleigh_amd.algebra.hip.precond import ApproximateInverse
    A = base.matrix(code)
    for kw, raw in (({}, lambda: base.built(A, bits=32)), ({'levels': 2}, lambda: base.built(A, '_levels', 2, bits=32)),
                    ({'steps': 2}, lambda: base.built(A, '_adaptive', 1, 2, 1, bits=32))):
        want, f = raw()
        for T in (ApproximateInverse(A, **kw), ApproximateInverse(A, drop=0.0, **kw), ApproximateInverse(A, drop=0, **kw),
                  ApproximateInverse(csr_tensor(A, device), drop=0.0, **kw)):
            assert same_bits(T.csr(), want) and T.drop == 0.0 and T.dropped_entries == 0 and T.nnz == f['nnz']
            assert filtered_of(T._h) == (0.0, 0)


# ---------------------------------------------------------------- 10. device memory
def device_memory():
    def live():
        nbytes, nblocks = ctypes.c_int64(-1), ctypes.c_int64(-1)
        _check(_L().rlh_device_live(ctypes.byref(nbytes), ctypes.byref(nblocks)))
        return nbytes.value, nblocks.value
    A = lv.banded('d')
    first = live()
    for host in (True, False):
        rc, h = create_filtered(A, 2, 2, 2, 0.03, host=host)
        _check(rc)
        assert live()[0] >= first[0]
        destroy(h)
        assert live() == first
        rc, h = create_filtered(ad.indefinite(), 1, 1, 1, 0.03, host=host)
        assert rc != 0 and not h.value and 'local block of row 21 is not positive definite' in last_error()
        assert live() == first


# ---------------------------------------------------------------- 11. rejections
def rejections_raw():
    A = base.matrix('d')
    for host, name in ((False, 'rlh_fsfilter_create_device'), (True, 'rlh_fsfilter_create')):
        for drop, shown in ((0.0, '0'), (1.0, '1'), (-0.1, '-0.1'), (float('inf'), 'inf'), (float('nan'), 'nan')):
            rc, h = create_filtered(A, drop=drop, host=host)
            assert rc != 0 and not h.value, (name, drop)
            text = last_error()
            assert '%s: drop must lie in (0, 1), got ' % name in text and text.endswith(shown), text
        for kw, text in (({'max_row': 65}, 'max_row must lie in [1, 64], got 65'), ({'max_row': 0}, 'max_row must lie in [1, 64], got 0'),
                         ({'levels': 0}, 'levels must lie in [1, 8], got 0'), ({'levels': 9}, 'levels must lie in [1, 8], got 9'),
                         ({'steps': 64}, 'steps must lie in [1, 63], got 64'), ({'steps': -1}, 'steps must lie in [1, 63], got -1'),
                         ({'steps': 1, 'step_size': 0}, 'step_size must lie in [1, 16], got 0'),
                         ({'steps': 1, 'step_size': 17}, 'step_size must lie in [1, 16], got 17'),
                         ({'max_row': 65, 'drop': 2.0}, 'max_row must lie in [1, 64], got 65')):
            rc, h = create_filtered(A, host=host, **kw)
            assert rc != 0 and not h.value, (name, kw)
            assert last_error().endswith('%s: %s' % (name, text)), last_error()
        rc, h = create_filtered(A, 1, 0, 99, 0.5, host=host)          # steps == 0: step_size is not looked at
        _check(rc)
        assert base.adaptive_of(h) == (0, 0) and filtered_of(h)[0] == 0.5
        destroy(h)
    rc, h = base.create(A)                                       # a handle of another entry point answers (0, 0)
    _check(rc)
    assert filtered_of(h) == (0.0, 0)
    destroy(h)
    assert _L().rlh_fsfilter_info(None, None, None) != 0 and 'rlh_fsfilter_info: null handle or output' in last_error()


def rejections_class(fake=None):
    from raleigh_amd.algebra.hip.precond import ApproximateInverse
    A = base.matrix('d')
    before = dict(fake.calls) if fake is not None else None
    for drop, shown in ((1.0, '1'), (-0.1, r'-0\.1'), (2.5, r'2\.5'), (float('inf'), 'inf'), (float('nan'), 'nan')):
        with pytest.raises(ValueError, match=r'drop must lie in \[0, 1\), got %s' % shown):
            ApproximateInverse(A, drop=drop)
    with pytest.raises(ValueError, match='max_row'):
        ApproximateInverse(A, max_row=65, drop=0.1)
    with pytest.raises(ValueError, match='levels'):
        ApproximateInverse(A, levels=9, drop=0.1)
    with pytest.raises(ValueError, match='work must be'):
        ApproximateInverse(A, drop=0.1, work='float16')
    if fake is not None:
        assert dict(fake.calls) == before                   # refused before any library call


# ---------------------------------------------------------------- 12. end to end
def end_to_end(device):
    import scipy.linalg
    import torch
    from raleigh_amd.interfaces import partial_hevp
    from raleigh_amd.algebra.hip.precond import ApproximateInverse
    A = lv.lap('d', 12, 11, 10)
    which = 6
    exact = scipy.linalg.eigvalsh(hermitian_from_upper(A).toarray())[:which]
    a = csr_tensor(A, device)
    its, nnz = {}, {}
    for drop in (0.02, 0.0):
        T = ApproximateInverse(a, levels=3, drop=drop)
        nnz[drop] = T.nnz
        np.random.seed(1)
        lmd, x, status = partial_hevp(a, T=T, which=which, tol=1e-6, verb=-1)
        its[drop] = partial_hevp.last['iterations']
        assert status == 0
        if drop:
            assert T.dropped_entries > 0
            assert np.max(np.abs(lmd[:which] - exact)) <= 1e-10
            assert isinstance(x, torch.Tensor) and x.device.type == torch.device(device).type
    print('level 3: %d iterations on %d entries with drop=0.02, %d iterations on %d entries without'
          % (its[0.02], nnz[0.02], its[0.0], nnz[0.0]))
    assert nnz[0.02] < nnz[0.0]
    return its, nnz
