"""Prefiltration of the approximate inverse's pattern by value (rlh_fsthreshold_create*, rlh_fsthreshold_info,
ApproximateInverse(prefilter=...)): cases shared by the CPU tier (tests/fake_fsai.py) and the GPU tier.
Matrices, helpers and the bound of the defining property (`check_row`, `beta`) come from tests/_fsai_cases.py (`base`),
the banded and Laplacian matrices and the idea of the pattern oracle from tests/_fsai_levels_cases.py (`lv`), the matrix
names and `wide_dense` from tests/_fsai_filter_cases.py (`fl`), the raw update from tests/_fsai_values_cases.py (`vl`).

THE ORACLE (`Oracle`) is written from the rule in include/rlhip.h and shares nothing with the library or the stand-in.
For every stored entry (i, j), j < i, of A it forms, in longdouble, with the division and the roots,
    r_ij = |a_ji| / sqrt(a_ii a_jj),
a_ji the partner stored above the diagonal (nothing below it is read) and a_ii, a_jj the real diagonals; the entry is
strong iff r_ij >= tau (false for a NaN).  With T the boolean pattern of the strong entries and the diagonal, the level
pattern is that of T^levels by SciPy sparse products, cut to the max_row largest columns of every row after EVERY
level; a row is truncated when any level had more.

WHAT IS COMPARED EXACTLY.  The library decides by |a_ji|^2 >= (tau^2 a_ii) a_jj in double, without division or root.
Float32 inputs widen exactly, so only a few roundings of 2^-53 separate the two evaluations.  A row any of whose
decisions -- its own entries or those of a row it can reach within its levels (judged on the unthresholded pattern,
which holds every thresholded one) -- has |r / tau - 1| < GAP = 1e-12 is left out of the exact comparison (its pattern
must still pass `check_row`); at most 1 % of a case's rows may be left out, which every case asserts.

LAUNCH GEOMETRY the loop case relies on: the two kernels that decide the entries and fill the strong lower structure
(fsai_strong) take 8 lanes per row, 256 threads per workgroup -- 32 rows per workgroup -- on at most 8 workgroups per
CU, in a grid-stride loop: one pass covers CU * 8 * 32 rows.  The pattern kernels that follow (every level, 1 included)
take 4 rows per workgroup (one wave each) on at most 8 workgroups per CU; the 8-lane set-up 32 rows, the 16-lane set-up
16 rows per workgroup (tests/_fsai_cases.py, tests/_fsai_levels_cases.py).
"""

import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import _fsai_cases as base
import _fsai_levels_cases as lv
import _fsai_filter_cases as fl
import _fsai_values_cases as vl
import _fsai_work_cases as wk
from _fsai_cases import TYPES, _L, _check, check_row, csr_tensor, destroy, get, hermitian_from_upper, info, kaporin, last_error, same_bits
from _fsai_filter_cases import matrix, row_of, wide_dense

GAP = 1e-12
BLOCKS_PER_CU = 8
STRONG_ROWS_PER_BLOCK = 32
PATTERN_ROWS_PER_BLOCK = 4
PATTERN_CASES = ([(which, tau) for which in ('profile-d', 'profile-s', 'profile-c', 'profile-z', 'banded-d', 'cut-d') for tau in (0.02, 0.05)]
                 + [('lap', 0.2)])
LEVELS = (1, 2, 3)


# ---------------------------------------------------------------- the raw entry points
def create(A, prefilter, levels=1, steps=0, step_size=1, drop=0.0, host=False, bits=64, max_row=64, null=()):
    """(rc, handle) of rlh_fsthreshold_create on A's arrays (host=True) or rlh_fsthreshold_create_device on device copies
    of them; null: positions among the three arrays passed as null pointers."""
    from raleigh_amd import _lib
    it = {32: np.int32, 64: np.int64}.get(bits, np.int64)
    arrays = (A.indptr.astype(np.int64 if host else it), A.indices.astype(np.int32 if host else it), np.ascontiguousarray(A.data))
    h = ctypes.c_void_p(12345)
    head = (ctypes.byref(h), _lib.DTYPE_CODE[A.dtype.type], A.shape[0])
    tail = (max_row, levels, steps, step_size, drop, prefilter)
    if host:
        return _L().rlh_fsthreshold_create(*head, *[None if k in null else _lib.host_ptr(a) for k, a in enumerate(arrays)], *tail), h
    bufs = [base.dev(a) for a in arrays]
    return _L().rlh_fsthreshold_create_device(*head, bits, *[None if k in null else b.ptr for k, b in enumerate(bufs)], *tail), h


def threshold_of(h):
    tau, weak = ctypes.c_double(-1.0), ctypes.c_int64(-1)
    _check(_L().rlh_fsthreshold_info(h, ctypes.byref(tau), ctypes.byref(weak)))
    return tau.value, weak.value


def built(A, prefilter, levels=1, steps=0, step_size=1, drop=0.0, **kw):
    """G (SciPy) and the info record, with the weak entries under 'weak' and the dropped ones under 'removed', of a
    thresholded build that must succeed."""
    rc, h = create(A, prefilter, levels, steps, step_size, drop, **kw)
    _check(rc)
    try:
        assert base.levels_of(h) == levels and base.adaptive_of(h) == ((steps, step_size) if steps else (0, 0))
        f = info(h)
        got, f['weak'] = threshold_of(h)
        assert got == prefilter
        got, f['removed'] = fl.filtered_of(h)
        assert got == drop
        return get(h, A.dtype.type), f
    finally:
        destroy(h)


def live():
    nbytes, nblocks = ctypes.c_int64(-1), ctypes.c_int64(-1)
    _check(_L().rlh_device_live(ctypes.byref(nbytes), ctypes.byref(nblocks)))
    return nbytes.value, nblocks.value


# ---------------------------------------------------------------- the oracle
def ratios(A):
    """Rows, columns and r of the stored entries below the diagonal (r is NaN where the partner is NaN or missing)."""
    n = A.shape[0]
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(A.indptr))
    cols = A.indices.astype(np.int64)
    u = sp.triu(A, format='coo')
    key = u.row.astype(np.int64) * n + u.col
    order = np.argsort(key)
    key, val = key[order], u.data[order].astype(np.clongdouble)
    low = cols < rows
    i, j = rows[low], cols[low]
    at = np.minimum(np.searchsorted(key, j * n + i), key.size - 1)
    a = np.where(key[at] == j * n + i, val[at], np.nan)
    d = np.zeros(n, dtype=np.longdouble)
    on = u.row == u.col
    d[u.row[on]] = u.data[on].real.astype(np.longdouble)
    with np.errstate(all='ignore'):
        r = np.abs(a) / np.sqrt(d[i] * d[j])
    return i, j, r


def capped(P, max_row):
    """The max_row largest columns of every row of a CSR pattern with sorted columns, and the rows that had more."""
    lens = np.diff(P.indptr)
    at = np.arange(P.nnz) - np.repeat(P.indptr[:-1], lens)
    keep = at >= np.repeat(lens - max_row, lens)
    indptr = np.zeros(P.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.minimum(lens, max_row), out=indptr[1:])
    return sp.csr_matrix((np.ones(int(keep.sum())), P.indices[keep], indptr), shape=P.shape), lens > max_row


class Oracle:
    def __init__(self, A, tau, levels, max_row):
        n = A.shape[0]
        i, j, r = ratios(A)
        with np.errstate(all='ignore'):
            strong = r >= np.longdouble(tau)
            near = ~(np.abs(r / np.longdouble(tau) - 1) >= GAP) & ~np.isnan(r)
        self.weak, self.near, self.strong_share = int(np.sum(~strong)), int(near.sum()), float(strong.mean()) if r.size else 1.0
        finite = r[~np.isnan(r)]
        self.smallest_gap = float(np.min(np.abs(finite / np.longdouble(tau) - 1))) if finite.size else np.inf
        T = sp.csr_matrix((np.ones(int(strong.sum()) + n), (np.concatenate([i[strong], np.arange(n)]),
                                                           np.concatenate([j[strong], np.arange(n)]))), shape=(n, n))
        T.sort_indices()
        P, over = capped(T, max_row)
        for _ in range(levels - 1):
            P = sp.csr_matrix(P @ T)
            P.data[:] = 1.0
            P.sort_indices()
            P, more = capped(P, max_row)
            over = over | more
        self.indptr, self.indices = P.indptr.astype(np.int64), P.indices.astype(np.int64)
        self.truncated, self.longest, self.nnz = int(over.sum()), int(np.diff(P.indptr).max()), int(P.nnz)
        touched = np.bincount(i[near], minlength=n) > 0                 # rows with a decision too close to call
        if levels > 1 and touched.any():
            touched = touched | ((lv.full_pattern(A, levels - 1) @ touched.astype(np.float64)) > 0)
        self.compared = ~touched
        self.left_out = int(touched.sum())

    def row(self, i):
        return self.indices[self.indptr[i]:self.indptr[i + 1]]


_KEPT = {}


@functools.lru_cache(maxsize=None)
def _oracle(A_id, tau, levels, max_row):
    return Oracle(_KEPT[A_id], tau, levels, max_row)


def oracle(A, tau, levels, max_row=64):
    """Computed once per matrix object and configuration, never written."""
    _KEPT[id(A)] = A
    return _oracle(id(A), tau, levels, max_row)


def compare_pattern(G, f, o, what):
    """The pattern of G and the counts of its info record against the oracle; rows left out are only well formed."""
    n = G.shape[0]
    assert o.left_out <= n // 100, (what, o.left_out)
    assert f['nnz'] == G.nnz == int(G.indptr[-1]) and f['longest'] == int(np.diff(G.indptr).max()), what
    if o.left_out == 0:
        assert np.array_equal(G.indptr, o.indptr) and np.array_equal(G.indices, o.indices), what
        assert (f['nnz'], f['truncated'], f['longest'], f['weak']) == (o.nnz, o.truncated, o.longest, o.weak), (what, f)
        return
    assert abs(f['weak'] - o.weak) <= o.near, what
    for i in range(n):
        p = row_of(G, i)
        if o.compared[i]:
            assert np.array_equal(p, o.row(i)), (what, i)
        else:
            assert p[-1] == i and np.all(np.diff(p) > 0), (what, i)


# ---------------------------------------------------------------- 1. the pattern, exactly
def gaps():
    """The taus of the cases stay clear of every ratio of the matrices they are used on."""
    for which, tau in PATTERN_CASES + [('lap', 0.02), ('profile-d', 0.5)]:
        o = oracle(matrix(which), tau, 1)
        print('%s tau %g: %.1f %% strong, smallest |r / tau - 1| %.3g' % (which, tau, 100 * o.strong_share, o.smallest_gap))
        assert o.left_out == 0 and o.smallest_gap >= GAP


def pattern(which, tau, levels):
    A = matrix(which)
    for max_row in (64, 5):
        o = oracle(A, tau, levels, max_row)
        print('%s tau %g level %d max_row %d: %d entries, %d weak, %d rows cut, longest %d, %d rows left out'
              % (which, tau, levels, max_row, o.nnz, o.weak, o.truncated, o.longest, o.left_out))
        for host, bits in ((False, 32), (False, 64), (True, 64)):
            G, f = built(A, tau, levels, host=host, bits=bits, max_row=max_row)
            compare_pattern(G, f, o, (which, tau, levels, max_row, host, bits))


def cut_is_exercised():
    """The shapes the cases rely on: full level patterns far beyond max_row on the profile matrix at tau = 0.02, short rows
    at 0.05; every class of the bins on the banded one."""
    A = matrix('profile-d')
    assert oracle(A, 0.02, 2, 10 ** 6).longest > 64 and oracle(A, 0.02, 3, 10 ** 6).longest > 64
    assert oracle(A, 0.02, 2).truncated > 0 and oracle(A, 0.02, 3).truncated > 0
    assert oracle(A, 0.05, 1).nnz < 2 * A.shape[0]
    o = oracle(matrix('banded-d'), 0.02, 2)
    lens = np.diff(o.indptr)
    for lo, hi in lv.CLASSES[:4]:
        assert np.any((lens >= lo) & (lens <= hi)), (lo, hi)


# ---------------------------------------------------------------- 2. the values: the block of the FULL matrix
def values(code, tau=0.02, levels=2):
    A = base.matrix(code)
    D = base.dense_wide(code)
    o = oracle(A, tau, levels)
    G, f = built(A, tau, levels, bits=32)
    compare_pattern(G, f, o, (code, tau, levels))
    assert 0 < o.weak and o.truncated > 0
    inside = 0                                                  # weak entries inside the blocks: they belong to S
    i_, j_, r = ratios(A)
    weak = sp.csr_matrix((np.ones(int(np.sum(r < tau))), (i_[r < tau], j_[r < tau])), shape=A.shape)
    worst = 0.0
    for i in range(A.shape[0]):
        p = row_of(G, i)
        inside += int(weak[p][:, p].nnz)
        worst = max(worst, check_row(G, i, p, D[np.ix_(p, p)], TYPES[code]))
    print('largest residual / bound: %.3g; %d weak entries lie inside the blocks' % (worst, inside))
    assert inside > 0


# ---------------------------------------------------------------- 3. nothing weak, 4. everything weak
def nothing_weak():
    A = lv.lap('d')
    for levels in LEVELS:
        assert oracle(A, 0.02, levels).weak == 0
        for host in (False, True):
            G, f = built(A, 0.02, levels, host=host)
            G0, f0 = fl.built_plain(A, levels, host=host)
            assert same_bits(G, G0) and f['weak'] == 0, (levels, host)
            assert (f['nnz'], f['longest'], f['truncated']) == (f0['nnz'], f0['longest'], f0['truncated'])


def everything_weak():
    A = base.matrix('d')
    n = A.shape[0]
    i, j, r = ratios(A)
    assert float(r.max()) < 0.2 and r.size > 0                  # the largest ratio of the profile matrix is 0.158
    for levels in (1, 3):
        G, f = built(A, 0.5, levels, bits=32)
        assert np.array_equal(G.indptr, np.arange(n + 1)) and np.array_equal(G.indices, np.arange(n))
        want = np.array([base.rsqrt_rounded(float(d)) for d in A.diagonal().real]).astype(A.dtype)
        assert np.array_equal(G.data, want)                     # (1 / sqrt(a_ii), rounded once to the storage type)
        assert f['longest'] == 1 and f['nnz'] == n and f['weak'] == r.size and f['truncated'] == 0


# ---------------------------------------------------------------- 5. the lower triangle is never read
def lower_never_read(code):
    A = base.matrix(code)
    B = A.copy()
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    B.data[B.indices < rows] = np.nan
    for levels in (1, 2):
        G, f = built(A, 0.02, levels, bits=32)
        Gn, fn = built(B, 0.02, levels, bits=32)
        assert same_bits(G, Gn) and fn == dict(f, seconds=fn['seconds'])


def nan_above_is_weak():
    """A NaN at the upper entry (i - 1, i) of the 7-point Laplacian: the entry (i, i - 1) is weak, row i loses column i - 1, and
    at level 1 no other row holds both i - 1 and i (the members of a row differ by 1 only as (k - 1, k)): the build succeeds."""
    A = lv.lap('d')
    n, i = A.shape[0], 44
    assert i % 6 != 0
    B = A.copy()
    k = int(np.flatnonzero(A.indices[A.indptr[i - 1]:A.indptr[i]] == i)[0]) + int(A.indptr[i - 1])
    B.data[k] = np.nan
    o, ob = oracle(A, 0.02, 1), oracle(B, 0.02, 1)
    assert o.weak == 0 and ob.weak == 1 and ob.left_out == 0 and ob.nnz == o.nnz - 1
    assert np.array_equal(ob.row(i), np.setdiff1d(o.row(i), [i - 1]))
    D = wide_dense(A)
    for host in (False, True):
        G, f = built(B, 0.02, 1, host=host)
        compare_pattern(G, f, ob, host)
        for q in range(n):
            p = row_of(G, q)
            check_row(G, q, p, D[np.ix_(p, p)], np.float64)     # (no block holds the NaN)


# ---------------------------------------------------------------- 6. diagonal scaling by powers of two
def scaling(which, tau, levels, exact=True):
    """The patterns are equal exactly.  exact: G' = G D^-1 bit for bit (the library: every operation of its build commutes
    with a scaling by powers of two).  The stand-in solves by LAPACK's pivoted LU, whose pivots a scaling moves: there every
    row has the defining property on the scaled matrix."""
    A = matrix(which)
    n = A.shape[0]
    rng = np.random.default_rng(61)
    d = 2.0 ** rng.integers(-20, 21, n)
    B = sp.csr_matrix(sp.diags(d) @ A.astype(np.complex128 if A.dtype.kind == 'c' else np.float64) @ sp.diags(d)).astype(A.dtype)
    B.sort_indices()
    assert np.array_equal(B.indptr, A.indptr) and np.array_equal(B.indices, A.indices)
    assert np.array_equal(B.data, A.data * (d[np.repeat(np.arange(n), np.diff(A.indptr))] * d[A.indices]).astype(A.real.dtype))
    G, f = built(A, tau, levels, bits=32)
    Gs, fs = built(B, tau, levels, bits=32)
    assert 0 < f['weak']
    assert np.array_equal(Gs.indptr, G.indptr) and np.array_equal(Gs.indices, G.indices)
    assert (fs['weak'], fs['nnz'], fs['longest'], fs['truncated']) == (f['weak'], f['nnz'], f['longest'], f['truncated'])
    if exact:
        want = sp.csr_matrix((G.data / d[G.indices].astype(G.real.dtype), G.indices, G.indptr), shape=G.shape)
        assert same_bits(Gs, want)
        return
    D = wide_dense(B)
    for i in range(n):
        p = row_of(Gs, i)
        check_row(Gs, i, p, D[np.ix_(p, p)], A.dtype.type)


# ---------------------------------------------------------------- 7. nested patterns
def _inside(G_small, G_big):
    a = sp.csr_matrix((np.ones(G_small.nnz), G_small.indices, G_small.indptr), shape=G_small.shape)
    b = sp.csr_matrix((np.ones(G_big.nnz), G_big.indices, G_big.indptr), shape=G_big.shape)
    return (a - a.multiply(b)).nnz == 0


def nested():
    A = lv.banded('d', narrow=True)
    n = A.shape[0]
    d = hermitian_from_upper(A).toarray()
    slack = 1 + 100 * n * base.unit(np.float64)                 # (that of lv.monotone_quality)

    def number(G):
        g = G.toarray()
        return kaporin(g @ d @ g.T)
    by_tau = []
    for tau in (0.02, 0.05, 0.1):
        G, f = built(A, tau, 2, bits=32)
        assert f['truncated'] == 0 and f['weak'] > 0, tau
        by_tau.append((G, number(G), f))
    assert by_tau[0][2]['longest'] == 43
    print('Kaporin numbers at level 2, tau 0.02, 0.05, 0.1 (n = %d): %.6f %.6f %.6f' % ((n,) + tuple(k for _, k, _ in by_tau)))
    for (Ga, ka, fa), (Gb, kb, fb) in zip(by_tau, by_tau[1:]):
        assert _inside(Gb, Ga) and fb['weak'] >= fa['weak'] and Gb.nnz < Ga.nnz
        assert ka <= kb * slack
    by_level = []
    for levels in LEVELS:
        G, f = built(A, 0.05, levels, bits=32)
        assert f['truncated'] == 0, levels
        by_level.append((G, number(G), f))
    assert by_level[2][2]['longest'] == 34
    print('Kaporin numbers at tau 0.05, levels 1, 2, 3: %.6f %.6f %.6f' % tuple(k for _, k, _ in by_level))
    for (Ga, ka, _), (Gb, kb, _) in zip(by_level, by_level[1:]):
        assert _inside(Ga, Gb) and kb <= ka * slack
    return by_tau, by_level


# ---------------------------------------------------------------- 8. composition
def with_steps():
    A = matrix('profile-d')
    n, tau, levels = A.shape[0], 0.05, 2
    o = oracle(A, tau, levels)
    G, f = built(A, tau, levels, 2, 2, bits=32)
    G0, f0 = built(A, tau, levels, bits=32)
    assert f['weak'] == f0['weak'] == o.weak and G.nnz > G0.nnz and o.left_out == 0
    D = wide_dense(A)
    grown = 0
    for i in range(n):
        p = row_of(G, i)
        assert np.all(np.isin(o.row(i), p)) and len(p) <= len(o.row(i)) + 4, i
        grown += int(len(p) > len(o.row(i)))
        check_row(G, i, p, D[np.ix_(p, p)], np.float64)
    assert grown > n // 2


def with_drop(drop=0.03):
    """The rule of post-filtration (`rule` of tests/_fsai_filter_cases.py) against the undropped build of the same prefilter."""
    A = matrix('banded-d')
    n, tau, levels = A.shape[0], 0.02, 2
    G0, f0 = built(A, tau, levels, bits=32)
    G, f = built(A, tau, levels, drop=drop, bits=32)
    assert f['truncated'] == f0['truncated'] and f['weak'] == f0['weak'] and f['removed'] == G0.nnz - G.nnz and f['nnz'] == G.nnz
    diag = hermitian_from_upper(A).diagonal().real.astype(np.float64)
    D = wide_dense(A)
    judged = 0
    for i in range(n):
        p0, p = row_of(G0, i), row_of(G, i)
        assert np.all(np.isin(p, p0)) and p[-1] == i, i
        g = G0.data[G0.indptr[i]:G0.indptr[i + 1]].astype(np.float64)
        r = np.abs(g[:-1]) * np.sqrt(diag[p0[:-1]]) / (g[-1].real * np.sqrt(diag[i]))
        sure = np.abs(r / drop - 1.0) > 1e-12
        assert np.array_equal(np.isin(p0[:-1], p)[sure], (r >= drop)[sure]), i
        judged += int(sure.sum())
        check_row(G, i, p, D[np.ix_(p, p)], np.float64)
    assert judged >= (G0.nnz - n) - n // 100
    assert 0 < f['removed'] < G0.nnz - n


def with_plan(work='native'):
    from raleigh_amd.algebra.hip import Vectors
    from raleigh_amd.algebra.hip.precond import ApproximateInverse
    A = matrix('banded-d')
    n, m = A.shape[0], 9
    want, f = built(A, 0.02, 2, bits=64)
    T = ApproximateInverse(A, levels=2, prefilter=0.02, work=work)
    assert same_bits(T.csr(), want) and T.weak_entries == f['weak'] > 0
    g = wk.plan_info(T._plan)
    assert g['work'] == wk.WORKS[work]
    x = wk.random_block(np.random.default_rng(63), m, n, np.float64)
    y = Vectors(np.zeros((m, n)))
    T.apply(Vectors(x.copy()), y)
    wk.Reference(want, np.float64, work).check(x, y.data())


# ---------------------------------------------------------------- 9. the bins
def bins(code, monkeypatch):
    A = lv.banded(code)
    monkeypatch.setenv('RLH_FSAI_BINS', '0')
    two, f2 = built(A, 0.02, 2, bits=32)
    monkeypatch.delenv('RLH_FSAI_BINS')
    four, f4 = built(A, 0.02, 2, bits=32)
    assert same_bits(two, four) and f2 == dict(f4, seconds=f2['seconds'])
    lens = np.diff(four.indptr)
    if code == 'd':
        for lo, hi in lv.CLASSES[:4]:
            assert np.any((lens >= lo) & (lens <= hi)), (lo, hi)


# ---------------------------------------------------------------- 10. every loop past its first trip (GPU tier)
def hashed_band(n, w=4):
    """A band of w with values decided by a hash of the position: magnitude 1 (ratio 1 / 9 to the diagonal) or 0.01 (ratio
    0.0011), about half of each; the diagonal 9 dominates the at most 2 w entries of a row.  The hash is the 64-bit
    finaliser of MurmurHash3 on the entry's number (a multiplicative hash alone repeats with a short period in the row,
    and no row of the second level then grows past 7 members)."""
    rows, cols, vals = [], [], []
    for o in range(1, w + 1):
        r = np.arange(o, n, dtype=np.int64)
        hashed = (r * (w + 1) + o).astype(np.uint64)
        for shift, factor in ((33, 0xff51afd7ed558ccd), (33, 0xc4ceb9fe1a85ec53)):
            hashed = (hashed ^ (hashed >> np.uint64(shift))) * np.uint64(factor)       # wraps modulo 2^64
        hashed = (hashed ^ (hashed >> np.uint64(33))).astype(np.int64) >> 7
        big = (hashed & 1) == 1
        sign = np.where((hashed & 2) == 2, -1.0, 1.0)
        rows.append(r)
        cols.append(r - o)
        vals.append(sign * np.where(big, 1.0, 0.01))
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    low = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    A = sp.csr_matrix(low + low.T + sp.diags(np.full(n, 9.0)))
    A.sort_indices()
    return A


def loops(cu):
    tau, w = 0.05, 4
    per_pass, per_pattern_pass = cu * BLOCKS_PER_CU * STRONG_ROWS_PER_BLOCK, cu * BLOCKS_PER_CU * PATTERN_ROWS_PER_BLOCK
    n = per_pass + 300
    A = hashed_band(n, w)
    o = oracle(A, tau, 2)
    print('n = %d: %.1f %% strong, %d entries, longest row %d' % (n, 100 * o.strong_share, o.nnz, o.longest))
    # the second level reaches past the band (a first-level row has at most w + 1 members) and stays uncut
    assert 0.4 < o.strong_share < 0.6 and o.left_out == 0 and o.truncated == 0 and w + 1 < o.longest <= 2 * w + 1
    G, f = built(A, tau, 2, bits=32)
    compare_pattern(G, f, o, 'loops')
    rows = {0, 1, w, n - 1}
    for edge in list(range(per_pattern_pass, n, per_pattern_pass)) + [per_pass]:
        rows.update((edge - 1, edge, edge + 1))
    F = hermitian_from_upper(A).tocsr()
    for i in sorted(r for r in rows if 0 <= r < n):
        p = o.row(i)
        check_row(G, i, p, F[p][:, p].toarray().astype(np.longdouble), np.float64)


# ---------------------------------------------------------------- 11. new values keep the pattern
def update_values():
    A = matrix('profile-d')
    n, tau, levels = A.shape[0], 0.02, 2
    B = vl.revalued(A, 64)
    oa, ob = oracle(A, tau, levels), oracle(B, tau, levels)
    assert ob.left_out == 0 and (ob.weak != oa.weak or not np.array_equal(ob.indices, oa.indices))      # another strong set
    want, _ = built(A, tau, levels)
    rc, h = create(A, tau, levels)
    _check(rc)
    try:
        _check(vl.update(h, A))
        assert same_bits(get(h, A.dtype.type), want) and vl.values_info(h)[0] == 1
        _check(vl.update(h, B, host=True))
        G = get(h, A.dtype.type)
        assert threshold_of(h) == (tau, oa.weak) and vl.values_info(h)[0] == 2      # (the rule is not applied again)
    finally:
        destroy(h)
    assert np.array_equal(G.indptr, want.indptr) and np.array_equal(G.indices, want.indices)
    vl.check_all(G, want, wide_dense(B), np.float64)


# ---------------------------------------------------------------- 12. the class
def class_inputs(device):
    from raleigh_amd.algebra.hip.precond import ApproximateInverse
    A = lv.banded('d')
    want, f = built(A, 0.02, 2, bits=64)
    kw = dict(levels=2, prefilter=0.02)
    made = [ApproximateInverse(A, **kw), ApproximateInverse(csr_tensor(A, device, np.int32), **kw),
            ApproximateInverse(csr_tensor(A, device, np.int64), **kw), ApproximateInverse(csr_tensor(A, 'cpu'), **kw)]
    for T in made:
        assert (T.levels, T.steps, T.drop, T.prefilter) == (2, 0, 0.0, 0.02) and same_bits(T.csr(), want)
        assert threshold_of(T._h) == (0.02, f['weak']) and T.weak_entries == f['weak'] > 0 and T.dropped_entries == 0
        assert T.truncated_rows == f['truncated'] and T.longest_row == f['longest'] and T.nnz == want.nnz
        assert abs(T.fill - want.nnz / A.nnz) < 1e-15
    T = ApproximateInverse(A, levels=2, steps=1, step_size=2, drop=0.03, prefilter=0.02, max_row=40)
    wanted, g = built(A, 0.02, 2, 1, 2, 0.03, max_row=40)
    assert same_bits(T.csr(), wanted) and (T.weak_entries, T.dropped_entries) == (g['weak'], g['removed']) and g['removed'] > 0
    return made


def unchanged_without_prefilter(code, device):
    from raleigh_amd.algebra.hip.precond import ApproximateInverse
    A = base.matrix(code)
    for kw, raw in (({}, lambda: base.built(A, bits=32)), ({'levels': 2}, lambda: base.built(A, '_levels', 2, bits=32)),
                    ({'steps': 2}, lambda: base.built(A, '_adaptive', 1, 2, 1, bits=32)),
                    ({'levels': 2, 'drop': 0.03}, lambda: fl.built_filtered(A, 2, drop=0.03, bits=32))):
        want, f = raw()
        for T in (ApproximateInverse(A, **kw), ApproximateInverse(A, prefilter=0.0, **kw), ApproximateInverse(A, prefilter=0, **kw),
                  ApproximateInverse(csr_tensor(A, device), prefilter=0.0, **kw)):
            assert same_bits(T.csr(), want) and T.prefilter == 0.0 and T.weak_entries == 0 and T.nnz == f['nnz']
            assert threshold_of(T._h) == (0.0, 0)


# ---------------------------------------------------------------- 13. rejections
def rejections_raw():
    A = base.matrix('d')
    for host, name in ((False, 'rlh_fsthreshold_create_device'), (True, 'rlh_fsthreshold_create')):
        def refused(text, M=A, **kw):
            kw.setdefault('prefilter', 0.02)
            rc, h = create(M, host=host, **kw)
            assert rc != 0 and not h.value, (name, text)
            assert last_error().endswith('%s: %s' % (name, text)), (text, last_error())
        for tau, shown in ((0.0, '0'), (-0.1, '-0.1'), (1.0, '1'), (2.5, '2.5'), (float('inf'), 'inf'), (float('nan'), 'nan')):
            refused('prefilter must lie in (0, 1), got ' + shown, prefilter=tau)
        refused('max_row must lie in [1, 64], got 65', max_row=65, prefilter=2.0)
        refused('levels must lie in [1, 8], got 9', levels=9)
        refused('steps must lie in [1, 63], got 64', steps=64)
        refused('step_size must lie in [1, 16], got 17', steps=1, step_size=17)
        refused('drop must lie in (0, 1), got 1', drop=1.0, prefilter=2.0)
        refused('drop must lie in (0, 1), got nan', drop=float('nan'))
        refused('null indptr', null=(0,))
        if host:
            refused('null indices or values', null=(1,))
            refused('null indices or values', null=(2,))
        else:
            refused('index_bits must be 32 or 64, got 16', bits=16)
        # a missing diagonal wins over a missing partner, whichever row comes first
        j1 = int(A.indices[A.indptr[203]])
        assert j1 < 203
        B = base._without(A, j1, 203)
        refused('the stored structure is not symmetric: entry (203, %d) has no partner (%d, 203); the device build creates no entries'
                % (j1, j1), B)
        refused('row 300 does not store its diagonal entry', base._without(B, 300, 300))
        C = A.copy().tolil()
        C[350, 350] = -3.0
        C = sp.csr_matrix(C)
        C.sort_indices()
        refused('local block of row 350 is not positive definite', C)
        rc, h = create(A, 0.5, 1, 0, 99, 0.0, host=host)          # steps == 0: step_size is not looked at; drop == 0: none
        _check(rc)
        assert base.adaptive_of(h) == (0, 0) and fl.filtered_of(h) == (0.0, 0) and threshold_of(h)[0] == 0.5
        destroy(h)
    from raleigh_amd import _lib
    L = _L()
    ip, ix, va = A.indptr.astype(np.int64), A.indices.astype(np.int32), np.ascontiguousarray(A.data)
    rc = L.rlh_fsthreshold_create(None, _lib.DTYPE_CODE[A.dtype.type], A.shape[0], _lib.host_ptr(ip), _lib.host_ptr(ix), _lib.host_ptr(va),
                                  64, 1, 0, 1, 0.0, 0.02)
    assert rc != 0 and last_error().endswith('rlh_fsthreshold_create: null handle pointer'), last_error()
    rc, h = base.create(A)                                       # a handle of another entry point answers (0, 0)
    _check(rc)
    assert threshold_of(h) == (0.0, 0)
    destroy(h)
    assert L.rlh_fsthreshold_info(None, None, None) != 0 and 'rlh_fsthreshold_info: null handle or output' in last_error()


def rejections_class(fake=None):
    from raleigh_amd.algebra.hip.precond import ApproximateInverse
    A = base.matrix('d')
    before = dict(fake.calls) if fake is not None else None
    for tau, shown in ((1.0, '1'), (-0.1, r'-0\.1'), (2.5, r'2\.5'), (float('inf'), 'inf'), (float('nan'), 'nan')):
        with pytest.raises(ValueError, match=r'prefilter must lie in \[0, 1\), got %s' % shown):
            ApproximateInverse(A, prefilter=tau)
    with pytest.raises(ValueError, match='max_row'):
        ApproximateInverse(A, max_row=65, prefilter=0.1)
    with pytest.raises(ValueError, match='drop must lie'):
        ApproximateInverse(A, drop=1.0, prefilter=0.1)
    with pytest.raises(ValueError, match='work must be'):
        ApproximateInverse(A, prefilter=0.1, work='float16')
    if fake is not None:
        assert dict(fake.calls) == before                   # refused before any library call


# ---------------------------------------------------------------- 14. device memory
def device_memory():
    A = lv.banded('d')
    first = live()
    for host in (True, False):
        rc, h = create(A, 0.02, 2, 2, 2, 0.03, host=host)
        _check(rc)
        assert live()[0] >= first[0]
        destroy(h)
        assert live() == first
        bad = A.copy().tolil()
        bad[350, 350] = -3.0
        bad = sp.csr_matrix(bad)
        bad.sort_indices()
        for M, kw, text in ((bad, {}, 'local block of row 350 is not positive definite'),
                            (base._without(A, 300, 300), {}, 'row 300 does not store its diagonal entry'),
                            (base._without(A, int(A.indices[A.indptr[203]]), 203), {}, 'has no partner'),
                            (A, {'prefilter': 1.5}, 'prefilter must lie in (0, 1), got 1.5')):
            kw.setdefault('prefilter', 0.02)
            rc, h = create(M, levels=2, host=host, **kw)
            assert rc != 0 and not h.value and text in last_error(), (text, last_error())
            assert live() == first, text


# ---------------------------------------------------------------- 15. end to end
def end_to_end(device):
    """The solver tolerance is that of `lv.end_to_end` (1e-6).  Its bound on the eigenvalues, 1e-10, is absolute on an operator
    of norm at most 4 (cx + cy + cz) = 1706 (Gershgorin, the coefficients of lap3d_rows(12, 11, 10, 1, 1.01, 1.02)); the
    operator here has 4 (121 + 12100 + 1210000) = 4.889e6, where 1e-10 is below one rounding u ||A|| = 5.4e-10 of the dense
    reference.  The bound is carried over relative to that norm: 1e-10 * 4.889e6 / 1706 = 2.87e-7 (about the n u ||A|| =
    5.4e-7 the reference is good for).  The four smallest eigenvalues lie within 3e-4 of each other relative to the norm;
    the solver's stagnation test locks such pairs early whatever the preconditioner, so it is switched off, and the
    iteration limit is raised for the run without a preconditioner."""
    import scipy.linalg
    import torch
    from raleigh_amd.interfaces import partial_hevp
    from raleigh_amd.algebra.hip.precond import ApproximateInverse
    from raleigh_amd.core.solver import Options
    from raleigh_amd.synthetic import lap3d_coefficients, lap3d_rows
    A = sp.csr_matrix(lap3d_rows(10, 10, 10, 1.0, 0.1, 0.01, 0, 1000)).astype(np.float64)
    A.sort_indices()
    which = 4
    bound = 1e-10 * sum(lap3d_coefficients(10, 10, 10, 1.0, 0.1, 0.01)) / sum(lap3d_coefficients(12, 11, 10, 1.0, 1.01, 1.02))
    exact = scipy.linalg.eigvalsh(hermitian_from_upper(A).toarray())[:which]
    a = csr_tensor(A, device)
    its, nnz = {}, {}
    for name, make in (('prefilter=0.1', lambda: ApproximateInverse(a, levels=3, prefilter=0.1)),
                       ('prefilter=0', lambda: ApproximateInverse(a, levels=3)), ('T=True', lambda: True)):
        T = make()
        nnz[name] = T.nnz if T is not True else 0
        np.random.seed(1)
        opt = Options()
        opt.max_iter, opt.detect_stagnation = 3000, False
        lmd, x, status = partial_hevp(a, T=T, which=which, tol=1e-6, verb=-1, opt=opt)
        its[name] = partial_hevp.last['iterations']
        assert status == 0, name
        print('%s: largest eigenvalue error %.3g (bound %.3g)' % (name, float(np.max(np.abs(lmd[:which] - exact))), bound))
        if name == 'prefilter=0.1':
            assert T.weak_entries > 0 and T.prefilter == 0.1
            assert np.max(np.abs(lmd[:which] - exact)) <= bound
            assert isinstance(x, torch.Tensor) and x.device.type == torch.device(device).type
    print('level 3: %d iterations on %d entries with prefilter=0.1, %d on %d entries with prefilter=0, %d with T=True'
          % (its['prefilter=0.1'], nnz['prefilter=0.1'], its['prefilter=0'], nnz['prefilter=0'], its['T=True']))
    assert its['prefilter=0.1'] < its['T=True'] and nnz['prefilter=0.1'] < nnz['prefilter=0']
    return its, nnz


# ---------------------------------------------------------------- 16. row shards
def sharded(A, comm, off, tau=0.02):
    """At levels = 1, steps = 0 every rank's rows are those of the single build bit for bit (A[E, E] holds every a_ji, a_ii
    and a_jj the rule reads), without and with drop; with drop the rank's count of dropped entries is the single build's
    over its rows."""
    import _fsai_shard_cases as sh
    from raleigh_amd.algebra.hip.precond import ApproximateInverse
    r0, r1 = int(off[comm.rank]), int(off[comm.rank + 1])
    plain = ApproximateInverse(A, prefilter=tau)
    assert 0 < plain.weak_entries < np.sum(base.lower_lengths(A) - 1)
    before = sp.csr_matrix(plain.csr()[r0:r1, :])
    for drop in (0.0, 0.03):
        whole = ApproximateInverse(A, prefilter=tau, drop=drop)
        want = sp.csr_matrix(whole.csr()[r0:r1, :])
        assert whole.weak_entries == plain.weak_entries and (whole.dropped_entries > 0) == (drop > 0)
        for T in sh.both_constructors(A, comm, off, prefilter=tau, drop=drop):
            got = T.csr()
            assert got.shape == (r1 - r0, A.shape[0]) and got.dtype == A.dtype and T.prefilter == tau
            assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
            assert np.array_equal(sh.bits(got.data), sh.bits(want.data))
            assert T.nnz == whole.nnz and T.longest_row == whole.longest_row and abs(T.fill - whole.fill) < 1e-15
            assert T.dropped_entries == int(before.nnz - want.nnz)
    assert int(before.nnz - want.nnz) > 0 or r1 - r0 < 50
