"""New matrix values on the pattern an approximate inverse already has (rlh_fsvalues_update*, rlh_fsvalues_plan,
rlh_fsvalues_info, ApproximateInverse.update_values): cases shared by the CPU tier (tests/fake_fsai.py) and the
GPU tier.  Matrices, helpers and the bound of the defining property (`check_row`) come from tests/_fsai_cases.py (`base`),
the configurations and the longdouble operator (`wide_dense`) from tests/_fsai_filter_cases.py (`fl`).

`revalued(A, seed)` multiplies every stored off-diagonal entry of the upper triangle by a real factor uniform in [0.5, 1)
and every diagonal entry by one in [1, 2), and mirrors the lower triangle: the structure is unchanged.  The test matrices
have a positive diagonal at least the sum of the moduli of the off-diagonal entries of the row (plus 1 for the profile and
band matrices; the Laplacian is dominant with strict rows at the boundary), so after `revalued` every row with an
off-diagonal entry is STRICTLY dominant: the matrix and every local block are positive definite, which needs no GPU to
see.  Removing an off-diagonal pair, or scaling by D A D, keeps that.

WHAT IS COMPARED EXACTLY.  Where the pattern came from levels alone and the structure of the matrix is unchanged, the
updated handle must be the fresh build of the new matrix bit for bit (G, and the application through G^H).  Where the
pattern was chosen by value (steps, drop) a fresh build may choose another pattern: there the kept pattern must be
unchanged, every row must have the defining property (`check_row`: a bound from the arithmetic, tests/_fsai_cases.py) on
the new matrix, and the application must stay within the bound of `base.application` computed from the fetched G, which
a stale G^H would miss by a factor of the order 1 / unit roundoff.

LAUNCH GEOMETRY the loop case relies on: the update's own kernels (the diagonal check with the keys of the bins, the
rows of the bins, the conjugated values of G^H, and the row check of rlh_fsvalues_plan) take one thread per row -- or per
entry of G^H -- in workgroups of 256 threads, at most 8 workgroups per CU, in grid-stride loops: one pass covers
CU * 8 * 256 rows (entries).  The 64-lane set-up takes one row per workgroup on at most 8 workgroups per CU
(tests/_fsai_cases.py).
"""

import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import _fsai_cases as base
import _fsai_levels_cases as lv
import _fsai_filter_cases as fl
import _fsai_work_cases as wk
from _fsai_cases import TYPES, VECTORS, _L, _check, _without, check_row, csr_tensor, destroy, get, hermitian_from_upper, info, \
    last_error, padded_with, same_bits, unit
from _fsai_filter_cases import ADAPTIVE, LEVEL_1, LEVEL_2, SHORT_ROWS, matrix, wide_dense

BLOCKS_PER_CU = 8
ROWS_PER_BLOCK = 256            # the update's own kernels: one thread per row (per entry of G^H)
CONFIGS = (LEVEL_1, LEVEL_2, ADAPTIVE, SHORT_ROWS)
DROPS = (0, 0.1)
LEVELS_ONLY = [(which, config) for which in ('profile-d', 'cut-d', 'lap') for config in (LEVEL_1, LEVEL_2, SHORT_ROWS)] \
    + [(which, LEVEL_1) for which in ('profile-s', 'profile-c', 'profile-z')] + [('profile-z', LEVEL_2)]
BY_VALUE = [('profile-d', ADAPTIVE, 0), ('banded-d', ADAPTIVE, 0), ('lap', ADAPTIVE, 0), ('profile-z', LEVEL_1, 0.1)] \
    + [(which, config, 0.1) for which in ('profile-d', 'banded-d') for config in CONFIGS]


def revalued(A, seed):
    n = A.shape[0]
    rng = np.random.default_rng(seed)
    u = sp.triu(A, format='coo')
    factor = np.where(u.row == u.col, rng.uniform(1.0, 2.0, u.nnz), rng.uniform(0.5, 1.0, u.nnz)).astype(A.real.dtype)
    up = sp.csr_matrix((u.data * factor, (u.row, u.col)), shape=(n, n))
    B = sp.csr_matrix(up + sp.triu(up, k=1).conj().T).astype(A.dtype)
    B.sort_indices()
    assert np.array_equal(B.indptr, A.indptr) and np.array_equal(B.indices, A.indices)
    return B


# ---------------------------------------------------------------- the raw entry points
def create(A, config, drop=0, **kw):
    """(rc, handle) of the create call a configuration (levels, steps, step_size, max_row) and a drop go through."""
    levels, steps, step_size, max_row = config
    if drop:
        return fl.create_filtered(A, levels, steps, step_size, drop, max_row=max_row, **kw)
    if steps:
        return base.create(A, '_adaptive', levels, steps, step_size, max_row=max_row, **kw)
    return base.create(A, '_levels', levels, max_row=max_row, **kw) if levels > 1 else base.create(A, max_row=max_row, **kw)


def made(A, config, drop=0, **kw):
    rc, h = create(A, config, drop, **kw)
    _check(rc)
    return h


def fresh(A, config, drop=0, **kw):
    """G of a build that must succeed."""
    h = made(A, config, drop, **kw)
    try:
        return get(h, A.dtype.type)
    finally:
        destroy(h)


def update(h, A, host=False, bits=64, indptr=None, indices=None, null=()):
    """rc of rlh_fsvalues_update on A's arrays (host=True) or of rlh_fsvalues_update_device on device copies of them (or of
    the given indptr / indices); null: positions among the three arrays passed as null pointers."""
    from raleigh_amd import _lib
    it = {32: np.int32, 64: np.int64}.get(bits, np.int64)
    arrays = ((A.indptr if indptr is None else indptr).astype(np.int64 if host else it),
              (A.indices if indices is None else indices).astype(np.int32 if host else it), np.ascontiguousarray(A.data))
    if host:
        ptrs = [None if k in null else _lib.host_ptr(a) for k, a in enumerate(arrays)]
        return _L().rlh_fsvalues_update(h, *ptrs)
    bufs = [base.dev(a) for a in arrays]
    ptrs = [None if k in null else b.ptr for k, b in enumerate(bufs)]
    return _L().rlh_fsvalues_update_device(h, bits, *ptrs)


def values_info(h):
    updates, sec = ctypes.c_int64(-1), ctypes.c_double(-1.0)
    _check(_L().rlh_fsvalues_info(h, ctypes.byref(updates), ctypes.byref(sec)))
    return updates.value, sec.value


def live():
    nbytes, nblocks = ctypes.c_int64(-1), ctypes.c_int64(-1)
    _check(_L().rlh_device_live(ctypes.byref(nbytes), ctypes.byref(nblocks)))
    return nbytes.value, nblocks.value


def applied(h, dt, n, G=None, run=None):
    """The bits of rlh_fsai_apply (or of run(m, X, ld, Y, ldy)) on the blocks of `base.application`: VECTORS vectors, padding
    rows and guard columns NaN and untouched.  G: the fetched G; with it the result must lie within the bound of
    `base.application`."""
    dt = np.dtype(dt)
    rng = np.random.default_rng(21)
    ld, guard = n + 5, 2
    if run is None:
        def run(m, X, ldx, Y, ldy):
            return _L().rlh_fsai_apply(h, m, X, ldx, Y, ldy)
    if G is not None:
        wide = np.clongdouble if dt.kind == 'c' else np.longdouble
        Gd = G.toarray().astype(wide)
        Ga = np.abs(G.toarray()).astype(np.float64)
        a, b = int(np.diff(G.indptr).max()), int(np.diff(G.tocsc().indptr).max())
    out = []
    for m in VECTORS:
        x = rng.standard_normal((m + guard, ld))
        if dt.kind == 'c':
            x = x + 1j * rng.standard_normal((m + guard, ld))
        x = x.astype(dt)
        x[:, n:] = np.nan
        x[m:, :] = np.nan
        y0 = np.full((m + guard, ld + 3), np.nan, dtype=dt)
        X, Y = base.dev(x), base.dev(y0)
        _check(run(m, X.ptr, ld, Y.ptr, ld + 3))
        y = base.fetch(Y, y0.size, dt).reshape(y0.shape)
        assert np.all(np.isnan(y[:, n:])) and np.all(np.isnan(y[m:, :]))
        assert np.all(np.isfinite(y[:m, :n].astype(np.complex128)))
        if G is not None:
            exact = (np.conj(Gd.T) @ (Gd @ x[:m, :n].astype(wide).T)).T
            bound = (a + b + 2) * unit(dt) * (Ga.T @ (Ga @ np.abs(x[:m, :n]).astype(np.float64).T)).T
            err = np.abs(y[:m, :n].astype(wide) - exact).astype(np.float64)
            assert np.all(err <= bound), (m, float(np.max(err / bound)))
        out.append(np.ascontiguousarray(y).view(np.uint8).copy())
    return out


def same_blocks(a, b):
    return len(a) == len(b) and all(np.array_equal(p, q) for p, q in zip(a, b))


def check_all(G, pattern, D, dt):
    """Every row of G has the columns of `pattern` and the defining property on the longdouble operator D."""
    worst = 0.0
    for i in range(G.shape[0]):
        p = fl.row_of(pattern, i)
        worst = max(worst, check_row(G, i, p, D[np.ix_(p, p)], dt))
    print('largest residual / bound: %.3g' % worst)


# ---------------------------------------------------------------- 1. the same matrix
def same_matrix(which, config, drop, host=False, bits=64):
    A = matrix(which)
    h = made(A, config, drop, bits=32)
    try:
        G0, f0 = get(h, A.dtype.type), info(h)
        assert values_info(h) == (0, 0.0)
        for k in (1, 2):
            _check(update(h, A, host=host, bits=bits))
            assert same_bits(get(h, A.dtype.type), G0)
            got = values_info(h)
            assert got[0] == k and got[1] >= 0.0
        assert info(h) == f0
        levels, steps, step_size, _ = config
        assert base.levels_of(h) == levels and base.adaptive_of(h) == ((steps, step_size) if steps else (0, 0))
        assert fl.filtered_of(h)[0] == float(drop)
    finally:
        destroy(h)


# ---------------------------------------------------------------- 2. new values, pattern from levels alone
def levels_only(which, config, host=False):
    A = matrix(which)
    B = revalued(A, 61)
    dt, n = A.dtype.type, A.shape[0]
    h, hb = made(A, config, bits=32), made(B, config, bits=32)
    try:
        G0, Gb, f0 = get(h, dt), get(hb, dt), info(h)
        assert not same_bits(G0, Gb)
        _check(update(h, B, host=host, bits=32))
        assert same_bits(get(h, dt), Gb) and info(h) == f0
        assert same_blocks(applied(h, dt, n), applied(hb, dt, n))
    finally:
        destroy(h)
        destroy(hb)


# ---------------------------------------------------------------- 3. new values, pattern chosen by value
def by_value(which, config, drop):
    A = matrix(which)
    B = revalued(A, 62)
    dt, n = A.dtype.type, A.shape[0]
    h = made(A, config, drop, bits=32)
    try:
        G0, f0 = get(h, dt), info(h)
        kept = fl.filtered_of(h)
        _check(update(h, B))
        G = get(h, dt)
        assert np.array_equal(G.indptr, G0.indptr) and np.array_equal(G.indices, G0.indices) and not same_bits(G, G0)
        check_all(G, G0, wide_dense(B), dt)
        applied(h, dt, n, G=G)
        f = info(h)
        assert (f['nnz'], f['longest'], f['truncated'], f['seconds']) == (f0['nnz'], f0['longest'], f0['truncated'], f0['seconds'])
        assert fl.filtered_of(h) == kept and values_info(h)[0] == 1
    finally:
        destroy(h)


# ---------------------------------------------------------------- 4. scaling by powers of two
def scaling(which, config, drop, exact=True):
    """A' = D A D with the D of `fl.scaling`.  exact: the update is the fresh build of A' bit for bit (every operation of
    the build commutes with a scaling by powers of two, so the fresh build chooses the same pattern).  The stand-in solves
    by LAPACK's pivoted LU, whose pivots a scaling moves: there every row has the defining property on A' on its kept
    pattern."""
    A = matrix(which)
    n, dt = A.shape[0], A.dtype.type
    rng = np.random.default_rng(51)
    d = 2.0 ** rng.integers(-20, 21, n)
    B = sp.csr_matrix(sp.diags(d) @ A.astype(np.complex128 if A.dtype.kind == 'c' else np.float64) @ sp.diags(d)).astype(A.dtype)
    B.sort_indices()
    assert np.array_equal(B.indptr, A.indptr) and np.array_equal(B.indices, A.indices)
    h = made(A, config, drop, bits=32)
    try:
        G0 = get(h, dt)
        _check(update(h, B, bits=32))
        G = get(h, dt)
    finally:
        destroy(h)
    assert np.array_equal(G.indptr, G0.indptr) and np.array_equal(G.indices, G0.indices)
    if exact:
        assert same_bits(G, fresh(B, config, drop, bits=32))
        want = sp.csr_matrix((G0.data / d[G0.indices].astype(G0.real.dtype), G0.indices, G0.indptr), shape=G0.shape)
        assert same_bits(G, want)
        return
    check_all(G, G0, wide_dense(B), dt)


# ---------------------------------------------------------------- 5. another structure
def padded(code):
    """Explicit zeros change nothing: the padded A' gives the bits of A'."""
    A = base.matrix(code)
    B = revalued(A, 63)
    n = A.shape[0]
    rng = np.random.default_rng(64)
    rows, cols = rng.integers(0, n, 400), rng.integers(0, n, 400)
    P = padded_with(B, rows, cols)
    assert P.nnz > B.nnz
    h = made(A, LEVEL_1, bits=32)
    try:
        for host in (False, True):
            _check(update(h, A, host=host))
            _check(update(h, P, host=host, bits=32))
            assert same_bits(get(h, A.dtype.type), fresh(B, LEVEL_1))
    finally:
        destroy(h)


def entry_removed():
    """A' without one stored entry above the diagonal (its mirror image stays: nothing below the diagonal is read and no
    partner is asked for): that position of every local block is zero."""
    A = base.matrix('d')
    B = revalued(A, 65)
    i = 404
    lower = A.indices[A.indptr[i]:A.indptr[i + 1]]
    j = int(lower[lower < i][-1])
    C = _without(B, j, i)
    D = wide_dense(B).copy()
    assert D[j, i] != 0
    D[j, i] = D[i, j] = 0
    for config in (LEVEL_1, LEVEL_2):
        h = made(A, config, bits=32)
        try:
            G0 = get(h, np.float64)
            holders = [r for r in range(A.shape[0]) if np.all(np.isin((j, i), fl.row_of(G0, r)))]
            assert holders and holders[0] == i
            _check(update(h, C))
            G = get(h, np.float64)
            check_all(G, G0, D, np.float64)
            full = fresh(B, config)
            for r in holders:
                assert not np.array_equal(G.data[G.indptr[r]:G.indptr[r + 1]], full.data[full.indptr[r]:full.indptr[r + 1]]), r
        finally:
            destroy(h)


# ---------------------------------------------------------------- 6. plans
def plans(work):
    A = base.matrix('d')
    B = revalued(A, 66)
    n, dt = A.shape[0], np.float64
    L = _L()
    h = made(A, LEVEL_2, bits=32)
    rc, p = wk.plan_create(h, wk.WORKS[work])
    _check(rc)
    others = []
    try:
        f0, bytes0 = wk.plan_info(p), info(h)['bytes']

        def through(plan):
            return applied(None, dt, n, run=lambda m, X, ldx, Y, ldy: wk.run(plan, m, X, ldx, Y, ldy))
        old = through(p)
        grown = wk.plan_info(p)['bytes']
        _check(update(h, B))
        assert same_blocks(through(p), old)                         # a plan that is not refilled keeps its values
        _check(L.rlh_fsvalues_plan(p, h))
        rc, q = wk.plan_create(h, wk.WORKS[work])
        _check(rc)
        others.append((wk.plan_destroy, q))
        new = through(p)
        assert same_blocks(new, through(q)) and not same_blocks(new, old)
        f = wk.plan_info(p)
        assert (f['work'], f['slots'], f['tail']) == (f0['work'], f0['slots'], f0['tail']) and f['bytes'] == grown
        assert info(h)['bytes'] == bytes0
        # mismatched plan and handle
        for text, C, config in (('rlh_fsvalues_plan: the plan has %d rows, the handle %d' % (n, lv.lap('d').shape[0]), lv.lap('d'), LEVEL_1),
                                ("rlh_fsvalues_plan: the plan's dtype", base.matrix('s'), LEVEL_2),
                                ('rlh_fsvalues_plan: the plan holds', A, SHORT_ROWS)):
            g = made(C, config)
            others.append((destroy, g))
            assert L.rlh_fsvalues_plan(p, g) != 0 and text in last_error(), last_error()
        assert L.rlh_fsvalues_plan(None, h) != 0 and 'rlh_fsvalues_plan: null plan' in last_error()
        assert L.rlh_fsvalues_plan(p, None) != 0 and 'rlh_fsvalues_plan: null handle' in last_error()
        assert same_blocks(through(p), new)                         # a refused refill leaves the plan as it was
    finally:
        for release, obj in others:
            release(obj)
        wk.plan_destroy(p)
        destroy(h)


# ---------------------------------------------------------------- 7. refusals leave the handle as it was
def refusals(host):
    """The array mutations of `base.rejections_raw` and what else the entry points refuse, each with a message naming the
    entry point and the smallest row; afterwards the handle has the bits it had, and a good update works."""
    name = 'rlh_fsvalues_update' if host else 'rlh_fsvalues_update_device'
    A = base.matrix('d')
    N, dt = A.shape[0], np.float64
    B = revalued(A, 67)
    ip, ix = B.indptr.astype(np.int64), B.indices.astype(np.int64)
    h = made(A, LEVEL_1, bits=32)
    try:
        G0, before, f0, first = get(h, dt), applied(h, dt, N), info(h), live()

        def refused(text, M=B, **kw):
            rc = update(h, M, host=host, **kw)
            assert rc != 0, text
            assert '%s: %s' % (name, text) in last_error(), (text, last_error())
            assert same_bits(get(h, dt), G0) and live() == first and values_info(h) == (0, 0.0)
        row = 100
        k = int(ip[row]) + 1
        assert ip[row + 1] - ip[row] >= 3

        def changed(a, i, v):
            b = a.copy()
            b[i] = v
            return b
        swapped = ix.copy()
        swapped[k], swapped[k + 1] = ix[k + 1], ix[k]
        refused('indptr[0] must be 0', indptr=changed(ip, 0, 1))
        refused('indptr decreases at row 49', indptr=changed(ip, 50, ip[49] - 1))
        refused('column index out of range in row %d' % row, indices=changed(ix, k, N))
        refused('the columns of row %d must ascend strictly (no duplicates)' % row, indices=swapped)
        refused('row 300 does not store its diagonal entry', M=_without(_without(B, 500, 500), 300, 300))
        C = B.copy().tolil()
        C[350, 350] = -3.0
        C[600, 600] = -1.0
        C = sp.csr_matrix(C)
        C.sort_indices()
        refused('local block of row 350 is not positive definite', M=C)
        refused('null indptr', null=(0,))
        if host:
            refused('null indices or values', null=(1,))
            refused('null indices or values', null=(2,))
        else:
            refused('index_bits must be 32 or 64, got 16', bits=16)
            for null in ((1,), (2,)):
                refused("indptr's last entry (%d) is not the number of stored entries (the index and value arrays hold at most 0)"
                        % B.nnz, null=null)
        assert update(None, B, host=host) != 0 and '%s: null handle' % name in last_error()
        assert _L().rlh_fsvalues_info(None, None, None) != 0 and 'rlh_fsvalues_info: null handle' in last_error()
        assert same_blocks(applied(h, dt, N), before) and info(h) == f0
        _check(update(h, B, host=host))
        assert same_bits(get(h, dt), fresh(B, LEVEL_1)) and values_info(h)[0] == 1 and live() == first
    finally:
        destroy(h)


# ---------------------------------------------------------------- 8. every loop of the update past its first trip
def loops_short(n, work=None):
    """A band of 3 (rows of 4 entries, the 8-lane bin) of n rows: on the GPU tier n is one more than a whole grid pass of
    the update's own kernels, and G^H has more entries than a pass of its kernel."""
    A = lv.band(np.full(n, 3), np.float64, 71)
    B = revalued(A, 72)
    h = made(A, LEVEL_1, bits=32)
    try:
        _check(update(h, B, bits=32))
        G = get(h, np.float64)
        assert info(h)['longest'] == 4 and G.nnz == 4 * n - 6 > n
        Gb = fresh(B, LEVEL_1, bits=32)
        assert same_bits(G, Gb)
        # G^H through the application: one vector, against the fetched G
        x = np.random.default_rng(73).standard_normal(n)
        X, Y = base.dev(x), base.dev(np.zeros(n))
        _check(_L().rlh_fsai_apply(h, 1, X.ptr, n, Y.ptr, n))
        y, want = base.fetch(Y, n, np.float64), G.T @ (G @ x)
        assert np.all(np.abs(y - want) <= 10 * unit(np.float64) * (abs(G).T @ (abs(G) @ np.abs(x))))
        if work is not None:
            rc, p = wk.plan_create(h, wk.WORKS[work])
            _check(rc)
            try:
                _check(update(h, A, bits=32))
                _check(_L().rlh_fsvalues_plan(p, h))
                _check(update(h, B, bits=32))
                _check(_L().rlh_fsvalues_plan(p, h))
                Y2 = base.dev(np.zeros(n))
                _check(wk.run(p, 1, X.ptr, n, Y2.ptr, n))
                y2 = base.fetch(Y2, n, np.float64)
                assert np.all(np.abs(y2 - want) <= 10 * unit(np.float64) * (abs(G).T @ (abs(G) @ np.abs(x))))
            finally:
                wk.plan_destroy(p)
    finally:
        destroy(h)


def loops_long(n):
    """A band of 40 (rows of 41 entries, the 64-lane bin) of n rows: on the GPU tier one more than a pass of its set-up."""
    A = lv.band(np.full(n, 40), np.float64, 74)
    B = revalued(A, 75)
    h = made(A, LEVEL_1)
    try:
        _check(update(h, B))
        assert info(h)['longest'] == 41
        assert same_bits(get(h, np.float64), fresh(B, LEVEL_1))
    finally:
        destroy(h)


# ---------------------------------------------------------------- 9. the bins
def bins(code, monkeypatch):
    A = lv.banded(code)
    B = revalued(A, 76)
    dt = A.dtype.type
    h = made(A, LEVEL_2, bits=32)
    try:
        lens = np.diff(get(h, dt).indptr)
        for lo, hi in lv.CLASSES[:4]:
            assert np.any((lens >= lo) & (lens <= hi)), (lo, hi)
        _check(update(h, B))
        four = get(h, dt)
        _check(update(h, A))
        monkeypatch.setenv('RLH_FSAI_BINS', '0')
        _check(update(h, B))
        monkeypatch.delenv('RLH_FSAI_BINS')
        two = get(h, dt)
        assert same_bits(two, four) and same_bits(four, fresh(B, LEVEL_2))
    finally:
        destroy(h)


# ---------------------------------------------------------------- 10. device memory
def device_memory(handle_bytes):
    """handle_bytes(n, nnz, element size): what a handle that has applied nothing holds, by the formula it always had."""
    A = lv.banded('d')
    B = revalued(A, 77)
    n = A.shape[0]
    first = live()
    for config, drop in ((LEVEL_2, 0), (ADAPTIVE, 0.1)):
        h = made(A, config, drop)
        rc, p = wk.plan_create(h, 0)
        _check(rc)
        try:
            f, held, plan_held = info(h), live(), wk.plan_info(p)['bytes']
            assert f['bytes'] == handle_bytes(n, f['nnz'], 8)
            for host in (False, True):
                _check(update(h, B, host=host))
                assert live() == held
                _check(_L().rlh_fsvalues_plan(p, h))
                assert live() == held
                assert update(h, _without(B, 5, 5), host=host) != 0
                assert 'row 5 does not store its diagonal entry' in last_error() and live() == held
            assert info(h)['bytes'] == f['bytes'] and wk.plan_info(p)['bytes'] == plan_held
        finally:
            wk.plan_destroy(p)
            destroy(h)
        assert live() == first


# ---------------------------------------------------------------- 11. the class
def class_inputs(device, fake=None):
    """fake: the stand-in, whose calls are counted (there every tensor counts as lying in device memory)."""
    from raleigh_amd.algebra.hip import Vectors
    from raleigh_amd.algebra.hip.precond import ApproximateInverse
    A = lv.banded('d')
    n = A.shape[0]
    news = [revalued(A, 80 + k) for k in range(4)]
    for work in (None, 'float32'):
        T = ApproximateInverse(csr_tensor(A, device), levels=2, work=work)
        assert (T.updates, T.update_seconds) == (0, 0.0)
        kept = (T.nnz, T.fill, T.longest_row, T.truncated_rows, T.dropped_entries, T.setup_seconds)
        before = dict(fake.calls) if fake is not None else None
        inputs = [news[0], csr_tensor(news[1], device, np.int32), csr_tensor(news[2], device, np.int64), csr_tensor(news[3], 'cpu')]
        for k, (B, given) in enumerate(zip(news, inputs)):
            T.update_values(given)
            assert T.updates == k + 1 and T.update_seconds >= 0.0
            want = ApproximateInverse(B, levels=2, work=work)
            assert same_bits(T.csr(), want.csr())
            x = np.random.default_rng(90).standard_normal((5, n))
            y, y0 = Vectors(np.zeros((5, n))), Vectors(np.zeros((5, n)))
            T.apply(Vectors(x.copy()), y)
            want.apply(Vectors(x.copy()), y0)
            assert np.array_equal(y.data().view(np.uint8), y0.data().view(np.uint8))
        assert (T.nnz, T.fill, T.longest_row, T.truncated_rows, T.dropped_entries, T.setup_seconds) == kept
        if fake is not None:
            def since(name):
                return fake.calls.get(name, 0) - before.get(name, 0)
            assert since('fsvalues_update_device') == 3 and since('fsvalues_update') == 1
            assert since('fsvalues_plan') == (4 if work else 0)


def cpu_tensor_takes_host_path(fake):
    """(CPU tier, tensors NOT counted as device memory) a CPU tensor is taken as its SciPy matrix."""
    from raleigh_amd.algebra.hip.precond import ApproximateInverse
    A = lv.lap('d')
    B = revalued(A, 92)
    T = ApproximateInverse(A)
    T.update_values(csr_tensor(B, 'cpu'))
    assert fake.calls.get('fsvalues_update', 0) == 1 and fake.calls.get('fsvalues_update_device', 0) == 0
    assert T.updates == 1 and same_bits(T.csr(), ApproximateInverse(B).csr())


def class_rejections(device, fake=None):
    from raleigh_amd import _lib
    from raleigh_amd.algebra.hip.precond import ApproximateInverse
    A = base.matrix('d')
    T = ApproximateInverse(A, steps=2, drop=0.05, work='native')
    G = T.csr()
    before = dict(fake.calls) if fake is not None else None
    small = lv.lap('d')
    for bad, text in ((small, 'built for a matrix of size 777, got one of size %d' % small.shape[0]),
                      (csr_tensor(small, device), 'built for a matrix of size 777'),
                      (A.astype(np.float32), 'built for a matrix of type float64, got one of type float32'),
                      (csr_tensor(A.astype(np.complex128), device), 'built for a matrix of type float64'),
                      (sp.csr_matrix(A[:400]), 'square')):
        with pytest.raises(ValueError, match=text):
            T.update_values(bad)
    with pytest.raises(ValueError, match='layout'):
        T.update_values(csr_tensor(A, device).to_dense())
    if fake is not None:
        assert dict(fake.calls) == before                   # refused before any library call
    import torch
    t = csr_tensor(A, device)
    col = t.col_indices().clone()
    k = int(A.indptr[100]) + 1
    col[k], col[k + 1] = int(A.indices[k + 1]), int(A.indices[k])
    with pytest.raises(ValueError, match='not canonical CSR.*rlh_fsvalues_update_device: the columns of row 100 must ascend'):
        T.update_values(torch.sparse_csr_tensor(t.crow_indices(), col, t.values(), size=t.shape))
    with pytest.raises(_lib.RlhError, match='rlh_fsvalues_update_device: row 300 does not store its diagonal entry'):
        T.update_values(csr_tensor(_without(A, 300, 300), device))
    C = A.copy().tolil()
    C[350, 350] = -3.0
    with pytest.raises(_lib.RlhError, match='rlh_fsvalues_update: local block of row 350 is not positive definite'):
        T.update_values(sp.csr_matrix(C))
    assert T.updates == 0 and same_bits(T.csr(), G)
    T.update_values(revalued(A, 91))
    assert T.updates == 1 and (T.steps, T.drop) == (2, 0.05) and T.dropped_entries > 0 and not same_bits(T.csr(), G)


# ---------------------------------------------------------------- 12. end to end
def end_to_end(device):
    import scipy.linalg
    from raleigh_amd.synthetic import fe_surrogate
    from raleigh_amd.interfaces import partial_hevp
    from raleigh_amd.algebra.hip.precond import ApproximateInverse
    from _device_operator_cases import TOL
    A = sp.csr_matrix(fe_surrogate(grid=(7, 6, 5))).astype(np.float64)
    A.sort_indices()
    B = revalued(A, 95)
    which = 6
    exact = {id(M): scipy.linalg.eigvalsh(hermitian_from_upper(M).toarray())[:which] for M in (A, B)}
    a, b = csr_tensor(A, device), csr_tensor(B, device)

    def solved(t, M, T):
        np.random.seed(1)
        lmd, x, status = partial_hevp(t, T=T, which=which, tol=TOL, verb=-1)
        assert status == 0
        assert np.max(np.abs(lmd[:which] - exact[id(M)])) <= 1e-10
        return partial_hevp.last['iterations']
    its = {}
    for name, kw in (('level 1', {}), ('adaptive, drop=0.1', dict(steps=4, step_size=2, drop=0.1))):
        T = ApproximateInverse(a, **kw)
        first = solved(a, A, T)
        T.update_values(b)
        assert T.updates == 1
        its[name] = (first, solved(b, B, T), solved(b, B, ApproximateInverse(b, **kw)))
        print('%s: %d iterations on A; on A\' %d with the updated preconditioner, %d with a fresh one' % ((name,) + its[name]))
    assert its['level 1'][1] == its['level 1'][2]
    return its
