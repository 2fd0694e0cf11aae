"""Level-of-fill patterns of the approximate inverse (rlh_fsai_create_levels*, ApproximateInverse(levels=...)): cases
shared by the CPU tier (tests/fake_fsai.py) and the GPU tier.  The raw entry points (`create`, `built`), the helpers, the
bound of the defining property (`check_row`, `beta`) and the N = 777 profile matrix come from tests/_fsai_cases.py.

THE ORACLE.  With T the boolean pattern of the stored entries (i, j), j <= i, of A (explicit zeros count), the level
pattern is that of T^levels, formed by SciPy sparse products; a row keeps its max_row largest columns, and is
truncated when it has more.  Nothing of it is shared with the library or with the stand-in (which unites index sets).

THE BANDED MATRIX.  Row i stores the columns i - w_i .. i below and on the diagonal, w constant over five stretches
of 80 rows: w = 1, 5, 10, 20, 40, mirrored above, n = 400.  Inside a stretch a level-2 row is i - 2 w .. i: 3, 11, 21,
41 and 81 members, one of every class of the set-up's bins (1 .. 8, 9 .. 16, 17 .. 32, 33 .. 64) and one that
max_row = 64 cuts.  `banded_narrow` (w = 1, 2, 4, 7, 12, 21) has at most 64 members at level 3: the comparison of
Kaporin numbers needs nested, hence uncut, patterns, which the first matrix by its construction cannot give.

LAUNCH GEOMETRY the loop cases rely on: every kernel runs at most 8 workgroups per CU and walks its rows in a
grid-stride loop; the pattern kernels take 4 rows per workgroup (one wave each), the 16-lane set-up 16 rows, the 32-lane
set-up 8 rows in real arithmetic.
"""

import functools

import numpy as np
import pytest
import scipy.sparse as sp

import _fsai_cases as base
from _fsai_cases import (TYPES, _L, _check, built, check_row, create, csr_tensor, destroy, get, hermitian_from_upper, kaporin,
                         last_error, levels_of, same_bits)

BLOCKS_PER_CU = 8
PATTERN_ROWS_PER_BLOCK = 4
ROWS_PER_BLOCK = {16: 16, 32: 8}
WIDTHS = (1, 5, 10, 20, 40)
WIDTHS_NARROW = (1, 2, 4, 7, 12, 21)
CLASSES = ((1, 8), (9, 16), (17, 32), (33, 64), (65, 10 ** 9))


# ---------------------------------------------------------------- matrices
def band(widths, dt, seed):
    """Hermitian, strictly diagonally dominant with a positive diagonal; row i stores the columns i - widths[i] .. i
    (from 0 on) and their mirror images."""
    widths = np.asarray(widths, dtype=np.int64)
    n = widths.size
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for o in range(1, int(widths.max()) + 1):
        r = np.flatnonzero((widths >= o) & (np.arange(n) >= o))
        rows.append(r)
        cols.append(r - o)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = rng.uniform(-1.0, 1.0, rows.size)
    if np.dtype(dt).kind == 'c':
        vals = vals + 1j * rng.uniform(-1.0, 1.0, rows.size)
    low = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    off = low + low.conj().T
    diag = np.asarray(abs(off).sum(axis=1)).ravel() + 1.0 + rng.uniform(0.0, 1.0, n)
    A = sp.csr_matrix(off + sp.diags(diag)).astype(dt)
    A.sort_indices()
    return A


@functools.lru_cache(maxsize=None)
def banded(code, narrow=False):
    w = WIDTHS_NARROW if narrow else WIDTHS
    return band(np.repeat(w, 66 if narrow else 80), TYPES[code], 31 if narrow else 30)


@functools.lru_cache(maxsize=None)
def lap(code, nx=6, ny=5, nz=4):
    from raleigh_amd.synthetic import lap3d_rows
    A = sp.csr_matrix(lap3d_rows(nx, ny, nz, 1.0, 1.01, 1.02, 0, nx * ny * nz)).astype(TYPES[code])
    A.sort_indices()
    return A


def inputs(code):
    return {'lap3d': lap(code), 'profile': base.matrix(code), 'banded': banded(code)}


# ---------------------------------------------------------------- the oracle
def _tril_pattern(A):
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    keep = A.indices <= rows
    return sp.csr_matrix((np.ones(int(keep.sum())), (rows[keep], A.indices[keep])), shape=A.shape)


@functools.lru_cache(maxsize=None)
def _full_pattern(A_id, levels):
    T = _tril_pattern(_KEPT[A_id])
    P = T.copy()
    for _ in range(levels - 1):
        P = sp.csr_matrix(P @ T)
        P.data[:] = 1.0
    P.sort_indices()
    return P


_KEPT = {}


def full_pattern(A, levels):
    """The pattern of tril(A)^levels as CSR (computed once per matrix object and level, never written)."""
    _KEPT[id(A)] = A
    return _full_pattern(id(A), levels)


def oracle(A, levels, max_row):
    """indptr, indices, truncated rows and the longest row of G's pattern."""
    P = full_pattern(A, levels)
    lens = np.diff(P.indptr)
    at = np.arange(P.nnz) - np.repeat(P.indptr[:-1], lens)
    keep = at >= np.repeat(lens - max_row, lens)
    kept = np.minimum(lens, max_row)
    indptr = np.zeros(A.shape[0] + 1, dtype=np.int64)
    np.cumsum(kept, out=indptr[1:])
    return indptr, P.indices[keep], int(np.sum(lens > max_row)), int(kept.max())


def padded(A, levels):
    """A plus explicit zeros on the symmetrised pattern of tril(A)^levels."""
    P = full_pattern(A, levels).tocoo()
    return base.padded_with(A, P.row, P.col)


# ---------------------------------------------------------------- 1. the pattern, exactly
def banded_classes():
    A = banded('d')
    lens = np.diff(full_pattern(A, 2).indptr)
    for lo, hi in CLASSES:
        assert np.any((lens >= lo) & (lens <= hi)), (lo, hi)


def pattern(which, levels):
    A = inputs('d')[which]
    for max_row in (64, 5):
        indptr, indices, cut, longest = oracle(A, levels, max_row)
        for bits in (32, 64):
            G, f = built(A, '_levels', levels, bits=bits, max_row=max_row)
            assert np.array_equal(G.indptr, indptr) and np.array_equal(G.indices, indices), (which, levels, max_row, bits)
            assert f['truncated'] == cut and f['longest'] == longest and f['nnz'] == len(indices)


# ---------------------------------------------------------------- 2. padding, bit for bit
def padding(code):
    for A in (lap(code), banded(code)):
        for levels in (2, 3):
            B = padded(A, levels)
            for max_row in (64, 5):
                want, fw = built(B, max_row=max_row)
                cut = oracle(A, levels, max_row)[2]
                assert fw['truncated'] == cut and (cut > 0) == (max_row == 5 or A is banded(code))
                for host in (False, True):
                    G, f = built(A, '_levels', levels, host=host, max_row=max_row)
                    assert same_bits(G, want), (levels, max_row, host)
                    assert f['truncated'] == cut


# ---------------------------------------------------------------- 3. the defining property on the level pattern
def defining_property(code, levels):
    A, D = base.matrix(code), base.dense_wide(code)
    B = A.copy()
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    B.data[B.indices < rows] = np.nan                      # nothing below the diagonal is read
    G, f = built(B, '_levels', levels, bits=32)
    indptr, indices, cut, longest = oracle(A, levels, 64)
    assert np.array_equal(G.indptr, indptr) and f['truncated'] == cut and cut > 0 and f['longest'] == longest == 64
    worst = 0.0
    for i in range(A.shape[0]):
        p = indices[indptr[i]:indptr[i + 1]]
        worst = max(worst, check_row(G, i, p, D[np.ix_(p, p)], TYPES[code]))
    print('largest residual / bound: %.3g' % worst)


# ---------------------------------------------------------------- 4. level 1 is what it was
def unchanged_level_one(code):
    from raleigh_amd.algebra.hip.precond import ApproximateInverse
    A = base.matrix(code)
    dt = A.dtype.type
    made = [create(A, '_levels', 1, bits=32), create(A, bits=32), create(A, '_levels', 1, host=True), create(A, host=True)]
    try:
        for rc, _ in made:
            _check(rc)
        gs = [get(h, dt) for _, h in made]
        assert all(levels_of(h) == 1 for _, h in made)
        for G in gs[1:]:
            assert same_bits(gs[0], G)
        assert same_bits(gs[0], ApproximateInverse(A).csr()) and same_bits(gs[0], ApproximateInverse(A, levels=1).csr())
        assert ApproximateInverse(A).levels == 1
        n, m = A.shape[0], 5
        rng = np.random.default_rng(41)
        x = rng.standard_normal((m, n))
        if np.dtype(dt).kind == 'c':
            x = x + 1j * rng.standard_normal((m, n))
        x = x.astype(dt)
        out = []
        for _, h in made[:2]:
            X, Y = base.dev(x), base.dev(np.zeros_like(x))
            _check(_L().rlh_fsai_apply(h, m, X.ptr, n, Y.ptr, n))
            out.append(base.fetch(Y, x.size, dt))
        assert np.array_equal(out[0].view(np.uint8), out[1].view(np.uint8))
        assert np.all(np.isfinite(out[0]))
    finally:
        for _, h in made:
            destroy(h)


# ---------------------------------------------------------------- 5. the bins
def bins(code, monkeypatch):
    A = banded(code)
    monkeypatch.setenv('RLH_FSAI_BINS', '0')
    two, f2 = built(A, '_levels', 2, bits=32)
    monkeypatch.delenv('RLH_FSAI_BINS')
    four, f4 = built(A, '_levels', 2, bits=32)
    assert same_bits(two, four) and f2['truncated'] == f4['truncated'] > 0 and f2['longest'] == f4['longest'] == 64
    lens = np.diff(four.indptr)
    for lo, hi in CLASSES[:4]:
        assert np.any((lens >= lo) & (lens <= hi)), (lo, hi)


# ---------------------------------------------------------------- 6. every loop past its first trip
def loops(cu, lanes):
    """A band of w = 4 (16 lanes) or 8 (32 lanes) at level 2: rows of 2 w + 1 = 9 or 17 entries, more of them than one
    pass of the bin's set-up grid holds, which is more than one pass of the pattern kernels holds."""
    w = {16: 4, 32: 8}[lanes]
    per_pass, per_pattern_pass = cu * BLOCKS_PER_CU * ROWS_PER_BLOCK[lanes], cu * BLOCKS_PER_CU * PATTERN_ROWS_PER_BLOCK
    n = per_pass + 300
    A = band(np.full(n, w), np.float64, 32)
    G, f = built(A, '_levels', 2, bits=32)
    indptr, indices, cut, longest = oracle(A, 2, 64)
    assert cut == 0 == f['truncated'] and longest == 2 * w + 1 == f['longest']
    assert np.array_equal(G.indptr, indptr) and np.array_equal(G.indices, indices)
    lens = np.diff(indptr)
    in_bin = np.flatnonzero((lens > lanes // 2) & (lens <= lanes))          # ascending: the order of the bin's list
    assert in_bin.size > per_pass and n > per_pattern_pass + 1
    rows = [0, 1, w, in_bin[0], per_pattern_pass - 1, per_pattern_pass, per_pattern_pass + 1, in_bin[per_pass - 1],
            in_bin[per_pass], n - 1]
    F = hermitian_from_upper(A).tocsr()
    for i in sorted(set(int(r) for r in rows)):
        p = indices[indptr[i]:indptr[i + 1]]
        check_row(G, i, p, F[p][:, p].toarray().astype(np.longdouble), np.float64)


# ---------------------------------------------------------------- 7. quality never falls with the level
def monotone_quality():
    out = []
    for A in (lap('d', 8, 8, 8), banded('d', narrow=True)):
        n = A.shape[0]
        d = hermitian_from_upper(A).toarray()
        ks = []
        for levels in (1, 2, 3):
            G, f = built(A, '_levels', levels, bits=32)
            assert f['truncated'] == 0, levels
            g = G.toarray()
            ks.append(kaporin(g @ d @ g.T))
        print('Kaporin numbers at levels 1, 2, 3 (n = %d): %.6f %.6f %.6f' % ((n,) + tuple(ks)))
        for a, b in zip(ks, ks[1:]):
            assert b <= a * (1 + 100 * n * base.unit(np.float64))
        out.append(ks)
    return out


# ---------------------------------------------------------------- 8. rejections
def rejections_raw():
    A = base.matrix('d')
    for host, name in ((False, 'rlh_fsai_create_levels_device'), (True, 'rlh_fsai_create_levels')):
        for levels in (0, 9):
            rc, h = create(A, '_levels', levels, host=host)
            assert rc != 0 and not h.value
            assert last_error().endswith('%s: levels must lie in [1, 8], got %d' % (name, levels)), last_error()
        rc, h = create(A, '_levels', 9, host=host, max_row=65)
        assert rc != 0 and not h.value
        assert last_error().endswith('%s: max_row must lie in [1, 64], got 65' % name), last_error()
        rc, h = create(A, '_levels', 8, host=host, max_row=3)
        _check(rc)
        assert levels_of(h) == 8
        destroy(h)


def rejections_class(fake=None):
    from raleigh_amd.algebra.hip.precond import ApproximateInverse
    A = base.matrix('d')
    before = dict(fake.calls) if fake is not None else None
    for levels in (0, 9, -1):
        with pytest.raises(ValueError, match=r'levels must lie in \[1, 8\], got %d' % levels):
            ApproximateInverse(A, levels=levels)
    with pytest.raises(ValueError, match='max_row'):
        ApproximateInverse(A, max_row=65, levels=9)
    if fake is not None:
        assert dict(fake.calls) == before                   # refused before any library call


# ---------------------------------------------------------------- the class: three kinds of input
def class_inputs(device):
    from raleigh_amd.algebra.hip.precond import ApproximateInverse
    A = banded('d')
    want, f = built(A, '_levels', 2)
    made = [ApproximateInverse(A, levels=2), ApproximateInverse(csr_tensor(A, device), levels=2),
            ApproximateInverse(csr_tensor(A, 'cpu'), levels=2)]
    for T in made:
        assert T.levels == 2 and same_bits(T.csr(), want)
        assert T.truncated_rows == f['truncated'] and T.longest_row == 64 and T.nnz == want.nnz
        assert abs(T.fill - want.nnz / A.nnz) < 1e-15
    return made


# ---------------------------------------------------------------- 9. end to end
def end_to_end(device):
    import scipy.linalg
    import torch
    from raleigh_amd.interfaces import partial_hevp
    from raleigh_amd.algebra.hip.precond import ApproximateInverse
    A = lap('d', 12, 11, 10)
    which = 6
    exact = scipy.linalg.eigvalsh(hermitian_from_upper(A).toarray())[:which]
    a = csr_tensor(A, device)
    its = {}
    for levels in (2, 1):
        T = ApproximateInverse(a, levels=levels)
        np.random.seed(1)
        lmd, x, status = partial_hevp(a, T=T, which=which, tol=1e-6, verb=-1)
        its[levels] = partial_hevp.last['iterations']
        assert status == 0
        if levels == 2:
            assert np.max(np.abs(lmd[:which] - exact)) <= 1e-10
            assert isinstance(x, torch.Tensor) and x.device.type == torch.device(device).type
    print('iterations: %d at level 2, %d at level 1' % (its[2], its[1]))
    assert its[2] < its[1]
    return its
