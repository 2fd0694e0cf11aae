"""The approximate-inverse preconditioner (rlh_fsai_*, ApproximateInverse), cases shared by the CPU tier
(tests/fake_fsai.py; CPU tensors stand for device tensors) and the GPU tier.

Test matrices are sparse Hermitian with a chosen profile of lower-row lengths (row i stores L_i = min(profile[i mod
len(profile)], i + 1) entries with column <= i, the diagonal among them, and the structure is made symmetric), strictly
diagonally dominant with a positive diagonal, hence positive definite.

The library's set-up takes rows of at most SHORT = 8 kept entries on 8 lanes each, 32 rows per workgroup, and longer
rows on one single-wave workgroup each; both kernels run at most 8 workgroups per CU and walk their rows in a
grid-stride loop.  The short / long boundary of the profiles is therefore 8 | 9.

THE BOUND OF THE DEFINING PROPERTY (`beta`).  Row i of G is g with S g^H = e_k / g_kk, S = A[P, P] (k x k).  The library
factorises S = R^H R in double (unit roundoff u = 2^-53) and solves R w = e_k by back substitution; g = conj(w).
Higham, Accuracy and Stability, Thm 10.3 / 10.4 and (10.7): R^H R = S + D1, |D1| <= gamma_{k+1} |R^H| |R|; the solve
gives (R + D2) w = e_k (1 + d), |D2| <= gamma_k |R|, where |d| <= 2 u comes from w_k = 1 / R_kk being formed by one
division; and || |R^H| |R| ||_2 <= k / (1 - k gamma_{k+1}) ||S||_2.  Multiplying by R^H,
    S w - e_k R_kk (1 + d) = -(D1 + R^H D2) w,  of norm <= gamma_{3k+1} k / (1 - k gamma_{k+1}) ||S|| ||w||
(gamma_{k+1} + gamma_k <= gamma_{3k+1}: the constant of Thm 10.4, which covers a second triangular solve the library
does not need).  1 / g_kk = R_kk up to two more roundings, and R_kk = 1 / g_kk <= ||S|| ||g|| (the norm of the
defining equation), so e_k / g_kk differs from e_k R_kk (1 + d) by at most 4 u ||S|| ||g||.  Then g is rounded ONCE to
the storage type (unit roundoff us, relative, per entry): S g^H moves by at most us ||S|| ||g||, 1 / g_kk by at most
us / (1 - us) times itself, and ||g|| itself by a factor 1 + us.  Together
    ||S g^H - e_k / g_kk||_2 <= beta ||S||_2 ||g||_2,
    beta = (gamma_{3k+1} k / (1 - k gamma_{k+1}) + 4 u) (1 + us) + 2 us / (1 - us).
In complex arithmetic a product carries sqrt(2) gamma_2 < 4 u in place of u (Higham Lemma 3.5; the divisions are by
real numbers), so the gammas are formed with 4 u there.  Nothing in beta comes from a measurement.  The same bound
covers the diagonal: (G A G^H)_ii = g S g^H = 1 + g r, |g r| <= ||g|| ||r|| <= beta ||S|| ||g||^2.
The residual is evaluated in longdouble; ||S||_2 is a float64 singular value (relative error ~1e-15 on the bound's side).
"""

import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from _device_data_cases import csr_tensor, host

N = 777
TYPES = {'s': np.float32, 'd': np.float64, 'c': np.complex64, 'z': np.complex128}
SHORT = 8                       # rows of at most SHORT kept entries take the 8-lane path
BLOCKS_PER_CU = 8               # grid of a set-up kernel: at most this many workgroups per CU
SHORT_ROWS_PER_BLOCK = 32
PROFILE = (1, 2, 8, 9, 32, 33, 63, 64)
PROFILE_CUT = (3, 65, 100, 8, 9, 20)
VECTORS = (1, 3, 8, 33)


def _L():
    from raleigh_amd import _lib
    return _lib.lib()


def _check(rc):
    from raleigh_amd import _lib
    _lib.check(rc)


def last_error():
    msg = _L().rlh_last_error()
    return msg.decode() if isinstance(msg, bytes) else msg


def dev(a):
    """A device copy of a host array (kept alive by the returned buffer)."""
    from raleigh_amd.algebra.hip.memory import DeviceBuffer
    from raleigh_amd import _lib
    a = np.ascontiguousarray(a)
    buf = DeviceBuffer(max(a.nbytes, 16), zero=False)
    if a.nbytes:
        _check(_L().rlh_h2d(buf.ptr, _lib.host_ptr(a), a.nbytes))
    return buf


def fetch(buf, count, dt):
    from raleigh_amd import _lib
    out = np.empty(count, dtype=dt)
    if count:
        _check(_L().rlh_d2h(_lib.host_ptr(out), buf.ptr, out.nbytes))
    return out


def unit(dt):
    return float(np.finfo(np.dtype(dt)).eps) / 2


def rsqrt_rounded(d):
    """d^(-1/2) correctly rounded to double: the longdouble value rounded, then moved to a neighbour where the exact
    comparison d m^2 <> 1 at the midpoint m says so (rounding twice, 64 then 53 bits, misses about one value in 2^11)."""
    from fractions import Fraction
    g = float(1 / np.sqrt(np.longdouble(d)))
    for _ in range(2):
        up, down = float(np.nextafter(g, np.inf)), float(np.nextafter(g, 0.0))
        if Fraction(d) * ((Fraction(g) + Fraction(up)) / 2) ** 2 < 1:
            g = up
        elif Fraction(d) * ((Fraction(g) + Fraction(down)) / 2) ** 2 > 1:
            g = down
        else:
            break
    return g


# ---------------------------------------------------------------- matrices
def _with_profile(n, profile, dt, seed, window=160):
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for i in range(n):
        want = min(profile[i % len(profile)], i + 1) - 1
        lo = max(0, i - max(window, want))
        pick = np.sort(rng.choice(np.arange(lo, i), want, replace=False)) if want else np.zeros(0, dtype=np.int64)
        rows.append(np.full(want, i))
        cols.append(pick)
    rows, cols = np.concatenate(rows).astype(np.int64), np.concatenate(cols).astype(np.int64)
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
def matrix(code, which='profile'):
    """The n = 777 test matrices: 'profile' (lower-row lengths 1, 2, 8, 9, 32, 33, 63, 64) and 'cut' (3, 65, 100, 8, 9,
    20: rows longer than max_row = 64)."""
    A = _with_profile(N, PROFILE if which == 'profile' else PROFILE_CUT, TYPES[code], 11 if which == 'profile' else 12)
    lower = lower_lengths(A)
    for want in (PROFILE if which == 'profile' else PROFILE_CUT):
        assert np.any(lower == want), want
    return A


def lower_lengths(A):
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    return np.bincount(rows[A.indices <= rows], minlength=A.shape[0])


def hermitian_from_upper(A):
    u = sp.triu(A, format='csr')
    return sp.csr_matrix(u + sp.triu(A, k=1, format='csr').conj().T)


@functools.lru_cache(maxsize=None)
def dense_wide(code, which='profile'):
    """The operator the upper triangle defines, dense, in longdouble / clongdouble (computed once, never written)."""
    A = matrix(code, which)
    d = hermitian_from_upper(A).toarray().astype(np.clongdouble if A.dtype.kind == 'c' else np.longdouble)
    d.setflags(write=False)
    return d


# ---------------------------------------------------------------- the raw entry points
def create(A, entry='', levels=None, steps=None, step_size=None, host=False, bits=64, max_row=64, indptr=None, indices=None,
           keep=None, n=None):
    """(rc, handle) of one of the six create calls: rlh_fsai_create<entry> on A's arrays (host=True) or
    rlh_fsai_create<entry>_device on device copies of them (or of the given indptr / indices; keep collects the arrays
    and their buffers).  entry: '' , '_levels' (takes levels) or '_adaptive' (takes levels, steps and step_size)."""
    from raleigh_amd import _lib
    more = {'': (), '_levels': (levels,), '_adaptive': (levels, steps, step_size)}[entry]
    it = {32: np.int32, 64: np.int64}.get(bits, np.int64)
    arrays = ((A.indptr if indptr is None else indptr).astype(np.int64 if host else it),
              (A.indices if indices is None else indices).astype(np.int32 if host else it), np.ascontiguousarray(A.data))
    h = ctypes.c_void_p(12345)
    head = (ctypes.byref(h), _lib.DTYPE_CODE[A.dtype.type], A.shape[0] if n is None else n)
    if host:
        return getattr(_L(), 'rlh_fsai_create' + entry)(*head, *[_lib.host_ptr(a) for a in arrays], max_row, *more), h
    bufs = [dev(a) for a in arrays]
    rc = getattr(_L(), 'rlh_fsai_create%s_device' % entry)(*head, bits, *[b.ptr for b in bufs], max_row, *more)
    if keep is not None:
        keep.extend(zip(arrays, bufs))
    return rc, h


def info(h):
    n, nnz, longest, cut, nbytes, sec = (ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(),
                                         ctypes.c_int64(), ctypes.c_double())
    _check(_L().rlh_fsai_info(h, ctypes.byref(n), ctypes.byref(nnz), ctypes.byref(longest), ctypes.byref(cut),
                              ctypes.byref(nbytes), ctypes.byref(sec)))
    return dict(n=n.value, nnz=nnz.value, longest=longest.value, truncated=cut.value, bytes=nbytes.value, seconds=sec.value)


def get(h, dt):
    """G of a handle as SciPy CSR."""
    from raleigh_amd import _lib
    f = info(h)
    ip = np.zeros(f['n'] + 1, dtype=np.int64)
    ix = np.zeros(max(f['nnz'], 1), dtype=np.int32)
    va = np.zeros(max(f['nnz'], 1), dtype=dt)
    _check(_L().rlh_fsai_get(h, _lib.host_ptr(ip), _lib.host_ptr(ix), _lib.host_ptr(va)))
    assert ip[0] == 0 and ip[-1] == f['nnz']
    return sp.csr_matrix((va[:f['nnz']], ix[:f['nnz']], ip), shape=(f['n'], f['n']))


def destroy(h):
    _L().rlh_fsai_destroy(h)


def levels_of(h):
    v = ctypes.c_int(-1)
    _check(_L().rlh_fsai_levels(h, ctypes.byref(v)))
    return v.value


def adaptive_of(h):
    a, b = ctypes.c_int(-1), ctypes.c_int(-1)
    _check(_L().rlh_fsai_adaptive(h, ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


def built(A, entry='', levels=None, steps=None, step_size=None, **kw):
    """G (SciPy) and the info record of a build (the arguments of `create`) that must succeed; where the entry point
    takes levels or steps, the handle must answer with them."""
    rc, h = create(A, entry, levels, steps, step_size, **kw)
    _check(rc)
    try:
        if entry:
            assert levels_of(h) == levels
        if entry == '_adaptive':
            assert adaptive_of(h) == (steps, step_size)
        return get(h, A.dtype.type), info(h)
    finally:
        destroy(h)


def padded_with(A, rows, cols):
    """A plus explicit zeros at the positions (rows, cols) and at their mirror images."""
    n = A.shape[0]
    own = np.repeat(np.arange(n, dtype=np.int64), np.diff(A.indptr)) * n + A.indices
    pr, pc = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    key = np.unique(np.concatenate([own, pr * n + pc, pc * n + pr]))
    data = np.zeros(key.size, dtype=A.dtype)
    data[np.searchsorted(key, own)] = A.data
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(key // n, minlength=n), out=indptr[1:])
    B = sp.csr_matrix((data, (key % n).astype(np.int32), indptr), shape=A.shape)
    assert B.nnz == key.size and B.has_sorted_indices
    return B


def same_bits(G1, G2):
    return (np.array_equal(G1.indptr, G2.indptr) and np.array_equal(G1.indices, G2.indices)
            and np.array_equal(np.ascontiguousarray(G1.data).view(np.uint8), np.ascontiguousarray(G2.data).view(np.uint8)))


# ---------------------------------------------------------------- property 1
def beta(k, dt):
    u, us = 2.0 ** -53, unit(dt)
    if np.dtype(dt).kind == 'c':
        u = 4 * u

    def gamma(j):
        return j * u / (1 - j * u)
    return (gamma(3 * k + 1) * k / (1 - k * gamma(k + 1)) + 4 * u) * (1 + us) + 2 * us / (1 - us)


def expected_pattern(A, i, max_row):
    p = A.indices[A.indptr[i]:A.indptr[i + 1]]
    p = p[p <= i]
    return p[-max_row:] if len(p) > max_row else p


def check_row(G, i, pattern, block, dt):
    """The defining property of row i of the fetched G against S = `block` (longdouble, k x k) on `pattern`."""
    cols = G.indices[G.indptr[i]:G.indptr[i + 1]]
    assert np.array_equal(cols, pattern), i
    wide = block.dtype
    g = G.data[G.indptr[i]:G.indptr[i + 1]].astype(wide)
    assert np.all(np.isfinite(g.astype(np.complex128)))
    k = len(cols)
    assert g[-1].imag == 0 and g[-1].real > 0, i
    e = np.zeros(k, dtype=wide)
    e[-1] = 1 / g[-1].real
    r = block @ np.conj(g) - e
    snorm = float(np.linalg.norm(block.astype(np.complex128 if wide == np.clongdouble else np.float64), 2))
    gnorm = float(np.sqrt(np.sum(np.abs(g) ** 2)))
    rnorm = float(np.sqrt(np.sum(np.abs(r) ** 2)))
    b = beta(k, dt)
    assert rnorm <= b * snorm * gnorm, (i, k, rnorm / (snorm * gnorm), b)
    d = g @ block @ np.conj(g)
    assert abs(d - 1) <= b * snorm * gnorm ** 2, (i, k, float(abs(d - 1)), b)
    return rnorm / (snorm * gnorm * b)


def check_all_rows(G, code, which, max_row=64):
    A, D = matrix(code, which), dense_wide(code, which)
    worst = 0.0
    for i in range(A.shape[0]):
        p = expected_pattern(A, i, max_row)
        worst = max(worst, check_row(G, i, p, D[np.ix_(p, p)], TYPES[code]))
    print('largest residual / bound: %.3g' % worst)


def defining_property(code, bits):
    A = matrix(code)
    kept = []
    rc, h = create(A, bits=bits, keep=kept)
    _check(rc)
    try:
        G, f = get(h, A.dtype.type), info(h)
        for arr, buf in kept:                                   # the caller's arrays are as they were
            assert np.array_equal(fetch(buf, arr.size, arr.dtype), arr)
    finally:
        destroy(h)
    lower = lower_lengths(A)
    assert f['n'] == N and f['nnz'] == int(lower.sum()) == G.nnz and f['longest'] == 64 and f['truncated'] == 0
    assert f['bytes'] >= 2 * G.nnz * (A.dtype.itemsize + 4)
    check_all_rows(G, code, 'profile')


def truncation(code):
    A = matrix(code, 'cut')
    lower = lower_lengths(A)
    for max_row in (64, 8, 1):
        G, f = built(A, bits=32, max_row=max_row)
        assert f['truncated'] == int(np.sum(lower > max_row)) and f['truncated'] > 0
        assert f['longest'] == max_row and f['nnz'] == int(np.minimum(lower, max_row).sum())
        check_all_rows(G, code, 'cut', max_row)                 # (the kept columns are the largest: expected_pattern)
        if max_row == 1:
            want = np.array([rsqrt_rounded(float(d)) for d in A.diagonal().real]).astype(A.dtype)
            assert np.array_equal(G.indices, np.arange(N)) and np.array_equal(G.data, want)


def upper_defines(code):
    A = matrix(code)
    B = A.copy()
    rows = np.repeat(np.arange(N), np.diff(A.indptr))
    B.data[B.indices < rows] = np.nan
    G, _ = built(A)
    Gn, _ = built(B)
    assert same_bits(G, Gn) and np.all(np.isfinite(Gn.data))


def bit_identity(code):
    A = matrix(code)
    G, _ = built(A, bits=64)
    G2, _ = built(A, bits=64)
    G32, _ = built(A, bits=32)
    Gh, _ = built(A, host=True)
    assert same_bits(G, G2) and same_bits(G, G32) and same_bits(G, Gh)


# ---------------------------------------------------------------- every loop past its first trip
def _sampled(A, G, rows, dt):
    F = hermitian_from_upper(A).tocsr()
    wide = np.clongdouble if A.dtype.kind == 'c' else np.longdouble
    for i in rows:
        p = expected_pattern(A, int(i), 64)
        check_row(G, int(i), p, F[p][:, p].toarray().astype(wide), dt)


def loops_short(cu):
    """7-point Laplacian rows (k <= 4, all on the 8-lane path), more of them than one pass of the grid covers."""
    from raleigh_amd.synthetic import lap3d_rows
    per_pass = cu * BLOCKS_PER_CU * SHORT_ROWS_PER_BLOCK
    nz = per_pass // (32 * 32) + 1
    n = 32 * 32 * nz
    assert n > per_pass
    A = sp.csr_matrix(lap3d_rows(32, 32, nz, 1.0, 1.01, 1.02, 0, n).astype(np.float64))
    G, f = built(A, bits=32)
    assert f['longest'] == 4 and f['nnz'] == int(lower_lengths(A).sum())
    rows = [0, 1, 32, 1024, per_pass - 1, per_pass, per_pass + 1, n - 1]
    _sampled(A, G, [r for r in rows if 0 <= r < n], np.float64)


def loops_long(cu):
    """Rows of 20 lower entries (the one-wave path), more of them than the grid has workgroups."""
    per_pass = cu * BLOCKS_PER_CU
    n = per_pass + 300
    A = _with_profile(n, (20,), np.float64, 13, window=40)
    lower = lower_lengths(A)
    long_rows = np.flatnonzero(lower > SHORT)
    assert long_rows.size > per_pass and np.all(lower[19:] == 20)
    G, f = built(A, bits=64)
    assert f['longest'] == 20
    rows = [0, 7, long_rows[0], long_rows[1], long_rows[per_pass - 1], long_rows[per_pass], long_rows[per_pass + 1], n - 1]
    _sampled(A, G, rows, np.float64)


# ---------------------------------------------------------------- application
def application(code):
    dt = TYPES[code]
    A = matrix(code)
    rc, h = create(A, bits=32)
    _check(rc)
    try:
        G = get(h, dt)
        wide = np.clongdouble if A.dtype.kind == 'c' else np.longdouble
        Gd = G.toarray().astype(wide)
        Ga = np.abs(G.toarray()).astype(np.float64)
        a, b = int(np.diff(G.indptr).max()), int(np.diff(G.tocsc().indptr).max())
        rng = np.random.default_rng(21)
        ld, guard = N + 5, 2
        for m in VECTORS:
            x = rng.standard_normal((m + guard, ld))
            if np.dtype(dt).kind == 'c':
                x = x + 1j * rng.standard_normal((m + guard, ld))
            x = x.astype(dt)
            x[:, N:] = np.nan                                       # padding rows
            x[m:, :] = np.nan                                       # guard columns
            y0 = np.full((m + guard, ld + 3), np.nan, dtype=dt)
            X, Y = dev(x), dev(y0)
            _check(_L().rlh_fsai_apply(h, m, X.ptr, ld, Y.ptr, ld + 3))
            y = fetch(Y, y0.size, dt).reshape(y0.shape)
            assert np.array_equal(fetch(X, x.size, dt).reshape(x.shape).view(np.uint8), x.view(np.uint8))
            assert np.all(np.isnan(y[:, N:])) and np.all(np.isnan(y[m:, :]))
            exact = (np.conj(Gd.T) @ (Gd @ x[:m, :N].astype(wide).T)).T
            bound = (a + b + 2) * unit(dt) * (Ga.T @ (Ga @ np.abs(x[:m, :N]).astype(np.float64).T)).T
            err = np.abs(y[:m, :N].astype(wide) - exact).astype(np.float64)
            assert np.all(err <= bound), (m, float(np.max(err / bound)))
            Y2 = dev(y0)
            _check(_L().rlh_fsai_apply(h, m, X.ptr, ld, Y2.ptr, ld + 3))
            assert np.array_equal(fetch(Y2, y0.size, dt).view(np.uint8), y.reshape(-1).view(np.uint8))
            _check(_L().rlh_fsai_apply(h, m, X.ptr, ld, X.ptr, ld))    # in place
            z = fetch(X, x.size, dt).reshape(x.shape)
            assert np.array_equal(np.ascontiguousarray(z[:m, :N]).view(np.uint8), np.ascontiguousarray(y[:m, :N]).view(np.uint8))
            assert np.all(np.isnan(z[:, N:])) and np.all(np.isnan(z[m:, :]))
    finally:
        destroy(h)


# ---------------------------------------------------------------- rejections
def _without(A, i, j):
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    keep = ~((rows == i) & (A.indices == j))
    assert keep.sum() == A.nnz - 1
    B = sp.csr_matrix((A.data[keep], (rows[keep], A.indices[keep])), shape=A.shape)
    B.sort_indices()
    return B


def _refused(text, A, **kw):
    rc, h = create(A, **kw)
    assert rc != 0 and not h.value, text
    assert text in last_error(), (text, last_error())


def rejections_raw():
    """Status codes of the build, each naming the smallest offending row; a good build afterwards works."""
    A = matrix('d')
    ip, ix = A.indptr.astype(np.int64), A.indices.astype(np.int64)
    B = _without(_without(A, 500, 500), 300, 300)
    _refused('row 300 does not store its diagonal entry', B)
    # the first lower entries of rows 203 and 403 lose their partners above the diagonal: row 203 is named
    j1, j2 = int(A.indices[A.indptr[203]]), int(A.indices[A.indptr[403]])
    assert j1 < 203 and j2 < 403
    B = _without(_without(A, j2, 403), j1, 203)
    _refused('not symmetric: entry (203, %d) has no partner (%d, 203); the device build creates no entries' % (j1, j1), B)
    C = A.copy().tolil()
    C[350, 350] = -3.0
    C[600, 600] = -1.0
    C = sp.csr_matrix(C)
    C.sort_indices()
    _refused('local block of row 350 is not positive definite', C)
    _refused('max_row must lie in [1, 64], got 0', A, max_row=0)
    _refused('max_row must lie in [1, 64], got 65', A, max_row=65)
    _refused('index_bits must be 32 or 64, got 16', A, bits=16)
    row = 100
    k = int(ip[row]) + 1
    assert ip[row + 1] - ip[row] >= 3

    def changed(a, i, v):
        b = a.copy()
        b[i] = v
        return b
    swapped = ix.copy()
    swapped[k], swapped[k + 1] = ix[k + 1], ix[k]
    _refused('indptr decreases at row 49', A, indptr=changed(ip, 50, ip[49] - 1))
    _refused('indptr[0] must be 0', A, indptr=changed(ip, 0, 1))
    _refused('column index out of range in row %d' % row, A, indices=changed(ix, k, N))
    _refused('columns of row %d must ascend strictly' % row, A, indices=swapped)
    rc, h = create(C, host=True)
    assert rc != 0 and not h.value and 'rlh_fsai_create: local block of row 350 is not positive definite' in last_error()
    rc, h = create(A)
    _check(rc)
    destroy(h)


def rejections_class(device):
    from raleigh_amd import _lib
    from raleigh_amd.algebra.hip import Vectors
    from raleigh_amd.algebra.hip.precond import ApproximateInverse
    A = matrix('d')
    with pytest.raises(ValueError, match='max_row'):
        ApproximateInverse(A, max_row=0)
    with pytest.raises(ValueError, match='max_row'):
        ApproximateInverse(A, max_row=65)
    with pytest.raises(ValueError, match='square'):
        ApproximateInverse(sp.csr_matrix(A[:400]))
    with pytest.raises(ValueError, match='square'):
        ApproximateInverse(csr_tensor(sp.csr_matrix(A[:400]), device))
    with pytest.raises(ValueError, match='layout'):
        ApproximateInverse(csr_tensor(A, device).to_dense())
    with pytest.raises(_lib.RlhError, match='row 300 does not store its diagonal entry'):
        ApproximateInverse(csr_tensor(_without(A, 300, 300), device))
    with pytest.raises(_lib.RlhError, match=r'not symmetric: entry \(1, 0\)'):
        ApproximateInverse(csr_tensor(sp.csr_matrix(sp.tril(A)), device))
    import torch
    t = csr_tensor(A, device)
    col = t.col_indices().clone()
    k = int(A.indptr[100]) + 1
    col[k], col[k + 1] = int(A.indices[k + 1]), int(A.indices[k])
    with pytest.raises(ValueError, match='not canonical CSR.*row 100 must ascend'):
        ApproximateInverse(torch.sparse_csr_tensor(t.crow_indices(), col, t.values(), size=t.shape))
    T = ApproximateInverse(t)
    assert T.size() == N and T.data_type() == np.float64 and T.truncated_rows == 0 and T.setup_seconds >= 0
    assert abs(T.fill - lower_lengths(A).sum() / A.nnz) < 1e-15
    assert T.algorithmic_bytes(4) == 2 * T.nnz * 12 + 4 * N * 4 * 8
    x = Vectors(np.ones((3, N)))
    with pytest.raises(ValueError, match='data types differ'):
        T.apply(Vectors(np.ones((3, N), dtype=np.float32)), x)
    with pytest.raises(ValueError, match='dimensions incompatible'):
        T.apply(Vectors(np.ones((3, N + 1))), x)
    with pytest.raises(ValueError, match='vectors differ'):
        T.apply(Vectors(np.ones((2, N))), x)

    class Sharded:
        comm = object()
    with pytest.raises(ValueError, match='row-sharded'):
        T.apply(Sharded(), x)
    # a tensor on the CPU takes the host path and gives the same G; so does the SciPy matrix
    G = T.csr()
    assert same_bits(G, ApproximateInverse(A).csr())
    y = Vectors(np.zeros((3, N)))
    T.apply(x, y)
    ref = (G.conj().T @ (G @ np.ones((N, 3)))).T
    assert np.allclose(y.data(), ref, rtol=1e-12, atol=0)
    T.apply(x, x)
    assert np.array_equal(x.data(), y.data())
    return T, G


# ---------------------------------------------------------------- quality
def kaporin(M):
    ev = np.linalg.eigvalsh(M)
    assert ev[0] > 0
    return float(np.mean(ev) / np.exp(np.mean(np.log(ev))))


def quality():
    """FSAI minimises the Kaporin number of G A G^H over all G with the given pattern, and Jacobi scaling lies in
    that set."""
    from raleigh_amd.synthetic import fe_surrogate, lap3d_rows
    out = []
    for A in (sp.csr_matrix(fe_surrogate(grid=(7, 6, 5))), sp.csr_matrix(lap3d_rows(8, 8, 8, 1.0, 1.01, 1.02, 0, 512))):
        A = A.astype(np.float64)
        A.sort_indices()
        G, _ = built(A, bits=32)
        n = A.shape[0]
        d = hermitian_from_upper(A).toarray()
        g = G.toarray()
        s = 1 / np.sqrt(np.diag(d))
        kg, kj = kaporin(g @ d @ g.T), kaporin(d * s[:, None] * s[None, :])
        print('Kaporin number: FSAI %.6f, Jacobi %.6f (n = %d)' % (kg, kj, n))
        assert kg <= kj * (1 + 100 * n * unit(np.float64))
        out.append((kg, kj))
    return out


# ---------------------------------------------------------------- end to end
def end_to_end(device, as_tensor=True):
    import scipy.linalg
    from raleigh_amd.synthetic import fe_surrogate
    from raleigh_amd.interfaces import partial_hevp
    from raleigh_amd.algebra.hip.precond import ApproximateInverse
    from _device_operator_cases import TOL, _residual
    A = sp.csr_matrix(fe_surrogate(grid=(7, 6, 5))).astype(np.float64)
    A.sort_indices()
    which = 6
    exact = scipy.linalg.eigvalsh(hermitian_from_upper(A).toarray())[:which]
    a = csr_tensor(A, device) if as_tensor else A
    T = ApproximateInverse(a)
    np.random.seed(1)
    lmd, x, status = partial_hevp(a, T=T, which=which, tol=TOL, verb=-1)
    its = partial_hevp.last['iterations']
    np.random.seed(1)
    lmd_ref, x_ref, status_ref = partial_hevp(A, T=True, which=which, tol=TOL, verb=-1)
    assert status == 0 == status_ref
    print('iterations: %d with the approximate inverse, %d without a preconditioner' % (its, partial_hevp.last['iterations']))
    assert np.max(np.abs(lmd[:which] - exact)) <= 1e-10
    if as_tensor:
        import torch
        assert isinstance(x, torch.Tensor) and x.device.type == torch.device(device).type
        x = host(x)
    assert x.shape[0] == A.shape[0] and x.shape[1] >= which == len(exact)
    res, res_ref = _residual(A, None, lmd[:which], x[:, :which].astype(np.float64)), _residual(A, None, lmd_ref[:which], x_ref[:, :which])
    print('residual: approximate inverse %.3e, no preconditioner %.3e' % (res, res_ref))
    assert res <= 10 * res_ref
