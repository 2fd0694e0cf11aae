"""GPU tier: the sparse operator built on the device (rlh_csr_create_device) against the host build of the same
arrays (rlh_csr_create / rlh_csr_create_upper) through the raw C ABI -- with the same layout asked of both, the two
handles store every row's entries in the same order and run the same kernel, so every product must be equal bit for
bit --, its rejections, and SparseSymmetricMatrix / partial_hevp on torch.sparse_csr tensors (cases of
tests/_device_operator_cases.py)."""

import ctypes
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

import _device_operator_cases as cases

pytestmark = pytest.mark.gpu

_TYPES = {'s': np.float32, 'd': np.float64, 'c': np.complex64, 'z': np.complex128}
_LAYOUT = {0: 'sell', 1: 'well', 2: 'wide'}
VECTORS = (1, 3, 8, 33)
SENTINEL = 7.5


def _L():
    from raleigh_amd import _lib
    return _lib.lib()


def _check(rc):
    from raleigh_amd import _lib
    _lib.check(rc)


def _dev(a):
    """A device copy of a host array (kept alive by the returned buffer)."""
    from raleigh_amd.algebra.hip.memory import DeviceBuffer
    from raleigh_amd import _lib
    a = np.ascontiguousarray(a)
    buf = DeviceBuffer(max(a.nbytes, 16), zero=False)
    if a.nbytes:
        _check(_L().rlh_h2d(buf.ptr, _lib.host_ptr(a), a.nbytes))
    return buf


def _fetch(buf, count, dt):
    from raleigh_amd import _lib
    out = np.empty(count, dtype=dt)
    if count:
        _check(_L().rlh_d2h(_lib.host_ptr(out), buf.ptr, out.nbytes))
    return out


def _rand(rng, shape, dt):
    a = rng.standard_normal(shape)
    if np.dtype(dt).kind == 'c':
        a = a + 1j * rng.standard_normal(shape)
    return a.astype(dt)


def _from_rows(rows, shape, rng):
    """CSR with the given (sorted, distinct) columns per row and random real values (the tests cast them)."""
    indptr = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int64)
    indices = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows] + [np.zeros(0, dtype=np.int64)])
    return sp.csr_matrix((rng.standard_normal(indices.size), indices.astype(np.int32), indptr), shape=shape)


@functools.lru_cache(maxsize=None)
def _case(name):
    """The matrices of the comparison (fixed seed), real float64 values; see the module docstring of the issue's list:
    a  700 x 700: three blocks, the last partial; empty rows; a row of 19 entries (three chunks); in the second
       block two column clusters far apart (more than one window); a row whose only entry is the last column, which
       no other row references (a window at the far end, and the column of the non-finite test)
    b  5 x 5: narrower than one staging group
    c  513 x 513, two unknowns per node, 18 entries per row: the pairing rule applies; c1: one pair differs
    d  256 x 200 000, 20 random columns per row: the group set overflows -> sliced ELL
    e  3000 x 3000, 6 random columns per row: no locality -> sliced ELL by the 90 % rule"""
    rng = np.random.default_rng(8)
    if name == 'a':
        n = 700
        rows = []
        for i in range(n):
            band = {min(max(i + d, 0), n - 2) for d in (-9, -2, 0, 1, 5)}
            if 256 <= i < 512:
                band |= {40 + (i % 17), 41 + (i % 17)}          # a second cluster, columns 40 .. 57
            rows.append(sorted(band))
        for i in (3, 4, 300, 600, 698):
            rows[i] = []
        rows[130] = sorted(set(range(100, 157, 3)))             # 19 entries
        assert len(rows[130]) == 19
        rows[690] = [n - 1]
        assert sum(n - 1 in r for r in rows) == 1
        return _from_rows(rows, (n, n), rng)
    if name == 'b':
        return _from_rows([[0, 1, 4], [1], [], [0, 2, 3, 4], [4]], (5, 5), rng)
    if name in ('c', 'c1'):
        n, nodes = 513, 257
        rows = []
        for i in range(n):
            node = i // 2
            near = sorted({min(max(node + d, 0), nodes - 2) for d in range(-4, 5)})
            near = (near + [k for k in range(nodes - 1) if k not in near])[:9]
            rows.append(sorted(c for k in near for c in (2 * k, 2 * k + 1)))
        assert all(len(r) == 18 for r in rows) and all(rows[2 * q] == rows[2 * q + 1] for q in range(256))
        if name == 'c1':
            rows[203] = rows[203][:-1] + [rows[203][-1] + 2]
            assert rows[203] != rows[202] and len(set(rows[203])) == 18 and rows[203][-1] < n
        return _from_rows(rows, (n, n), rng)
    if name == 'd':
        return _from_rows([np.sort(rng.choice(200000, 20, replace=False)) for _ in range(256)], (256, 200000), rng)
    if name == 'e':
        return _from_rows([np.sort(rng.choice(3000, 6, replace=False)) for _ in range(3000)], (3000, 3000), rng)
    raise KeyError(name)


# (case, the layouts asked for (None: the build's own choice), the layout each must give)
PLAN = [('a', (None, 'wide', 'sell'), ('wide', 'wide', 'sell')), ('b', (None, 'wide', 'sell'), ('wide', 'wide', 'sell')),
        ('c', (None, 'sell'), ('wide', 'sell')), ('c1', (None, 'sell'), ('wide', 'sell')),
        ('d', (None, 'wide'), ('sell', 'sell')), ('e', (None,), ('sell',))]


def _typed(A, dt):
    """A's structure with values of type dt (complex: an imaginary part from the same generator)."""
    rng = np.random.default_rng(A.nnz)
    return sp.csr_matrix((_rand(rng, A.nnz, dt), A.indices, A.indptr), shape=A.shape)


class _Env:
    def __init__(self, fmt):
        self.fmt = fmt

    def __enter__(self):
        self.old = os.environ.pop('RLH_SPMM_FORMAT', None)
        if self.fmt is not None:
            os.environ['RLH_SPMM_FORMAT'] = self.fmt

    def __exit__(self, *a):
        os.environ.pop('RLH_SPMM_FORMAT', None)
        if self.old is not None:
            os.environ['RLH_SPMM_FORMAT'] = self.old


def _create_host(A, fmt, upper=False):
    from raleigh_amd import _lib
    h = ctypes.c_void_p()
    ip, ix, va = A.indptr.astype(np.int64), A.indices.astype(np.int32), np.ascontiguousarray(A.data)
    code = _lib.DTYPE_CODE[A.dtype.type]
    with _Env(fmt):
        if upper:
            _check(_L().rlh_csr_create_upper(ctypes.byref(h), code, A.shape[0], _lib.host_ptr(ip), _lib.host_ptr(ix),
                                             _lib.host_ptr(va)))
        else:
            _check(_L().rlh_csr_create(ctypes.byref(h), code, A.shape[0], A.shape[1], _lib.host_ptr(ip), _lib.host_ptr(ix),
                                       _lib.host_ptr(va)))
    return h


def _create_device(A, bits, fmt=None, mirror=0, indptr=None, indices=None, shape=None, keep=None):
    """(rc, handle) of rlh_csr_create_device on device copies of A's arrays (or of the given ones)."""
    from raleigh_amd import _lib
    it = {32: np.int32, 64: np.int64}.get(bits, np.int64)
    arrays = ((A.indptr if indptr is None else indptr).astype(it), (A.indices if indices is None else indices).astype(it),
              np.ascontiguousarray(A.data))
    bufs = [_dev(a) for a in arrays]
    h = ctypes.c_void_p(12345)
    shape = A.shape if shape is None else shape
    with _Env(fmt):
        rc = _L().rlh_csr_create_device(ctypes.byref(h), _lib.DTYPE_CODE[A.dtype.type], shape[0], shape[1], bits,
                                        bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, mirror)
    if keep is not None:
        keep.extend(zip(arrays, bufs))
    return rc, h


def _layout(h):
    lay, stored, ratio = ctypes.c_int(), ctypes.c_int64(), ctypes.c_double()
    _check(_L().rlh_csr_layout(h, ctypes.byref(lay), ctypes.byref(stored), ctypes.byref(ratio)))
    return _LAYOUT[lay.value]


def _product(h, shape, m, X, dt):
    ldy = shape[0] + 3
    y = _dev(np.full(ldy * m, SENTINEL, dtype=dt))
    _check(_L().rlh_spmm(h, m, X.ptr, shape[1], shape[1], None, 0, y.ptr, ldy))
    return _fetch(y, ldy * m, dt).reshape(m, ldy)


def _exact(A, x):
    """(A x in extended precision, sum_j |a_ij| |x_j|, row lengths): x is (m, n_cols), results (m, n_rows)."""
    wide = np.clongdouble if A.dtype.kind == 'c' else np.longdouble
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    prod = A.data.astype(wide)[None, :] * x.astype(wide)[:, A.indices]
    mag = np.abs(A.data).astype(np.float64)[None, :] * np.abs(x).astype(np.float64)[:, A.indices]
    out = np.zeros((x.shape[0], A.shape[0]), dtype=wide)
    tot = np.zeros((x.shape[0], A.shape[0]), dtype=np.float64)
    for j in range(x.shape[0]):
        np.add.at(out[j], rows, prod[j])
        np.add.at(tot[j], rows, mag[j])
    return out, tot, np.diff(A.indptr)


@pytest.mark.parametrize('bits', [32, 64])
@pytest.mark.parametrize('code', sorted(_TYPES))
@pytest.mark.parametrize('name,asked,expected', PLAN)
def test_device_build_equals_host_build(name, asked, expected, code, bits):
    dt = _TYPES[code]
    A = _typed(_case(name), dt)
    rng = np.random.default_rng(5)
    x = _rand(rng, (max(VECTORS), A.shape[1]), dt)
    X = _dev(x)
    unit = float(np.finfo(dt).eps) / 2
    exact, tot, length = _exact(A, x)
    for fmt, want in zip(asked, expected):
        kept = []
        rc, hd = _create_device(A, bits, fmt, keep=kept)
        _check(rc)
        hh = None
        try:
            assert _layout(hd) == want, (name, fmt)
            for arr, buf in kept:                                # (i) the caller's arrays are as they were
                assert np.array_equal(_fetch(buf, arr.size, arr.dtype), arr)
            nn = ctypes.c_int64()
            _check(_L().rlh_csr_info(hd, None, None, ctypes.byref(nn), None))
            assert nn.value == A.nnz
            hh = _create_host(A, want)
            assert _layout(hh) == want, (name, fmt)
            for m in VECTORS:
                got, ref = _product(hd, A.shape, m, X, dt), _product(hh, A.shape, m, X, dt)
                assert np.array_equal(got.view(np.uint8), ref.view(np.uint8)), (name, fmt, m)
                assert np.all(got[:, A.shape[0]:] == SENTINEL)
                if m == max(VECTORS):                          # every layout against the independent reference
                    err = np.abs(got[:, :A.shape[0]].astype(exact.dtype) - exact).astype(np.float64)
                    assert np.all(err <= (length[None, :] + 2) * unit * tot), (name, float(np.max(err / np.maximum(tot, 1e-300))))
        finally:
            _L().rlh_csr_destroy(hd)
            if hh is not None:
                _L().rlh_csr_destroy(hh)


def _bytes_and_stored(h):
    nb, lay, stored, ratio = ctypes.c_int64(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_double()
    _check(_L().rlh_csr_info(h, None, None, None, ctypes.byref(nb)))
    _check(_L().rlh_csr_layout(h, ctypes.byref(lay), ctypes.byref(stored), ctypes.byref(ratio)))
    return nb.value, stored.value


@pytest.mark.parametrize('code,paired', [('s', True), ('d', True), ('z', False)])
def test_pairing_rule_applies(code, paired):
    """(c) Equal products do not say whether rows were paired.  The handle's size does: a paired layout stores one
    16-byte piece of positions per row PAIR and chunk, so matrix c (every pair shares its columns) is smaller than
    c1 (one pair differs) by half the positions -- for real types, on the device build as on the host build."""
    size = {}
    for name in ('c', 'c1'):
        A = _typed(_case(name), _TYPES[code])
        rc, hd = _create_device(A, 32)
        _check(rc)
        hh = _create_host(A, 'wide')
        size[name] = (_bytes_and_stored(hd), _bytes_and_stored(hh))
        _L().rlh_csr_destroy(hd)
        _L().rlh_csr_destroy(hh)
    for k in (0, 1):                                            # device build, host build
        (small, stored), (large, stored1) = size['c'][k], size['c1'][k]
        assert stored == stored1
        half = (stored // (8 * 256) + 4) * 128 * 16             # positions of a paired layout (4 chunks of padding)
        if paired:
            assert large - small > 0.9 * half, (k, small, large)
        else:
            assert abs(large - small) < 0.1 * half, (k, small, large)


@pytest.mark.parametrize('code', sorted(_TYPES))
@pytest.mark.parametrize('fmt', ['wide', 'sell'])
def test_chebyshev_step_equals_host_build(code, fmt):
    dt = _TYPES[code]
    A = _typed(_case('a'), dt)
    n, m = A.shape[0], 5
    rng = np.random.default_rng(6)
    Y, B, p0 = _dev(_rand(rng, (m, n), dt)), _dev(_rand(rng, (m, n), dt)), _rand(rng, (m, n), dt)
    rc, hd = _create_device(A, 32, fmt)
    _check(rc)
    hh = _create_host(A, fmt)
    try:
        out = []
        for h in (hd, hh):
            P = _dev(p0)
            _check(_L().rlh_spmm_cheb(h, m, Y.ptr, n, n, None, 0, P.ptr, n, B.ptr, n, 0.75, -0.5, 1.25))
            out.append(_fetch(P, m * n, dt))
        assert np.array_equal(out[0].view(np.uint8), out[1].view(np.uint8))
        assert not np.array_equal(out[0], p0.ravel())
    finally:
        _L().rlh_csr_destroy(hd)
        _L().rlh_csr_destroy(hh)


@pytest.mark.parametrize('code', ['s', 'z'])
@pytest.mark.parametrize('fmt', ['wide', 'sell'])
def test_non_finite_input_stays_in_its_row(code, fmt):
    """(f) One Inf in a column that a single row references: exactly that row of y is non-finite and every other
    row is what it is for finite x (padding slots point at the row's own first entry, never at a foreign column)."""
    dt = _TYPES[code]
    A = _typed(_case('a'), dt)
    n, m = A.shape[0], 3
    x = _rand(np.random.default_rng(7), (m, n), dt)
    xi = x.copy()
    xi[:, n - 1] = np.inf
    rc, hd = _create_device(A, 64, fmt)
    _check(rc)
    try:
        fin, inf = _product(hd, A.shape, m, _dev(x), dt)[:, :n], _product(hd, A.shape, m, _dev(xi), dt)[:, :n]
        bad = ~np.isfinite(inf)
        assert np.all(bad[:, 690]) and bad.sum() == m
        keep = np.arange(n) != 690
        assert np.array_equal(np.ascontiguousarray(inf[:, keep]).view(np.uint8), np.ascontiguousarray(fin[:, keep]).view(np.uint8))
    finally:
        _L().rlh_csr_destroy(hd)


@pytest.mark.parametrize('code', ['s', 'd', 'z'])
def test_row_shard_parts(code):
    """A rectangular handle used as a row shard (rlh_spmm_part): 760 own columns, 240 halo columns.  Block 0 stays
    below column 300; block 1 references nothing past column 755, but its last 16-column group (752 .. 767) reaches
    over the own / halo boundary, so it STAGES halo columns and is not an interior block; block 2 references the
    halo.  Part 1 (with a halo block of NaN: it is not read) then writes block 0 alone, parts 1 and 2 together give
    part 0, and everything equals the host-built handle bit for bit."""
    dt = _TYPES[code]
    n, n_own, nc, m = 760, 760, 1000, 5
    rows = []
    for i in range(n):
        if i < 256:
            rows.append([i, i + 3, i + 40])
        elif i < 512:
            rows.append(sorted({i - 200, i} | ({755} if i % 5 == 0 else set())))
        else:
            rows.append([i - 300, i, 760 + (i * 7) % 240])
    A = _typed(_from_rows(rows, (n, nc), np.random.default_rng(12)), dt)
    x = _rand(np.random.default_rng(13), (m, nc), dt)
    X, H = _dev(np.ascontiguousarray(x[:, :n_own])), _dev(np.ascontiguousarray(x[:, n_own:]))
    Hnan = _dev(np.full((m, nc - n_own), np.nan, dtype=dt))
    ldy = n + 3

    def run(h, parts):
        y = _dev(np.full(ldy * m, SENTINEL, dtype=dt))
        out = []
        for part, halo in parts:
            _check(_L().rlh_spmm_part(h, part, m, X.ptr, n_own, n_own, halo.ptr, nc - n_own, y.ptr, ldy))
            out.append(_fetch(y, ldy * m, dt).reshape(m, ldy))
        return out

    rc, hd = _create_device(A, 32, 'wide')
    _check(rc)
    hh = _create_host(A, 'wide')
    try:
        assert _layout(hd) == _layout(hh) == 'wide'
        (whole,), (first, both) = run(hd, [(0, H)]), run(hd, [(1, Hnan), (2, H)])
        assert np.all(first[:, :256] != SENTINEL) and np.all(first[:, 256:] == SENTINEL)
        assert np.array_equal(both.view(np.uint8), whole.view(np.uint8))
        (whole_h,), (_, both_h) = run(hh, [(0, H)]), run(hh, [(1, Hnan), (2, H)])
        assert np.array_equal(whole.view(np.uint8), whole_h.view(np.uint8))
        assert np.array_equal(both.view(np.uint8), both_h.view(np.uint8))
        exact, tot, length = _exact(A, x)
        err = np.abs(whole[:, :n].astype(exact.dtype) - exact).astype(np.float64)
        assert np.all(err <= (length[None, :] + 2) * (float(np.finfo(dt).eps) / 2) * tot)
        assert np.all(whole[:, n:] == SENTINEL)
    finally:
        _L().rlh_csr_destroy(hd)
        _L().rlh_csr_destroy(hh)


def _hermitian_with_garbage_below():
    H = cases.hermitian()                                       # 300 rows, complex128, both triangles
    G = H.copy()
    rows = np.repeat(np.arange(H.shape[0]), np.diff(H.indptr))
    below = G.indices < rows
    G.data[below] = _rand(np.random.default_rng(9), int(below.sum()), np.complex128)
    return H, G, rows


@pytest.mark.parametrize('bits', [32, 64])
@pytest.mark.parametrize('fmt', ['wide', 'sell'])
def test_mirror_upper(fmt, bits):
    """(g) The Hermitian operator defined by the upper triangle: garbage below the diagonal changes nothing, and the
    product is that of rlh_csr_create_upper on the same arrays."""
    H, G, _ = _hermitian_with_garbage_below()
    n, dt = H.shape[0], np.complex128
    x = _rand(np.random.default_rng(10), (max(VECTORS), n), dt)
    X = _dev(x)
    rc, hd = _create_device(G, bits, fmt, mirror=1)
    _check(rc)
    hh = _create_host(G, fmt, upper=True)
    try:
        assert _layout(hd) == _layout(hh) == fmt
        for m in VECTORS:
            got, ref = _product(hd, H.shape, m, X, dt), _product(hh, H.shape, m, X, dt)
            assert np.array_equal(got.view(np.uint8), ref.view(np.uint8)), m
        exact, tot, length = _exact(H, x)
        err = np.abs(got[:, :n].astype(exact.dtype) - exact).astype(np.float64)
        assert np.all(err <= (length[None, :] + 2) * (float(np.finfo(dt).eps) / 2) * tot)
    finally:
        _L().rlh_csr_destroy(hd)
        _L().rlh_csr_destroy(hh)


def _last_error():
    return _L().rlh_last_error().decode()


def _without(A, k):
    """A with its stored entry k removed."""
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    keep = np.arange(A.nnz) != k
    return sp.csr_matrix((A.data[keep], (rows[keep], A.indices[keep])), shape=A.shape), int(rows[k]), int(A.indices[k])


def test_mirror_upper_needs_a_symmetric_structure():
    H, G, rows = _hermitian_with_garbage_below()
    lower = int(np.flatnonzero(G.indices < rows)[40])
    upper = int(np.flatnonzero(G.indices > rows)[77])
    for k in (lower, upper):
        B, i, j = _without(G, k)
        B.sort_indices()
        rc, h = _create_device(B, 32, mirror=1)
        assert rc != 0 and not h.value
        msg = _last_error()
        # the entry left without its partner is (j, i): both it and the missing one are named
        assert 'not symmetric' in msg and '(%d, %d)' % (j, i) in msg and '(%d, %d)' % (i, j) in msg, msg
    rc, h = _create_device(G, 32, mirror=1)
    _check(rc)
    _L().rlh_csr_destroy(h)


def test_malformed_input_is_refused():
    """(h) Every malformed input fails with its message and a null handle; a good build straight afterwards works."""
    A = _typed(_case('a'), np.float64)
    ip, ix = A.indptr.astype(np.int64), A.indices.astype(np.int64)
    row = 100
    assert ip[row + 1] - ip[row] >= 3
    k = int(ip[row]) + 1                                          # an inner entry of row 100

    def changed(a, i, v):
        b = a.copy()
        b[i] = v
        return b

    swapped = ix.copy()
    swapped[k], swapped[k + 1] = ix[k + 1], ix[k]
    bad = [(dict(indptr=changed(ip, 50, ip[49] - 1 if ip[49] > 0 else 0)), 'indptr decreases at row 49'),
           (dict(indptr=changed(ip, 0, 1)), 'indptr[0] must be 0'),
           (dict(indices=changed(ix, k, A.shape[1])), 'out of range in row %d' % row),
           (dict(indices=changed(ix, int(ip[row]), -1)), 'out of range in row %d' % row),
           (dict(indices=changed(ix, k, ix[k - 1])), 'columns of row %d must ascend' % row),
           (dict(indices=swapped), 'columns of row %d must ascend' % row),
           (dict(bits=16), 'index_bits must be 32 or 64'),
           (dict(mirror=1, shape=(A.shape[0], A.shape[1] + 1)), 'square'),
           (dict(fmt='well'), 'RLH_SPMM_FORMAT=well')]
    assert ip[50] > ip[49] - 1 and ip[49] > 0
    for kw, text in bad:
        kw = dict(kw)
        bits = kw.pop('bits', 64)
        rc, h = _create_device(A, bits, **kw)
        assert rc != 0 and not h.value, text
        assert text in _last_error(), (text, _last_error())
        rc, h = _create_device(A, 64)
        _check(rc)
        assert _layout(h) == 'wide'
        _L().rlh_csr_destroy(h)


# ---- SparseSymmetricMatrix and partial_hevp on tensors (tests/_device_operator_cases.py)

@pytest.fixture
def device():
    torch = pytest.importorskip('torch')
    assert torch.cuda.is_available()
    return 'cuda'


def test_apply_matches(device, monkeypatch):
    cases.apply_matches(device, monkeypatch)


def test_odd_storage(device):
    cases.odd_storage(device)


def test_tensor_on_another_gpu(monkeypatch):
    cases.other_gpu(monkeypatch)


def test_hevp_plain(device):
    cases.hevp_plain(device)


def test_hevp_chebyshev(device):
    cases.hevp_chebyshev(device)


def test_hevp_generalized(device):
    cases.hevp_generalized(device)


def test_hevp_iterative(device):
    cases.hevp_iterative(device)


def test_direct_mode(device):
    cases.direct_mode(device)


def test_rejections(device):
    import torch
    cases.rejections(device, 'cuda:1' if torch.cuda.device_count() > 1 else None)


def test_structure_must_be_symmetric(device):
    cases.structure_must_be_symmetric(device)


def test_cpu_tensor_takes_host_path():
    pytest.importorskip('torch')
    cases.cpu_tensor()
