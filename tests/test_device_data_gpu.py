"""GPU tier: data already in device memory.  The sparse operator built on the device (rlh_spd_create_device) against
the host build of the same matrix through the raw C ABI -- the two handles hold the same arrays, so every product
must be equal bit for bit --, its rejections and side values; the 8-bit and the dense operators over device buffers
and torch tensors; PCA and truncated SVD of torch tensors (cases of tests/_device_data_cases.py)."""

import ctypes
import functools
import os

import numpy as np
import pytest

import _device_data_cases as cases

pytestmark = pytest.mark.gpu

_TYPES = {'s': np.float32, 'd': np.float64, 'c': np.complex64, 'z': np.complex128}
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


@functools.lru_cache(maxsize=None)
def _matrices(code):
    return cases.build_matrices(_TYPES[code])


def _create_host(A, dt):
    from raleigh_amd import _lib
    h = ctypes.c_void_p()
    ip, ix, va = A.indptr.astype(np.int64), A.indices.astype(np.int32), np.ascontiguousarray(A.data, dtype=dt)
    _check(_L().rlh_spd_create(ctypes.byref(h), _lib.DTYPE_CODE[dt], A.shape[0], A.shape[1], _lib.host_ptr(ip),
                               _lib.host_ptr(ix), _lib.host_ptr(va)))
    return h


def _create_device(A, dt, bits, cap=None, indptr=None, indices=None):
    """(rc, handle) of rlh_spd_create_device on device copies of A's arrays (or of the given ones)."""
    from raleigh_amd import _lib
    it = np.int32 if bits == 32 else np.int64
    ip = _dev((A.indptr if indptr is None else indptr).astype(it))
    ix = _dev((A.indices if indices is None else indices).astype(it))
    va = _dev(np.ascontiguousarray(A.data, dtype=dt))
    h = ctypes.c_void_p()
    old = os.environ.pop('RLH_SPD_TABLE_BYTES', None)
    if cap is not None:
        os.environ['RLH_SPD_TABLE_BYTES'] = str(cap)
    try:
        rc = _L().rlh_spd_create_device(ctypes.byref(h), _lib.DTYPE_CODE[dt], A.shape[0], A.shape[1], bits, ip.ptr, ix.ptr,
                                        va.ptr)
    finally:
        os.environ.pop('RLH_SPD_TABLE_BYTES', None)
        if old is not None:
            os.environ['RLH_SPD_TABLE_BYTES'] = old
    return rc, h


def _products(h, A, dt, X, U, Cf):
    """Every product of the comparison, guard rows included: m in {1, 5, 33, 65}, both transp, with and without the
    rank-one term, into blocks of leading dimension rows + 3 prefilled with a sentinel."""
    out = []
    for transp in (0, 1):
        nx, ny = (A.shape[0], A.shape[1]) if transp else (A.shape[1], A.shape[0])
        ldy = ny + 3
        for m in (1, 5, 33, 65):
            for r1 in (False, True):
                y = _dev(np.full(ldy * m, SENTINEL, dtype=dt))
                _check(_L().rlh_spd_apply(h, transp, m, X[transp].ptr, max(nx, 1), y.ptr, ldy,
                                          U[transp].ptr if r1 else None, Cf.ptr if r1 else None))
                out.append(_fetch(y, ldy * m, dt))
    return out


@pytest.mark.parametrize('bits', [32, 64])
@pytest.mark.parametrize('code', sorted(_TYPES))
def test_device_build_equals_host_build(code, bits):
    dt = _TYPES[code]
    rng = np.random.default_rng(21)
    for name, A, cap in _matrices(code):
        hh = _create_host(A, dt)
        rc, hd = _create_device(A, dt, bits, cap)
        _check(rc)
        assert hd.value
        try:
            nh, nd = ctypes.c_int64(), ctypes.c_int64()
            _check(_L().rlh_spd_info(hh, None, None, ctypes.byref(nh), None))
            _check(_L().rlh_spd_info(hd, None, None, ctypes.byref(nd), None))
            assert nh.value == nd.value == A.nnz, name
            X = [_dev(_rand(rng, (65, max(n, 1)), dt)) for n in (A.shape[1], A.shape[0])]
            U = [_dev(_rand(rng, (max(n, 1),), dt)) for n in A.shape]
            Cf = _dev(_rand(rng, (65,), dt))
            ref, got = _products(hh, A, dt, X, U, Cf), _products(hd, A, dt, X, U, Cf)
            for k, (r, g) in enumerate(zip(ref, got)):
                assert np.array_equal(r.view(np.uint8), g.view(np.uint8)), (name, k)
            sec = ctypes.c_double(-1.0)
            _check(_L().rlh_spd_stats(hd, None, ctypes.byref(sec)))
            assert sec.value >= 0.0
        finally:
            _L().rlh_spd_destroy(hh)
            _L().rlh_spd_destroy(hd)


def test_products_are_right():
    """(the comparison above says the two builds agree; this one, that they agree on the right product)"""
    dt = np.float64
    (_, A, _), = [c for c in _matrices('d') if c[0] == 'powerlaw']
    rc, h = _create_device(A, dt, 32)
    _check(rc)
    rng = np.random.default_rng(2)
    for transp in (0, 1):
        nx, ny = (A.shape[0], A.shape[1]) if transp else (A.shape[1], A.shape[0])
        x = _rand(rng, (5, nx), dt)
        y = _dev(np.zeros(5 * ny))
        xd = _dev(x)
        _check(_L().rlh_spd_apply(h, transp, 5, xd.ptr, nx, y.ptr, ny, None, None))
        ref = ((A.T if transp else A) @ x.T).T
        got = _fetch(y, 5 * ny, dt).reshape(5, ny)
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    _L().rlh_spd_destroy(h)


def test_rejections_of_the_device_build():
    from raleigh_amd import _lib
    dt = np.float64
    (_, A, _), = [c for c in _matrices('d') if c[0] == 'nnz8191']
    ip, ix = A.indptr.astype(np.int64), A.indices.astype(np.int64)
    r = int(np.flatnonzero(np.diff(ip) >= 2)[0])           # a row with two entries at least
    k = int(ip[r])

    def changed(a, pos, val):
        b = a.copy()
        b[pos] = val
        return b

    def swapped(a, i, j):
        b = a.copy()
        b[i], b[j] = a[j], a[i]
        return b

    name = 'rlh_spd_create_device: '
    last = "indptr's last entry (%d) is not the number of stored entries" % (ip[-1] + 10 ** 7)
    order = 'the columns of a row must ascend strictly (no duplicates): entry %d' % (k + 1)
    bad = {'indptr[0] = 1': (dict(indptr=changed(ip, 0, 1)), 'indptr[0] must be 0'),
           'indptr decreasing': (dict(indptr=changed(ip, 5, ip[6] + 1)), 'indptr decreases at row 5'),
           'wrong last entry': (dict(indptr=changed(ip, -1, ip[-1] + 10 ** 7)), last),
           'column = n_cols': (dict(indices=changed(ix, k, A.shape[1])), 'column index out of range at entry %d' % k),
           'negative column': (dict(indices=changed(ix, k, -1)), 'column index out of range at entry %d' % k),
           'equal columns': (dict(indices=changed(ix, k + 1, ix[k])), order),
           'descending columns': (dict(indices=swapped(ix, k, k + 1)), order)}
    for bits in (32, 64):
        for what, (kw, text) in bad.items():
            rc, h = _create_device(A, dt, bits, **kw)
            msg = _lib.library().rlh_last_error().decode()
            assert rc != 0 and not h.value, (what, bits)
            assert msg.startswith(name + text) and (msg == name + text or what == 'wrong last entry'), (what, msg)
        rc, h = _create_device(A, dt, bits)                 # a valid create straight afterwards
        _check(rc)
        x = np.ones((1, A.shape[1]))
        y = _dev(np.zeros(A.shape[0]))
        xd = _dev(x)
        _check(_L().rlh_spd_apply(h, 0, 1, xd.ptr, A.shape[1], y.ptr, A.shape[0], None, None))
        ref = A @ np.ones(A.shape[1])
        assert np.abs(_fetch(y, A.shape[0], dt) - ref).max() <= 1e-12 * np.abs(ref).max()
        _L().rlh_spd_destroy(h)


@pytest.mark.parametrize('code', sorted(_TYPES))
def test_row_sumsq_and_absmax(code):
    """Against the float64 NumPy values SparseMatrix.__init__ forms on the host: equal bit for bit for real data
    (sequential float64 sums in entry order on both sides), within 4 ulp of float64 for complex data (the modulus is
    formed differently).  For complex64 numpy.abs rounds the modulus to float32 before it is squared; the device follows
    that computation step by step in float32 (every step correctly rounded on both sides), so those values agree too
    (and likewise in float64 for complex128).  The largest distance of each complex matrix is printed."""
    dt = _TYPES[code]
    for name, A, cap in _matrices(code):
        if cap is not None:
            continue
        rc, h = _create_device(A, dt, 64)
        _check(rc)
        rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
        ref = np.bincount(rows, weights=np.abs(A.data).astype(np.float64) ** 2, minlength=A.shape[0])
        if A.nnz == 0:
            amax = 0.0
        elif np.dtype(dt).kind == 'c':
            amax = float(max(np.abs(A.data.real).max(), np.abs(A.data.imag).max()))
        else:
            amax = float(np.abs(A.data).max())
        got = np.full(A.shape[0], -1.0)
        out = ctypes.c_double(-1.0)
        from raleigh_amd import _lib
        _check(_L().rlh_spd_row_sumsq(h, _lib.host_ptr(got)))
        _check(_L().rlh_spd_absmax(h, ctypes.byref(out)))
        _L().rlh_spd_destroy(h)
        assert out.value == amax, name
        if np.dtype(dt).kind == 'c':
            worst = np.max(np.abs(got - ref) / np.spacing(ref)) if A.shape[0] and A.nnz else 0.0
            print('%s %s: row_sumsq differs from the host values by at most %.2f ulp' % (code, name, worst))
            assert np.all(np.abs(got - ref) <= 4 * np.spacing(ref)), (name, worst)
        else:
            assert np.array_equal(got, ref), name


def test_sparse_matrix_side_values_from_the_device():
    import torch
    from raleigh_amd.algebra.hip import SparseMatrix
    (_, A, _), = [c for c in _matrices('s') if c[0] == 'powerlaw']
    a, b = SparseMatrix(cases.csr_tensor(A, 'cuda', np.int32)), SparseMatrix(A)
    assert np.array_equal(a.dots(), b.dots()) and a.absmax() == b.absmax() and a.nnz() == b.nnz() == A.nnz
    assert a.shape() == b.shape() and a.data_type() == np.float32 and a.transpose_seconds() >= 0
    with pytest.raises(ValueError, match='canonical'):      # columns out of order: torch builds it, the library refuses
        SparseMatrix(torch.sparse_csr_tensor(torch.tensor([0, 2]), torch.tensor([1, 0]), torch.tensor([1.0, 2.0]),
                                             size=(1, 2)).to('cuda'))


# ---------------------------------------------------------------- 8-bit data

def _byte_products(h, M, N, X, U, Cf):
    out = []
    for transp in (0, 1):
        nx, ny = (M, N) if transp else (N, M)
        ldy = ny + 3
        for r1 in (False, True):
            y = _dev(np.full(ldy * 5, SENTINEL, dtype=np.float32))
            _check(_L().rlh_bytes_apply(h, transp, 5, X[transp].ptr, nx, y.ptr, ldy, U[transp].ptr if r1 else None,
                                        Cf.ptr if r1 else None))
            out.append(_fetch(y, ldy * 5, np.float32))
    return out


@pytest.mark.parametrize('dt', [np.uint8, np.int8])
def test_bytes_device_create_equals_host_create(dt):
    from raleigh_amd import _lib
    rng = np.random.default_rng(8)
    M = 37
    info = np.iinfo(dt)
    # (N, row stride, column the view starts at): contiguous, and views of a 37 x 64 buffer
    for N, stride, c0 in ((1, 1, 0), (15, 15, 0), (16, 16, 0), (17, 17, 0), (48, 48, 0), (48, 64, 0), (48, 64, 5), (32, 64, 16)):
        base = rng.integers(info.min, int(info.max) + 1, size=(M, stride)).astype(dt)
        view = base[:, c0:c0 + N]
        d_base = _dev(base)
        hh, hd = ctypes.c_void_p(), ctypes.c_void_p()
        _check(_L().rlh_bytes_create(ctypes.byref(hh), 1 if dt == np.int8 else 0, M, N, ctypes.c_void_p(view.ctypes.data), stride))
        _check(_L().rlh_bytes_create_device(ctypes.byref(hd), 1 if dt == np.int8 else 0, M, N, ctypes.c_void_p(d_base.ptr + c0),
                                            stride))
        X = [_dev(_rand(rng, (5, n), np.float32)) for n in (N, M)]
        U = [_dev(_rand(rng, (n,), np.float32)) for n in (M, N)]
        Cf = _dev(_rand(rng, (5,), np.float32))
        for r, g in zip(_byte_products(hh, M, N, X, U, Cf), _byte_products(hd, M, N, X, U, Cf)):
            assert np.array_equal(r.view(np.uint8), g.view(np.uint8)), (N, stride, c0)
        sq_h, sq_d = np.zeros(M), np.zeros(M)
        _check(_L().rlh_bytes_row_sumsq(hh, _lib.host_ptr(sq_h)))
        _check(_L().rlh_bytes_row_sumsq(hd, _lib.host_ptr(sq_d)))
        assert np.array_equal(sq_d, sq_h) and np.array_equal(sq_h, (view.astype(np.int64) ** 2).sum(axis=1).astype(np.float64))
        mx_h, mx_d = ctypes.c_double(), ctypes.c_double()
        _check(_L().rlh_bytes_absmax(hh, ctypes.byref(mx_h)))
        _check(_L().rlh_bytes_absmax(hd, ctypes.byref(mx_d)))
        assert mx_h.value == mx_d.value == float(np.abs(view.astype(np.int64)).max())
        nb, nw = ctypes.c_int64(), ctypes.c_int64()
        _check(_L().rlh_bytes_info(hd, None, None, ctypes.byref(nb), ctypes.byref(nw)))
        borrowed = N % 16 == 0 and stride % 16 == 0 and c0 % 16 == 0
        assert (nb.value == nw.value) == borrowed, (N, stride, c0)         # a borrowed matrix counts only the workspace
        assert np.array_equal(_fetch(d_base, base.size, dt).reshape(base.shape), base)
        _L().rlh_bytes_destroy(hh)
        _L().rlh_bytes_destroy(hd)


def test_bytes_tensor_borrowed():
    import torch
    from raleigh_amd.algebra.hip import ByteMatrix, Vectors
    rng = np.random.default_rng(9)
    A = rng.integers(0, 256, size=(37, 48)).astype(np.uint8)
    T = torch.from_numpy(A).to('cuda')
    assert T.data_ptr() % 16 == 0
    keep = T.clone()
    op, ref = ByteMatrix(T), ByteMatrix(A)
    x = Vectors(_rand(rng, (5, 48), np.float32))
    y, z = Vectors(37, 5, np.float32), Vectors(37, 5, np.float32)
    op.apply(x, y)
    ref.apply(x, z)
    assert np.array_equal(y.data(), z.data())
    assert op.device_bytes() == op.workspace_bytes() and ref.device_bytes() > ref.workspace_bytes()
    assert np.array_equal(op.dots(), ref.dots()) and op.absmax() == ref.absmax()
    assert torch.equal(T, keep)


# ---------------------------------------------------------------- dense data

def _dense_layouts(A, device):
    """(name, tensor of A's values, borrowed).  M x N = 37 x 64."""
    import torch
    T = torch.from_numpy(A).to(device)
    wide = torch.zeros((37, 80), dtype=T.dtype, device=device)
    wide[:, :64] = T
    shifted = torch.zeros((37, 80), dtype=T.dtype, device=device)
    shifted[:, 1:65] = T
    tall = torch.zeros((64, 48), dtype=T.dtype, device=device)
    tall[:, :37] = T.T
    return [('contiguous', T, True), ('row slice of 37 x 80', wide[:, :64], True), ('from column 1', shifted[:, 1:65], False),
            # leading dimension 37: a multiple of 16 bytes for complex128 alone
            ('transposed 64 x 37', T.T.contiguous().T, (37 * T.element_size()) % 16 == 0),
            ('transposed slice of 64 x 48', tall[:, :37].T, True)]


@pytest.mark.parametrize('code', sorted(_TYPES))
def test_dense_matrix_from_tensor(code):
    import torch
    from raleigh_amd.algebra.hip import Matrix, Vectors
    from raleigh_amd.algebra.hip.memory import DeviceBuffer
    dt = _TYPES[code]
    rng = np.random.default_rng(4)
    A = _rand(rng, (37, 64), dt)
    layouts = _dense_layouts(A, 'cuda')
    A61 = np.ascontiguousarray(A[:, :61])
    # (61 elements are a multiple of 16 bytes for complex128 alone)
    layouts.append(('N = 61', torch.from_numpy(A61).to('cuda'), (61 * A61.itemsize) % 16 == 0))
    c = _dev(_rand(rng, (5,), dt))
    for name, T, borrowed in layouts:
        H = A61 if name == 'N = 61' else (np.asfortranarray(A) if name.startswith('transposed') else A)
        keep = T.clone()
        op, ref = Matrix(T), Matrix(H)
        assert op.borrowed() == borrowed, name
        assert isinstance(op.matrix_data(), DeviceBuffer) != borrowed, name
        assert op.shape() == ref.shape() == H.shape
        for transp in (False, True):
            nx, ny = (H.shape[0], H.shape[1]) if transp else (H.shape[1], H.shape[0])
            x = Vectors(_rand(rng, (5, nx), dt))
            u = Vectors(_rand(rng, (1, ny), dt))
            for r1 in (False, True):
                y, z = Vectors(ny, 5, dt), Vectors(ny, 5, dt)
                op.apply_r1(x, y, transp, u if r1 else None, c.ptr if r1 else None)
                ref.apply_r1(x, z, transp, u if r1 else None, c.ptr if r1 else None)
                assert np.array_equal(y.data().view(np.uint8), z.data().view(np.uint8)), (name, transp, r1)
        assert np.array_equal(op.dots(), ref.dots()) and op.absmax() == ref.absmax(), name
        assert torch.equal(T, keep), name


# ---------------------------------------------------------------- interfaces

@pytest.mark.parametrize('name', cases.NAMES)
def test_interfaces_match(name):
    cases.interfaces_match(name, 'cuda')


def test_pca_have():
    cases.pca_have('cuda')


def test_rejections():
    import torch
    cases.rejections('cuda', 'cuda:1' if torch.cuda.device_count() > 1 else None)


def test_grad_and_conj():
    cases.grad_and_conj('cuda')


def test_cpu_tensor_takes_host_path():
    cases.cpu_tensor_takes_host_path()
