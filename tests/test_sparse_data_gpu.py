"""GPU tier: the general sparse data operator (rlh_spd_*, hip.SparseMatrix) against SciPy on the host, its
determinism and memory, and truncated SVD / PCA of sparse data -- at a size whose dense form could not be held
anywhere -- through librlhip.so."""

import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import _sparse_data_cases as cases

pytestmark = pytest.mark.gpu

_TYPES = [np.float32, np.float64, np.complex64, np.complex128]


def _rtol(dt):
    return 1e-5 if dt in (np.float32, np.complex64) else 1e-13


def _rand(rng, shape, dt):
    a = rng.standard_normal(shape)
    if np.dtype(dt).kind == 'c':
        a = a + 1j * rng.standard_normal(shape)
    return a.astype(dt)


def _shapes(dt):
    """(name, csr): empty rows and columns, a row holding every column, a column holding every row, N < 64,
    a power-law matrix."""
    from raleigh_amd.synthetic import sparse_data
    rng = np.random.default_rng(7)
    out = []
    A = sp.random(300, 200, density=0.05, format='lil', random_state=1, dtype=np.float64)
    A[10:20, :] = 0
    A[:, 50:70] = 0
    A[5, :] = rng.standard_normal(200)           # one row with all N columns
    A[:, 123] = rng.standard_normal((300, 1))    # one column with all M rows
    A = sp.csr_matrix(A)
    if np.dtype(dt).kind == 'c':
        A = A + 1j * sp.csr_matrix((rng.standard_normal(A.nnz), A.indices, A.indptr), shape=A.shape)
    out.append(('mixed', sp.csr_matrix(A, dtype=dt)))
    out.append(('narrow', sparse_data(500, 37, 5, 'uniform', dt, 2)))
    out.append(('powerlaw', sparse_data(3000, 700, 20, 'powerlaw', dt, 3)))
    out.append(('empty', sp.csr_matrix((40, 30), dtype=dt)))
    return out


def _apply(op, A, x, transp, window, u=None, c=None):
    """y = Op(A) x (- u c^T) through the device operator on a window (offset, padded ld) of bigger blocks."""
    from raleigh_amd.algebra.hip import Vectors
    from raleigh_amd.algebra.hip.memory import DeviceBuffer
    from raleigh_amd import _lib
    m = x.shape[0]
    ny = A.shape[1] if transp else A.shape[0]
    off = 3 if window else 0
    xs = np.zeros((m + 2 * off, x.shape[1]), dtype=x.dtype)
    xs[off:off + m] = x
    X = Vectors(xs)
    X.select(m, off)
    Y = Vectors(ny, m + 2 * off, x.dtype)
    Y.select(m, off)
    U = cb = None
    if c is not None:
        cb = DeviceBuffer(max(c.nbytes, 16))
        cc = np.ascontiguousarray(c)
        _lib.check(_lib.lib().rlh_h2d(cb.ptr, _lib.host_ptr(cc), cc.nbytes))
        if u is not None:
            U = Vectors(u[None, :])
    op.apply_r1(X, Y, transp, U, None if cb is None else cb.ptr)
    return Y.data()


def _check(y, ref, dt):
    err = np.linalg.norm(y - ref, axis=1)
    nrm = np.maximum(np.linalg.norm(ref, axis=1), np.finfo(np.float64).tiny)
    assert np.all(err <= _rtol(dt) * nrm + (0 if np.any(ref) else 0)), (err / nrm).max()


@pytest.mark.parametrize('dt', _TYPES)
def test_operator_parity(dt):
    from raleigh_amd.algebra.hip import SparseMatrix
    rng = np.random.default_rng(11)
    for name, A in _shapes(dt):
        op = SparseMatrix(A)
        Ad = A.astype(np.complex128 if np.dtype(dt).kind == 'c' else np.float64)
        for m in (1, 7, 64, 130):
            for transp in (False, True):
                nx, ny = (A.shape[0], A.shape[1]) if transp else (A.shape[1], A.shape[0])
                x = _rand(rng, (m, nx), dt)
                ref = (Ad.conj().T @ x.T.astype(Ad.dtype)).T if transp else (Ad @ x.T.astype(Ad.dtype)).T
                _check(_apply(op, A, x, transp, window=(m == 7)), ref, dt)
                c = _rand(rng, (m,), dt)
                u = _rand(rng, (ny,), dt)
                _check(_apply(op, A, x, transp, True, u, c), ref - c[:, None] * u[None, :], dt)
                _check(_apply(op, A, x, transp, False, None, c), ref - c[:, None], dt)


@pytest.mark.parametrize('dt', [np.float32, np.complex128])
def test_determinism(dt):
    from raleigh_amd.algebra.hip import SparseMatrix
    from raleigh_amd.synthetic import sparse_data
    A = sparse_data(20000, 3000, 30, 'powerlaw', dt, 5)
    rng = np.random.default_rng(1)
    op1, op2 = SparseMatrix(A), SparseMatrix(A)
    for transp in (False, True):
        x = _rand(rng, (64, A.shape[0] if transp else A.shape[1]), dt)
        y1 = _apply(op1, A, x, transp, False)
        y2 = _apply(op1, A, x, transp, False)
        y3 = _apply(op2, A, x, transp, False)
        assert np.array_equal(y1.view(np.uint8), y2.view(np.uint8))
        assert np.array_equal(y1.view(np.uint8), y3.view(np.uint8))


@pytest.mark.parametrize('dt', _TYPES)
def test_no_densification(dt):
    from raleigh_amd.algebra.hip import SparseMatrix
    from raleigh_amd.synthetic import sparse_data
    A = sparse_data(5000, 2000, 15, 'powerlaw', dt, 9)
    op = SparseMatrix(A)
    rng = np.random.default_rng(2)
    for transp in (False, True):
        _apply(op, A, _rand(rng, (130, A.shape[0] if transp else A.shape[1]), dt), transp, False)
    M, N = A.shape
    es = np.dtype(dt).itemsize
    assert op.device_bytes() <= 2 * A.nnz * (es + 4) + 16 * (M + N + 2) + op.workspace_bytes()
    assert op.workspace_bytes() < M * N * es
    assert op.transpose_seconds() >= 0


def test_known_answers_beyond_dense_size():
    """A 2e6 x 2.2e5 fp64 matrix (3.5 TB dense): sigma against the exact union of the blocks' singular values."""
    from raleigh_amd.interfaces import truncated_svd
    from raleigh_amd.synthetic import block_diagonal_data
    A, exact = block_diagonal_data([(2, 20000, 1), (20000, 2, 1), (40, 4, 49450)], np.float64, seed=4)
    assert A.shape[0] * A.shape[1] * 8 > 3e12
    u, s, vt = truncated_svd(A, nsv=20)
    assert len(s) >= 20
    assert np.max(np.abs(s[:20] - exact[:20]) / exact[:20]) <= 1e-10
    k = len(s)
    assert np.abs(u.T @ u - np.eye(k)).max() <= 1e-12
    assert np.abs(vt @ vt.T - np.eye(k)).max() <= 1e-12
    assert np.linalg.norm(A @ vt.T - u * s) <= 1e-8 * s[0]


def test_pca_powerlaw_moderate():
    from raleigh_amd.interfaces import pca
    from raleigh_amd.interfaces.pca import pca_error
    from raleigh_amd.synthetic import sparse_data
    A = sparse_data(20000, 5000, 40, 'powerlaw', np.float64, 6)
    D = A.toarray()
    mean, trans, comps = pca(A, npc=10, svtol=1e-12)
    sig = pca.last['sigma']
    Ds = D - D.mean(axis=0)
    lam = np.linalg.eigvalsh(Ds.T @ Ds)[::-1][:10]
    exact = np.sqrt(lam)
    assert np.max(np.abs(sig[:10] - exact) / exact) <= 1e-10
    dmean, dtrans, dcomps = pca(D, npc=10, svtol=1e-12)
    assert np.allclose(pca_error(D, mean, trans, comps), pca_error(D, dmean, dtrans, dcomps), rtol=1e-6, atol=0)


@pytest.mark.parametrize('dt', [np.float32, np.float64])
def test_truncated_svd_matches_dense(dt):
    cases.truncated_svd_matches_dense(dt)


def test_truncated_svd_complex():
    cases.truncated_svd_matches_dense(np.complex128)


def test_truncated_svd_norms():
    cases.truncated_svd_norms()


def test_pca_matches_dense():
    cases.pca_matches_dense()


def test_pca_have_matches_dense():
    cases.pca_have_matches_dense()


def test_pca_batches_match_dense():
    cases.pca_batches_match_dense()


def test_refusals():
    cases.refusals()
