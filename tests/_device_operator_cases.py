"""Sparse eigenproblems whose matrix is a torch.sparse_csr tensor, shared by the CPU tier (tests/fake_device_operator.py,
where CPU tensors stand for device tensors) and the GPU tier: SparseSymmetricMatrix and partial_hevp on a tensor
against the same call on the SciPy matrix, with the same start vectors (numpy.random.seed before each)."""

import numpy as np
import pytest
import scipy.sparse as sp

from _device_data_cases import csr_tensor, host

GRID = (8, 8, 8, 1.0, 1.01, 1.02)
N = 512
WHICH = 4
TOL = 1e-8            # 'k eigenvector error' asked of partial_hevp: eigenvalue errors are its square


def lap(dt=np.float64):
    from raleigh_amd.synthetic import lap3d_rows
    return sp.csr_matrix(lap3d_rows(*GRID, 0, N).astype(dt))


def lap_eigenvalues(k):
    from raleigh_amd.synthetic import hermitian_lap3d_eigenvalues
    return hermitian_lap3d_eigenvalues(*GRID, skew=0.0)[:k]


def hermitian(dt=np.complex128):
    from raleigh_amd.synthetic import hermitian_lap3d_rows
    return sp.csr_matrix(hermitian_lap3d_rows(10, 6, 5, 1.0, 1.01, 1.02, 0, 300).astype(dt))


def _unit(dt):
    return float(np.finfo(np.dtype(dt)).eps) / 2


def _apply(matrix, x):
    from raleigh_amd.algebra.hip import SparseSymmetricMatrix, Vectors
    op = SparseSymmetricMatrix(matrix)
    X = Vectors(x)
    Y = Vectors(x.shape[1], x.shape[0], data_type=x.dtype.type)
    op.apply(X, Y)
    return op, Y.data().copy()


def apply_matches(device, monkeypatch):
    """SparseSymmetricMatrix(tensor).apply against the SciPy-built operator.  With the same layout asked of both
    builds (RLH_SPMM_FORMAT=wide: the host build would otherwise take the 1024-row windowed layout for the stencils,
    which the device build does not offer) the two results are equal bit for bit: same stored order, same kernel.
    Left to choose their layouts, both lie within (L + 2) u sum_j |a_ij| |x_j| of the float64 product, L = 7 entries
    per row at most."""
    rng = np.random.default_rng(3)
    for A in (lap(np.float32), lap(np.float64), hermitian()):
        dt = A.dtype.type
        n = A.shape[0]
        x = rng.standard_normal((3, n))
        if np.dtype(dt).kind == 'c':
            x = x + 1j * rng.standard_normal((3, n))
        x = x.astype(dt)
        if np.dtype(dt).kind == 'c':
            exact = (A.astype(np.complex128) @ x.astype(np.complex128).T).T
        else:
            exact = (A.astype(np.float64) @ x.astype(np.float64).T).T
        bound = (7 + 2) * _unit(dt) * np.asarray(abs(A).astype(np.float64) @ np.abs(x).astype(np.float64).T).T
        for index in (np.int32, np.int64):
            op, y = _apply(csr_tensor(A, device, index), x)
            _, ref = _apply(A, x)
            assert op.size() == n and op.data_type() == np.dtype(dt) and op.nnz_full() == A.nnz
            assert op.layout()[0] in ('sell', 'well', 'wide')
            # a little over the bound's own rounding: the reference product is float64, not exact
            assert np.all(np.abs(y - exact) <= bound * 1.001 + 9 * _unit(np.float64) * np.abs(exact))
            assert np.all(np.abs(ref - exact) <= bound * 1.001 + 9 * _unit(np.float64) * np.abs(exact))
        monkeypatch.setenv('RLH_SPMM_FORMAT', 'wide')
        op, y = _apply(csr_tensor(A, device), x)
        _, ref = _apply(A, x)
        monkeypatch.delenv('RLH_SPMM_FORMAT')
        assert np.array_equal(y.view(np.uint8), ref.view(np.uint8))
        u = op.csr()                                  # (the documented host copy: the upper triangle)
        assert (abs(u - sp.triu(A, format='csr'))).nnz == 0


def odd_storage(device):
    """Tensors torch accepts and keeps as they are -- int32 row pointers with int64 columns, values and columns that
    are strided views -- go through conversions on torch's stream before the library reads them: the operator is the
    one of the plain tensor, bit for bit (both built on the device, the same layout)."""
    import torch
    rng = np.random.default_rng(4)
    for A in (lap(np.float64), hermitian()):
        n = A.shape[0]
        x = rng.standard_normal((3, n)).astype(A.dtype)
        _, ref = _apply(csr_tensor(A, device), x)
        crow = torch.from_numpy(A.indptr.astype(np.int32)).to(device)
        col = torch.from_numpy(np.repeat(A.indices.astype(np.int64), 2)).to(device)[::2]
        val = torch.from_numpy(np.repeat(A.data, 3)).to(device)[::3]
        assert not col.is_contiguous() and not val.is_contiguous()
        t = torch.sparse_csr_tensor(crow, col, val, size=A.shape)
        assert t.crow_indices().dtype != t.col_indices().dtype and not t.values().is_contiguous()
        _, y = _apply(t, x)
        assert np.array_equal(y.view(np.uint8), ref.view(np.uint8))
        _, y = _apply(torch.sparse_csr_tensor(crow, col.to(torch.int32), val, size=A.shape), x)
        assert np.array_equal(y.view(np.uint8), ref.view(np.uint8))


class _Elsewhere:
    """A sparse_csr tensor that says it lies on GPU `index` (everything else is the wrapped tensor's)."""

    class _Device:
        type = 'cuda'

        def __init__(self, index):
            self.index = index

    def __init__(self, t, index):
        self._t, self.is_cuda, self.device = t, True, self._Device(index)

    def __getattr__(self, name):
        return getattr(self._t, name)


def other_gpu(monkeypatch):
    """The operator's own check of a tensor (sparse.operator_tensor) refuses one on a GPU the library is not bound
    to, whatever the machine has: the bound device is patched to 0, the tensor says 1."""
    from raleigh_amd import _lib
    from raleigh_amd.algebra.hip.sparse import operator_tensor
    monkeypatch.setattr(_lib, 'local_device', lambda: 0)
    with pytest.raises(ValueError, match='lies on GPU 1, the library is bound to GPU 0'):
        operator_tensor(_Elsewhere(csr_tensor(lap(), 'cpu'), 1))


def _residual(A, B, lmd, x):
    bx = x if B is None else B @ x
    return float(np.linalg.norm(A @ x - bx * lmd))


def _both(A, B, device, exact, precond=None, **kw):
    """partial_hevp on tensors and on the SciPy matrices; the checks the two tiers share."""
    import torch
    from raleigh_amd.interfaces import partial_hevp
    out = []
    for a, b in ((csr_tensor(A, device), None if B is None else csr_tensor(B, device, np.int32)), (A, B)):
        args = dict(kw)
        if precond is not None:
            args.update(precond(a))
        np.random.seed(1)
        lmd, x, status = partial_hevp(a, B=b, which=WHICH, tol=TOL, verb=-1, **args)
        assert status == 0
        out.append((lmd, x))
    (lmd, x), (lmd_ref, x_ref) = out
    assert isinstance(lmd, np.ndarray) and isinstance(x, torch.Tensor) and isinstance(x_ref, np.ndarray)
    assert x.device.type == torch.device(device).type and tuple(x.shape) == (N, WHICH) == x_ref.shape
    assert np.max(np.abs(lmd[:WHICH] - exact)) <= 1e-10
    assert np.max(np.abs(lmd_ref[:WHICH] - exact)) <= 1e-10
    res, res_ref = _residual(A, B, lmd, host(x).astype(np.float64)), _residual(A, B, lmd_ref, x_ref)
    print('residual: tensor %.3e, SciPy %.3e' % (res, res_ref))
    assert res <= 10 * res_ref
    return lmd, lmd_ref


def hevp_plain(device):
    _both(lap(), None, device, lap_eigenvalues(WHICH), T=True)


def hevp_chebyshev(device):
    from raleigh_amd.algebra.hip import SparseSymmetricMatrix
    from raleigh_amd.algebra.hip.precond import ChebyshevPreconditioner, gershgorin_upper_bound
    A = lap()
    hi = gershgorin_upper_bound(A)
    _both(A, None, device, lap_eigenvalues(WHICH),
          precond=lambda a: {'T': ChebyshevPreconditioner(SparseSymmetricMatrix(a), hi, ratio=50.0, degree=6)})


def hevp_generalized(device):
    """A x = lambda B x with the diagonal mass matrix B = 2 I: the closed form halved."""
    B = sp.identity(N, dtype=np.float64, format='csr') * 2.0
    _both(lap(), sp.csr_matrix(B), device, lap_eigenvalues(WHICH) / 2, T=True)


def hevp_iterative(device):
    """Shift-invert with the iterative solver, the shift below the fourth eigenvalue (between the first and the
    second): the matrix is positive definite, the shifted one is not."""
    from raleigh_amd.algebra.hip.shift_invert import IterativeSymmetricSolver
    ev = lap_eigenvalues(WHICH + 2)
    sigma = 0.5 * (ev[0] + ev[1])
    assert sigma < ev[3]
    order = np.argsort(np.abs(ev - sigma))           # which=4: the four eigenvalues nearest the shift
    exact = np.sort(ev[order[:WHICH]])
    _both(lap(), None, device, exact, precond=lambda a: {'solver': IterativeSymmetricSolver(dtype=np.float64, tol=1e-12)},
          sigma=sigma)


def direct_mode(device):
    """The direct factorisation is a host algorithm (one copy of the tensor to the host): the SciPy path's
    eigenvalues, eigenvectors as a tensor."""
    import torch
    from raleigh_amd.interfaces import partial_hevp
    A = lap()
    np.random.seed(1)
    lmd, x, status = partial_hevp(csr_tensor(A, device), sigma=0, which=WHICH, tol=1e-6, verb=-1)
    np.random.seed(1)
    lmd_ref, x_ref, status_ref = partial_hevp(A, sigma=0, which=WHICH, tol=1e-6, verb=-1)
    assert status == 0 == status_ref
    assert isinstance(x, torch.Tensor) and tuple(x.shape) == x_ref.shape
    assert np.allclose(lmd, lmd_ref, rtol=1e-12, atol=0)


def cpu_tensor(fake=None):
    """A CPU tensor goes down the host path: ndarrays, identical to those of the SciPy call."""
    from raleigh_amd.interfaces import partial_hevp
    A = lap()
    np.random.seed(1)
    lmd, x, status = partial_hevp(csr_tensor(A, 'cpu'), T=True, which=WHICH, tol=1e-6, verb=-1)
    np.random.seed(1)
    lmd_ref, x_ref, _ = partial_hevp(A, T=True, which=WHICH, tol=1e-6, verb=-1)
    assert status == 0 and isinstance(x, np.ndarray) and isinstance(lmd, np.ndarray)
    assert np.array_equal(lmd, lmd_ref) and np.array_equal(x, x_ref)


def rejections(device, other=None):
    import torch
    from raleigh_amd.algebra.hip import SparseSymmetricMatrix
    from raleigh_amd.interfaces import partial_hevp
    A = lap()
    good = csr_tensor(A, device)
    with pytest.raises(ValueError, match='square'):
        SparseSymmetricMatrix(csr_tensor(sp.csr_matrix(A[:400]), device))
    with pytest.raises(ValueError, match='layout'):
        SparseSymmetricMatrix(good.to_dense())
    with pytest.raises(ValueError, match='layout'):
        SparseSymmetricMatrix(good.to_sparse_coo())
    for bad in (torch.float16, torch.bfloat16, torch.int32):
        t = torch.sparse_csr_tensor(good.crow_indices(), good.col_indices(), good.values().to(bad), size=good.shape)
        with pytest.raises(ValueError, match='not supported'):
            SparseSymmetricMatrix(t)
        with pytest.raises(ValueError, match='not supported'):
            partial_hevp(t, T=True, which=2, verb=-1)
    if other is not None:
        with pytest.raises(ValueError, match='lies on GPU'):
            SparseSymmetricMatrix(csr_tensor(A, other))
    with pytest.raises(ValueError, match='square'):
        partial_hevp(good, B=csr_tensor(sp.csr_matrix(A[:400]), device), T=True, which=2, verb=-1)


def structure_must_be_symmetric(device):
    """An upper triangle alone is not taken on the device (the build creates no entries): RlhError names the entry."""
    from raleigh_amd import _lib
    from raleigh_amd.algebra.hip import SparseSymmetricMatrix
    with pytest.raises(_lib.RlhError, match=r'not symmetric: entry \(0, 1\)'):
        SparseSymmetricMatrix(csr_tensor(sp.csr_matrix(sp.triu(lap())), device))
