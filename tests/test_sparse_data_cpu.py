"""CPU tier: truncated SVD and PCA of scipy.sparse input (host logic of SparseAMatrix / the interfaces over
tests/fake_sparse_data.py), cases of tests/_sparse_data_cases.py."""

import numpy as np
import pytest
import scipy.sparse as sp

import fake_sparse_data
import fake_lib
import _sparse_data_cases as cases


@pytest.fixture(autouse=True)
def fake():
    f = fake_sparse_data.install()
    yield f
    fake_lib.uninstall()


@pytest.mark.parametrize('dt', [np.float32, np.float64])
def test_truncated_svd_matches_dense(dt):
    cases.truncated_svd_matches_dense(dt)


def test_truncated_svd_wide():
    cases.truncated_svd_matches_dense(np.float64, m=120, n=300)


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


def test_sparse_products_run_on_the_sparse_operator(fake):
    """Sparse input reaches the device sparse operator: no dense product is issued and the data never become
    a dense block."""
    from raleigh_amd.interfaces import truncated_svd
    truncated_svd(sp.csr_matrix(cases.data()), nsv=3)
    assert fake.calls.get('spd_apply', 0) > 0
    assert fake.calls.get('dense_apply', 0) == 0


def test_operator_surface(fake):
    from raleigh_amd.algebra.sparse_matrix import SparseAMatrix
    A = cases.data(dt=np.complex128)
    M = SparseAMatrix(A.tocoo())
    D = A.toarray()
    assert M.shape() == D.shape and M.data_type() == np.complex128
    assert np.allclose(M.dots(), (np.abs(D) ** 2).sum(1))
    assert np.isclose(M.frobenius2(), np.linalg.norm(D) ** 2)
    assert M.scale() == max(np.abs(D.real).max(), np.abs(D.imag).max())
    op = M.as_operator()
    assert op.nnz() == A.nnz
    from raleigh_amd.algebra.hip import Vectors
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((3, D.shape[1])) + 1j * rng.standard_normal((3, D.shape[1])))
    X, Y = Vectors(x), Vectors(D.shape[0], 3, np.complex128)
    op.apply(X, Y)
    assert np.allclose(Y.data(), (D @ x.T).T)
    Z = Vectors(D.shape[1], 3, np.complex128)
    op.apply(Y, Z, transp=True)
    assert np.allclose(Z.data(), (D.conj().T @ (D @ x.T)).T)
    with pytest.raises(ValueError):
        op.apply(Y, Y)
