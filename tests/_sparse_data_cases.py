"""Truncated SVD and PCA of sparse data (scipy.sparse input through SparseAMatrix), shared by the CPU tier
(tests/fake_sparse_data.py) and the GPU tier: every call on CSR input against the same call on the dense
array, which takes the dense path."""

import numpy as np
import pytest
import scipy.sparse as sp


def data(m=400, n=150, dt=np.float64, kind='powerlaw', seed=3):
    from raleigh_amd.synthetic import sparse_data
    return sparse_data(m, n, 12, kind=kind, dtype=dt, seed=seed)


def _tol(dt):
    return 2e-5 if np.dtype(dt).itemsize // (2 if np.dtype(dt).kind == 'c' else 1) == 4 else 1e-10


def truncated_svd_matches_dense(dt=np.float64, m=400, n=150):
    from raleigh_amd.interfaces import truncated_svd
    A = data(m, n, dt)
    D = A.toarray()
    u, s, vt = truncated_svd(A, nsv=5)
    ud, sd, vtd = truncated_svd(D, nsv=5)
    exact = np.linalg.svd(D.astype(np.complex128 if D.dtype.kind == 'c' else np.float64), compute_uv=False)
    assert len(s) >= 5
    assert np.max(np.abs(s[:5] - sd[:5])) <= _tol(dt) * sd[0]
    assert np.max(np.abs(s[:5] - exact[:5])) <= _tol(dt) * exact[0]
    k = len(s)
    assert np.abs(u.conj().T @ u - np.eye(k)).max() < 100 * _tol(dt)
    assert np.linalg.norm(D @ vt.T - u * s) <= 10 * np.sqrt(np.finfo(dt).eps) * s[0]


def truncated_svd_norms():
    from raleigh_amd.interfaces import truncated_svd
    A = data()
    D = A.toarray()
    for norm, tol in (('s', 0.3), ('f', 0.6), ('m', 0.7)):
        u, s, vt = truncated_svd(A, tol=tol, norm=norm)
        ud, sd, vtd = truncated_svd(D, tol=tol, norm=norm)
        assert len(s) == len(sd), norm
        assert np.max(np.abs(s - sd)) <= 1e-10 * sd[0]
        R = D - (u * s) @ vt
        err = {'s': np.linalg.norm(R, 2) / np.linalg.norm(D, 2), 'f': np.linalg.norm(R) / np.linalg.norm(D),
               'm': np.sqrt((np.abs(R) ** 2).sum(1).max() / (np.abs(D) ** 2).sum(1).max())}[norm]
        assert err <= tol * 1.001, norm


def pca_matches_dense(dt=np.float64):
    from raleigh_amd.interfaces import pca
    from raleigh_amd.interfaces.pca import pca_error
    A = data(dt=dt)
    D = A.toarray()
    mean, trans, comps = pca(A, npc=6, svtol=1e-12)
    sig = pca.last['sigma']
    dmean, dtrans, dcomps = pca(D, npc=6, svtol=1e-12)
    dsig = pca.last['sigma']
    Ds = D - D.mean(axis=0)
    exact = np.linalg.svd(Ds, compute_uv=False)
    assert np.max(np.abs(mean - dmean)) <= _tol(dt) * np.abs(dmean).max()
    assert np.max(np.abs(sig - dsig)) <= _tol(dt) * dsig[0]
    assert np.max(np.abs(sig - exact[:6])) <= _tol(dt) * exact[0]
    e, ed = pca_error(D, mean, trans, comps), pca_error(D, dmean, dtrans, dcomps)
    assert np.allclose(e, ed, rtol=1e-6, atol=0)


def pca_have_matches_dense():
    from raleigh_amd.interfaces import pca
    from raleigh_amd.interfaces.pca import pca_error
    A = data(600, 150)
    A0, A1 = A[:400], A[400:]
    have = pca(A0.toarray(), npc=6, svtol=1e-12)
    mean, trans, comps = pca(A1, npc=6, have=have, svtol=1e-12)
    dmean, dtrans, dcomps = pca(A1.toarray(), npc=6, have=have, svtol=1e-12)
    D = A.toarray()
    assert trans.shape[0] == 600
    assert np.max(np.abs(mean - dmean)) <= 1e-10 * np.abs(dmean).max()
    assert np.max(np.abs(mean - D.mean(axis=0))) <= 1e-10 * np.abs(dmean).max()
    assert np.allclose(pca_error(D, mean, trans, comps), pca_error(D, dmean, dtrans, dcomps), rtol=1e-6, atol=0)


def pca_batches_match_dense():
    from raleigh_amd.interfaces import pca
    from raleigh_amd.interfaces.pca import pca_error
    A = data(600, 150)
    D = A.toarray()
    mean, trans, comps = pca(A, npc=6, batch_size=200, svtol=1e-12)
    dmean, dtrans, dcomps = pca(np.ascontiguousarray(D), npc=6, batch_size=200, svtol=1e-12)
    assert trans.shape == (600, 6) and comps.shape == (6, 150)
    assert np.max(np.abs(mean - dmean)) <= 1e-10 * np.abs(dmean).max()
    assert np.allclose(pca_error(D, mean, trans, comps), pca_error(D, dmean, dtrans, dcomps), rtol=1e-6, atol=0)


def refusals():
    from raleigh_amd.interfaces import truncated_svd, pca
    A = data()
    with pytest.raises(ValueError):
        truncated_svd(sp.csr_matrix(A.astype(np.int64)), nsv=5)
    with pytest.raises(ValueError):
        pca(sp.csr_matrix(A.astype(np.int32)), npc=5)
    with pytest.raises(ValueError):
        truncated_svd(sp.csr_matrix(A)[0].toarray().ravel(), nsv=5)
    if hasattr(sp, 'coo_array'):
        try:
            one_d = sp.coo_array(np.arange(5.0))
        except (ValueError, TypeError):
            one_d = None            # scipy without 1-D sparse arrays
        if one_d is not None:
            with pytest.raises(ValueError):
                truncated_svd(one_d, nsv=2)
    with pytest.raises(ValueError):
        truncated_svd(A, nsv=5, norm='x')
    with pytest.raises(ValueError):
        pca(A, npc=5, norm='x')
