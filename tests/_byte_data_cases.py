"""PCA and truncated SVD of 8-bit data (uint8 / int8 ndarrays through ByteAMatrix), shared by the CPU tier
(tests/fake_byte_data.py) and the GPU tier: every call on bytes against float64 NumPy on the same integers and
against the same call on ``A.astype(float32)``, which takes the float32 path."""

import numpy as np
import pytest

# name -> (rows, columns, signed): synthetic.byte_images of rank 8
IMAGES = {'tall': (600, 200, False), 'wide': (150, 400, False), 'signed': (600, 200, True)}
NPC = 8
TOL = 2e-5          # the float32 figure of _sparse_data_cases._tol
ERR_RTOL = 1e-4     # pca_error against the optimal rank-NPC errors


def images(name, seed=5):
    from raleigh_amd.synthetic import byte_images
    m, n, signed = IMAGES[name]
    return byte_images(m, n, NPC, seed=seed, signed=signed)


def _optimal(A64, k):
    """Singular values of the centred data, its mean, and the (max row, Frobenius) relative errors of its best
    rank-k approximation, all in float64."""
    mean = A64.mean(axis=0)
    Ds = A64 - mean
    u, s, vt = np.linalg.svd(Ds, full_matrices=False)
    R = Ds - (u[:, :k] * s[:k]) @ vt[:k]
    rows = lambda a: np.sqrt((a * a).sum(axis=1))
    return s, mean, (rows(R).max() / rows(Ds).max(), np.linalg.norm(R) / np.linalg.norm(Ds))


def _errors(A64, mean, trans, comps):
    from raleigh_amd.interfaces.pca import pca_error
    return pca_error(A64, mean.astype(np.float64), trans.astype(np.float64), comps.astype(np.float64))


def _is_f32(*arrays):
    for a in arrays:
        assert a.dtype == np.float32


def pca_matches(name):
    from raleigh_amd.interfaces import pca
    A8 = images(name)
    A64 = A8.astype(np.float64)
    exact, mean64, opt = _optimal(A64, NPC)
    mean, trans, comps = pca(A8, npc=NPC, svtol=1e-12)
    sig = pca.last['sigma']
    fmean, ftrans, fcomps = pca(A8.astype(np.float32), npc=NPC, svtol=1e-12)
    fsig = pca.last['sigma']
    _is_f32(mean, trans, comps)
    assert trans.shape == (A8.shape[0], NPC) and comps.shape == (NPC, A8.shape[1])
    print(name, 'sigma vs float64', np.max(np.abs(sig - exact[:NPC])) / exact[0], 'vs float32 path',
          np.max(np.abs(sig - fsig)) / fsig[0])
    assert np.max(np.abs(sig - exact[:NPC])) <= TOL * exact[0]
    assert np.max(np.abs(sig - fsig)) <= TOL * fsig[0]
    assert np.max(np.abs(mean - mean64)) <= TOL * np.abs(mean64).max()
    assert np.max(np.abs(mean - fmean)) <= TOL * np.abs(fmean).max()
    e = _errors(A64, mean, trans, comps)
    print(name, 'pca_error', e, 'optimal', opt)
    assert np.allclose(e, opt, rtol=ERR_RTOL, atol=0)


def _update_checks(A8, got, ref, label):
    """An updated / incremental PCA is not the truncated SVD of the whole data (every step truncates), so the
    singular values and errors of the 8-bit run are held against the float32 path taking the SAME steps, with the
    tolerances of pca_matches; the mean, which no truncation touches, against float64 as well."""
    A64 = A8.astype(np.float64)
    (mean, trans, comps, sig), (fmean, ftrans, fcomps, fsig) = got, ref
    _is_f32(mean, trans, comps)
    assert trans.shape[0] == A8.shape[0]
    assert trans.shape == ftrans.shape and comps.shape == fcomps.shape
    mean64 = A64.mean(axis=0)
    print(label, 'sigma vs float32 path', np.max(np.abs(sig - fsig)) / fsig[0])
    assert np.max(np.abs(mean - mean64)) <= TOL * np.abs(mean64).max()
    assert np.max(np.abs(mean - fmean)) <= TOL * np.abs(fmean).max()
    assert np.max(np.abs(sig - fsig)) <= TOL * fsig[0]
    e, fe = _errors(A64, mean, trans, comps), _errors(A64, fmean, ftrans, fcomps)
    print(label, 'pca_error', e, 'float32 path', fe)
    assert np.allclose(e, fe, rtol=ERR_RTOL, atol=0)


def pca_have(bytes_first):
    """400 + 200 rows, one part float32 and the other bytes, against both parts float32."""
    from raleigh_amd.interfaces import pca
    A8 = images('tall')
    A32 = A8.astype(np.float32)
    first, second = (A8[:400], A32[400:]) if bytes_first else (A32[:400], A8[400:])
    have = pca(first, npc=NPC, svtol=1e-12)
    _is_f32(*have)
    got = pca(second, npc=NPC, have=have, svtol=1e-12) + (pca.last['sigma'],)
    fhave = pca(A32[:400], npc=NPC, svtol=1e-12)
    ref = pca(A32[400:], npc=NPC, have=fhave, svtol=1e-12) + (pca.last['sigma'],)
    _update_checks(A8, got, ref, 'have, bytes %s' % ('first' if bytes_first else 'second'))


def pca_batches():
    from raleigh_amd.interfaces import pca
    A8 = images('tall')
    got = pca(A8, npc=NPC, batch_size=200, svtol=1e-12) + (pca.last['sigma'],)
    ref = pca(A8.astype(np.float32), npc=NPC, batch_size=200, svtol=1e-12) + (pca.last['sigma'],)
    _update_checks(A8, got, ref, 'batch_size=200')


def truncated_svd_matches(name):
    from raleigh_amd.interfaces import truncated_svd
    A8 = images(name)
    A64 = A8.astype(np.float64)
    u, s, vt = truncated_svd(A8, nsv=5)
    fu, fs, fvt = truncated_svd(A8.astype(np.float32), nsv=5)
    exact = np.linalg.svd(A64, compute_uv=False)
    _is_f32(u, s, vt)
    assert len(s) >= 5
    print(name, 'sigma vs float64', np.max(np.abs(s[:5] - exact[:5])) / exact[0])
    assert np.max(np.abs(s[:5] - exact[:5])) <= TOL * exact[0]
    assert np.max(np.abs(s[:5] - fs[:5])) <= TOL * fs[0]
    k = len(s)
    assert np.abs(u.T @ u - np.eye(k)).max() < 2e-3
    assert np.linalg.norm(A64 @ vt.T - u * s) <= 10 * np.sqrt(np.finfo(np.float32).eps) * s[0]


def truncated_svd_norms(shape=None):
    """shape None: the 600 x 200 pictures (so few columns that the solver ends up with every singular value, on
    both paths); (700, 600): the stopping criteria decide."""
    from raleigh_amd.interfaces import truncated_svd
    from raleigh_amd.synthetic import byte_images
    A8 = images('tall') if shape is None else byte_images(shape[0], shape[1], NPC, seed=5, signed=True)
    A64 = A8.astype(np.float64)
    for norm, tol in (('s', 0.3), ('f', 0.2), ('m', 0.3)):
        u, s, vt = truncated_svd(A8, tol=tol, norm=norm)
        fu, fs, fvt = truncated_svd(A8.astype(np.float32), tol=tol, norm=norm)
        assert len(s) == len(fs), norm
        R = A64 - (u.astype(np.float64) * s) @ vt
        err = {'s': np.linalg.norm(R, 2) / np.linalg.norm(A64, 2), 'f': np.linalg.norm(R) / np.linalg.norm(A64),
               'm': np.sqrt((R ** 2).sum(1).max() / (A64 ** 2).sum(1).max())}[norm]
        print('norm', norm, 'values', len(s), 'error', err, 'tolerance', tol)
        assert err <= tol * 1.001, norm


BLOCKS = [(40, 30, 200), (50, 20, 150), (30, 33, 100), (20, 25, 90), (10, 10, 50)]


def known_values(signed=False):
    from raleigh_amd.interfaces import truncated_svd
    from raleigh_amd.synthetic import byte_blocks
    blocks = [(p, q, -v // 2 if signed and i % 2 else v // (2 if signed else 1)) for i, (p, q, v) in enumerate(BLOCKS)]
    A8, sigma = byte_blocks(blocks, shape=(300, 200), seed=2, signed=signed)
    assert A8.dtype == (np.int8 if signed else np.uint8) and A8.flags['C_CONTIGUOUS']
    assert np.allclose(np.linalg.svd(A8.astype(np.float64), compute_uv=False)[:len(sigma)], sigma, rtol=1e-12)
    u, s, vt = truncated_svd(A8, nsv=3)
    assert len(s) >= 3
    assert np.max(np.abs(s[:3] - sigma[:3])) <= TOL * sigma[0]


def operator_surface():
    from raleigh_amd.algebra.byte_matrix import ByteAMatrix
    from raleigh_amd.algebra.hip import Vectors
    rng = np.random.default_rng(4)
    for dt, lo, hi in ((np.uint8, 0, 256), (np.int8, -128, 128)):
        A8 = rng.integers(lo, hi, size=(70, 45)).astype(dt)
        A8[3, 7] = hi - 1
        A8[5, 9] = lo
        M = ByteAMatrix(A8)
        I = A8.astype(np.int64)
        assert M.shape() == A8.shape
        assert M.data_type() == np.float32
        d = M.dots()
        assert d.dtype == np.float64 and np.array_equal(d, (I * I).sum(axis=1).astype(np.float64))
        assert M.frobenius2() == float((I * I).sum())
        assert M.scale() == float(np.abs(I).max())
        op = M.as_operator()
        assert op.storage_type() == dt and not op.is_complex()
        assert op.workspace_bytes() >= 0 and op.device_bytes() >= A8.size
        x = rng.standard_normal((3, 45)).astype(np.float32)
        X, Y = Vectors(x), op.new_vectors(70, 3)
        assert Y.data_type() == np.float32
        op.apply(X, Y)
        assert np.allclose(Y.data(), (I @ x.T.astype(np.float64)).T, rtol=1e-5, atol=1e-3)
        Z = op.new_vectors(45, 3)
        op.apply(Y, Z, transp=True)
        assert np.allclose(Z.data(), (I.T @ Y.data().T.astype(np.float64)).T, rtol=1e-5, atol=1.0)
        with pytest.raises(ValueError):
            op.apply(Y, Y)
        with pytest.raises(ValueError):
            op.apply(Vectors(x.astype(np.float64)), Vectors(70, 3, np.float64))
    # the longest row of 255s a 32-bit sum cannot hold
    big = np.full((2, 70000), 255, dtype=np.uint8)
    assert np.array_equal(ByteAMatrix(big).dots(), np.full(2, 255.0 ** 2 * 70000))


def refusals():
    from raleigh_amd.interfaces import truncated_svd, pca
    from raleigh_amd.interfaces.lra import LowerRankApproximation, _as_matrix
    A8 = images('tall')
    for dt in (np.uint16, np.int32, np.bool_, np.float16):
        with pytest.raises(ValueError):
            pca(A8.astype(dt), npc=3)
        with pytest.raises(ValueError):
            truncated_svd(A8.astype(dt), nsv=3)
        with pytest.raises(ValueError):
            _as_matrix(A8.astype(dt), 'hip')
    with pytest.raises(ValueError):
        pca(A8[0].copy(), npc=3)
    with pytest.raises(ValueError):
        truncated_svd(A8[0].copy(), nsv=3)
    with pytest.raises(ValueError):
        pca(np.asfortranarray(A8), npc=3)
    with pytest.raises(ValueError):
        pca(np.asfortranarray(A8), npc=3, batch_size=200)
    with pytest.raises(ValueError):
        pca(A8, npc=3, norm='x')
    assert LowerRankApproximation is not None
