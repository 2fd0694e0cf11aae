"""PCA and truncated SVD of data given as torch tensors, shared by the CPU tier (tests/fake_device_data.py, where
CPU tensors stand for device tensors) and the GPU tier: every call on a tensor against the same call on the host
copy of the data, with the same start vectors (numpy.random.seed before each), so the results must be equal
bit for bit -- same operator arrays, same kernels, same order."""

import numpy as np
import pytest
import scipy.sparse as sp

from _sparse_data_cases import _tol

BYTE_BLOCKS = [(40, 30, 200), (50, 20, 150), (30, 33, 100), (20, 25, 90), (10, 10, 50), (12, 9, 40), (9, 7, 30), (6, 5, 20)]
SPARSE_BLOCKS = [(6, 5, 20), (3, 40, 2), (40, 3, 2)]


def dense_data(m=600, n=400, dt=np.float32, seed=5):
    """An m x n matrix with singular values 100 * 0.6^i, i < 12 (exact ones from a float64 SVD of the stored values)."""
    rng = np.random.default_rng(seed)
    u, _ = np.linalg.qr(rng.standard_normal((m, 12)))
    v, _ = np.linalg.qr(rng.standard_normal((n, 12)))
    A = np.ascontiguousarray(((u * (100.0 * 0.6 ** np.arange(12))) @ v.T + 3.0).astype(dt))
    return A, np.linalg.svd(A.astype(np.float64), compute_uv=False)


def byte_data():
    from raleigh_amd.synthetic import byte_blocks
    return byte_blocks(BYTE_BLOCKS, shape=(300, 208), seed=2)


def sparse_data(dt=np.float64):
    from raleigh_amd.synthetic import block_diagonal_data
    return block_diagonal_data(SPARSE_BLOCKS, dt, seed=4)


def tensor(a, device):
    import torch
    return torch.from_numpy(a).to(device)


def csr_tensor(A, device, index=np.int64):
    import torch
    return torch.sparse_csr_tensor(torch.from_numpy(A.indptr.astype(index)), torch.from_numpy(A.indices.astype(index)),
                                   torch.from_numpy(A.data), size=A.shape).to(device)


def host(t):
    return t.detach().cpu().numpy()


def _same(got, ref, device, dtype):
    """A tuple of tensors on `device`, equal in shape, type and every bit to the host path's arrays."""
    import torch
    assert len(got) == len(ref) and host(got[0]).dtype == np.dtype(dtype)
    for g, r in zip(got, ref):
        assert isinstance(g, torch.Tensor) and g.device.type == torch.device(device).type
        assert isinstance(r, np.ndarray)
        assert tuple(g.shape) == r.shape
        assert host(g).dtype == r.dtype
        assert np.array_equal(host(g), r)


def _run(fn, A, **kw):
    np.random.seed(1)
    return fn(A, **kw)


def _inputs(device):
    """(name, tensor, host data, result type, exact singular values or None)."""
    D, dsig = dense_data()
    B, bsig = byte_data()
    S, ssig = sparse_data()
    return [('dense', tensor(D, device), D, np.float32, dsig),
            ('bytes', tensor(B, device), B, np.float32, bsig),
            ('sparse64', csr_tensor(S, device, np.int64), S, np.float64, ssig),
            ('sparse32', csr_tensor(S, device, np.int32), S, np.float64, ssig)]


NAMES = ['dense', 'bytes', 'sparse64', 'sparse32']


def interfaces_match(name, device):
    from raleigh_amd.interfaces import pca, truncated_svd
    (_, T, H, dt, exact), = [c for c in _inputs(device) if c[0] == name]
    before = None if name.startswith('sparse') else T.clone()
    got = _run(pca, T, npc=6, svtol=1e-12)
    last = dict(pca.last)
    ref = _run(pca, H, npc=6, svtol=1e-12)
    _same(got, ref, device, dt)
    assert got[1].shape == (H.shape[0], 6) and got[2].shape == (6, H.shape[1]) and got[0].shape == (1, H.shape[1])
    assert np.array_equal(last['sigma'], pca.last['sigma']) and last['iterations'] == pca.last['iterations']
    got = _run(truncated_svd, T, nsv=5)
    ref = _run(truncated_svd, H, nsv=5)
    _same(got, ref, device, dt)
    s = host(got[1]).astype(np.float64)
    assert len(s) >= 5
    assert np.max(np.abs(s[:5] - exact[:5])) <= _tol(dt) * exact[0]
    if before is not None:
        assert np.array_equal(host(T), host(before))        # the caller's tensor is never written


def pca_have(device):
    """pca(A1, have=...) with tensors in `have`, with ndarrays in `have`, and with a mix."""
    from raleigh_amd.interfaces import pca
    D, _ = dense_data()
    D0, D1 = np.ascontiguousarray(D[:350]), np.ascontiguousarray(D[350:])
    have_h = _run(pca, D0, npc=6, svtol=1e-12)
    have_t = _run(pca, tensor(D0, device), npc=6, svtol=1e-12)
    _same(have_t, have_h, device, np.float32)
    ref = _run(pca, D1, npc=6, have=have_h, svtol=1e-12)
    T1 = tensor(D1, device)
    _same(_run(pca, T1, npc=6, have=have_t, svtol=1e-12), ref, device, np.float32)
    _same(_run(pca, T1, npc=6, have=have_h, svtol=1e-12), ref, device, np.float32)
    _same(_run(pca, T1, npc=6, have=(have_t[0], have_h[1], have_t[2]), svtol=1e-12), ref, device, np.float32)
    assert ref[1].shape == (600, 6)
    mixed = _run(pca, D1, npc=6, have=have_t, svtol=1e-12)      # host rows, tensors in have: host results
    assert all(isinstance(x, np.ndarray) and np.array_equal(x, r) for x, r in zip(mixed, ref))


def rejections(device, other_device=None):
    import torch
    from raleigh_amd.interfaces import pca, truncated_svd
    D, _ = dense_data(60, 40)
    T = tensor(D, device)
    bad = [T[0], T.reshape(6, 10, 40),                                                    # not 2-D
           T.to(torch.float16), T.to(torch.bfloat16), T > 0, T.to(torch.int16), T.to(torch.int32), T.to(torch.int64),
           T.to_sparse(), T.to_sparse_csc(), T.to_sparse_bsr((2, 2))]                     # the other sparse layouts
    for t in bad:
        with pytest.raises(ValueError):
            pca(t, npc=3)
        with pytest.raises(ValueError):
            truncated_svd(t, nsv=3)
    with pytest.raises(ValueError, match='batch_size'):
        pca(T, npc=3, batch_size=20)
    with pytest.raises(ValueError, match='batch_size'):
        pca(T.to_sparse_csr(), npc=3, batch_size=20)
    if other_device is not None:
        with pytest.raises(ValueError, match='GPU'):
            pca(tensor(D, other_device), npc=3)


def grad_and_conj(device):
    """A tensor that requires grad is detached; a conjugated view is resolved by one copy."""
    import torch
    from raleigh_amd.interfaces import truncated_svd
    D, _ = dense_data(120, 80)
    T = tensor(D, device).requires_grad_(True)
    _same(_run(truncated_svd, T, nsv=3), _run(truncated_svd, D, nsv=3), device, np.float32)
    Z = (D + 1j * dense_data(120, 80, seed=6)[0]).astype(np.complex64)
    C = tensor(Z, device).conj()
    assert C.is_conj()
    _same(_run(truncated_svd, C, nsv=3), _run(truncated_svd, np.ascontiguousarray(Z.conj()), nsv=3), device, np.complex64)
    assert np.array_equal(host(C.conj()), Z)


def cpu_tensor_takes_host_path():
    """A CPU tensor returns ndarrays equal to the ndarray path's."""
    import torch
    from raleigh_amd.interfaces import pca, truncated_svd
    D, _ = dense_data(120, 80)
    S, _ = sparse_data()
    B, _ = byte_data()
    for T, H in ((torch.from_numpy(D), D), (torch.from_numpy(B), B), (csr_tensor(S, 'cpu', np.int32), S),
                 (torch.from_numpy(D).T, np.ascontiguousarray(D.T))):
        got, ref = _run(truncated_svd, T, nsv=3), _run(truncated_svd, H, nsv=3)
        assert all(isinstance(g, np.ndarray) and np.array_equal(g, r) for g, r in zip(got, ref))
    got, ref = _run(pca, torch.from_numpy(D), npc=3), _run(pca, D, npc=3)
    assert all(isinstance(g, np.ndarray) and np.array_equal(g, r) for g, r in zip(got, ref))


# ---- the matrices of the raw C ABI comparison of the two sparse builds (all canonical)

def _values(rng, n, dt):
    v = rng.standard_normal(n)
    if np.dtype(dt).kind == 'c':
        v = v + 1j * rng.standard_normal(n)
    return v.astype(dt)


def build_matrices(dt):
    """(name, csr, RLH_SPD_TABLE_BYTES or None).  The device build changes path with the number of row chunks
    C = min(nnz // 8192 + 1, table cap // (8 (N + 1))), at least 1: one chunk below 8192 stored entries and two from
    there on ('nnz8191' / 'nnz8192'); and where the cap binds -- the power-law matrix would take C = nnz // 8192 + 1
    chunks, and is built with a table that holds exactly that many rows ('cap_at'), one fewer ('cap_below') and
    less than one ('cap_one': C = 1)."""
    from raleigh_amd.synthetic import sparse_data as synth
    rng = np.random.default_rng(12)
    out = [('0x5', sp.csr_matrix((0, 5), dtype=dt), None), ('5x0', sp.csr_matrix((5, 0), dtype=dt), None),
           ('1x1', sp.csr_matrix(np.array([[2.5]]).astype(dt)), None)]
    a = np.zeros((7, 3))
    a[0, 0] = a[0, 2] = a[3, 2] = a[6, 0] = 1.0                 # rows 1, 2, 4, 5 and column 1 are empty
    a = sp.csr_matrix(a.astype(dt))
    a.data[:] = _values(rng, a.nnz, dt)
    out.append(('7x3', a, None))
    # 300 x 70000: column 0 holds every row, row 0 holds 60000 entries
    cols0 = np.concatenate(([0], 1 + np.sort(rng.choice(69999, 59999, replace=False))))
    rows = np.concatenate((np.zeros(60000, dtype=np.int64), np.arange(1, 300), np.repeat(np.arange(1, 300), 4)))
    cols = np.concatenate((cols0, np.zeros(299, dtype=np.int64), rng.integers(1, 70000, 4 * 299)))
    key = np.unique(rows * 70000 + cols)
    a = sp.csr_matrix((_values(rng, key.size, dt), (key // 70000, key % 70000)), shape=(300, 70000))
    out.append(('long', a, None))
    out.append(('20000x257', synth(20000, 257, 3, 'uniform', dt, 3), None))
    p = synth(5000, 2000, 10, 'powerlaw', dt, 5)
    out.append(('powerlaw', p, None))
    C = p.nnz // 8192 + 1
    assert C >= 3
    out.append(('cap_at', p, C * 8 * 2001))
    out.append(('cap_below', p, C * 8 * 2001 - 1))
    out.append(('cap_one', p, 8 * 2001 - 1))
    for nnz in (8191, 8192):
        key = np.sort(rng.choice(900 * 700, nnz, replace=False))
        out.append(('nnz%d' % nnz, sp.csr_matrix((_values(rng, nnz, dt), (key // 700, key % 700)), shape=(900, 700)), None))
    for name, a, cap in out:
        a.sort_indices()
        assert a.has_canonical_format
    return out
