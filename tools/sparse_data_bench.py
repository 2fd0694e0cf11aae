"""Sparse data operator (rlh_spd_apply) on the MI355X: per-product time of A X and A^H Y, rates, torch.sparse.mm
(hipSPARSE) on the same matrix and block, and end-to-end truncated_svd / pca.  One JSON line per measurement.

  python tools/sparse_data_bench.py [--rows 1000000] [--cols 100000] [--nnz-per-row 100] [--m 64] [--reps 20]
                                    [--no-torch] [--no-e2e] [--svds]

Rates of a product with R output rows, C input rows, nnz entries, m vectors of es bytes:
  gathered bytes / s = nnz * m * es / t                                 (the rows of the block the entries fetch)
  HBM bytes / s      = (nnz * (es + 4) + 8 * (R + 1) + (C + R) * m * es) / t
                        (the matrix once, the interleave of the input and the write of the output once each)
Times are HIP-event medians (with min / max) of --reps calls after two warm-up calls."""

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from raleigh_amd import _lib  # noqa: E402
from raleigh_amd.algebra.hip import SparseMatrix, Vectors  # noqa: E402
from raleigh_amd.synthetic import sparse_data  # noqa: E402


def emit(rec):
    print(json.dumps(rec), flush=True)


def event_times(f, reps):
    L = _lib.lib()
    f()
    f()
    _lib.check(L.rlh_sync())
    ms = ctypes.c_float()
    ts = []
    for _ in range(reps):
        _lib.check(L.rlh_timer_start())
        f()
        _lib.check(L.rlh_timer_stop(ctypes.byref(ms)))
        ts.append(ms.value * 1e-3)
    return np.array(ts)


def torch_times(A, m, dt, reps):
    import torch
    dev = torch.device('cuda', 0)
    tdt = {np.float32: torch.float32, np.float64: torch.float64}[dt]
    out = {}
    for transp, B in ((False, A), (True, A.T.tocsr())):
        t = torch.sparse_csr_tensor(torch.from_numpy(B.indptr.astype(np.int64)), torch.from_numpy(B.indices.astype(np.int64)),
                                    torch.from_numpy(B.data), size=B.shape, dtype=tdt, device=dev)
        x = torch.randn(B.shape[1], m, dtype=tdt, device=dev)
        torch.sparse.mm(t, x)
        torch.sparse.mm(t, x)
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.sparse.mm(t, x)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e-3)
        out[transp] = np.array(ts)
        del t, x
        torch.cuda.empty_cache()
    return out


def products(A, kind, dt, m, reps, with_torch):
    M, N = A.shape
    es = np.dtype(dt).itemsize
    t0 = time.time()
    op = SparseMatrix(A)
    create_s = time.time() - t0
    rng = np.random.default_rng(0)
    X = Vectors(rng.standard_normal((m, N)).astype(dt))
    Z = Vectors(rng.standard_normal((m, M)).astype(dt))
    Y, W = Vectors(M, m, dt), Vectors(N, m, dt)
    tt = torch_times(A, m, dt, reps) if with_torch else {}
    for transp, (src, dst) in ((False, (X, Y)), (True, (Z, W))):
        R, C = (N, M) if transp else (M, N)
        ts = event_times(lambda: op.apply(src, dst, transp=transp), reps)
        t = float(np.median(ts))
        gathered = A.nnz * m * es
        hbm = A.nnz * (es + 4) + 8 * (R + 1) + (C + R) * m * es
        rec = {'what': 'product', 'op': 'AH*Y' if transp else 'A*X', 'kind': kind, 'dtype': np.dtype(dt).name,
               'rows': M, 'cols': N, 'nnz': int(A.nnz), 'm': m, 'median_s': t, 'min_s': float(ts.min()),
               'max_s': float(ts.max()), 'ns_per_nnz': t / A.nnz * 1e9, 'gathered_TBps': gathered / t / 1e12,
               'hbm_TBps': hbm / t / 1e12, 'hbm_share_of_8TBps': hbm / t / 8e12,
               'create_s': create_s, 'transpose_s': op.transpose_seconds(), 'device_bytes': op.device_bytes()}
        if transp in tt:
            rec['torch_sparse_mm_median_s'] = float(np.median(tt[transp]))
            rec['speedup_vs_torch'] = rec['torch_sparse_mm_median_s'] / t
        emit(rec)
    del op


def end_to_end(A, svds):
    from raleigh_amd.interfaces import truncated_svd, pca
    for name, f in (('truncated_svd(nsv=100)', lambda: truncated_svd(A, nsv=100)[1]),
                    ('pca(npc=100)', lambda: (pca(A, npc=100), pca.last['sigma'])[1])):
        t0 = time.time()
        sigma = f()
        _lib.synchronize()
        emit({'what': 'end_to_end', 'call': name, 'rows': A.shape[0], 'cols': A.shape[1], 'nnz': int(A.nnz),
              'dtype': A.dtype.name, 'seconds': time.time() - t0, 'sigma0': float(sigma[0]), 'k': len(sigma)})
    if svds:
        import scipy.sparse.linalg as sla
        t0 = time.time()
        sla.svds(A, k=100)
        emit({'what': 'host_svds', 'call': 'scipy.sparse.linalg.svds(k=100)', 'seconds': time.time() - t0,
              'cores': len(os.sched_getaffinity(0)), 'threads': os.environ.get('OMP_NUM_THREADS')})


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--rows', type=int, default=1000000)
    p.add_argument('--cols', type=int, default=100000)
    p.add_argument('--nnz-per-row', type=int, default=100)
    p.add_argument('--m', type=int, default=64)
    p.add_argument('--reps', type=int, default=20)
    p.add_argument('--no-torch', action='store_true')
    p.add_argument('--no-e2e', action='store_true')
    p.add_argument('--svds', action='store_true')
    a = p.parse_args()
    _lib.lib(0)
    for kind in ('uniform', 'powerlaw'):
        t0 = time.time()
        A64 = sparse_data(a.rows, a.cols, a.nnz_per_row, kind, np.float64, seed=1)
        emit({'what': 'generate', 'kind': kind, 'seconds': time.time() - t0, 'nnz': int(A64.nnz),
              'longest_row': int(np.diff(A64.indptr).max()), 'longest_col': int(np.bincount(A64.indices).max())})
        for dt in (np.float32, np.float64):
            products(A64.astype(dt) if dt != np.float64 else A64, kind, dt, a.m, a.reps, not a.no_torch)
        if kind == 'uniform' and not a.no_e2e:
            end_to_end(A64.astype(np.float32), a.svds)
        del A64


if __name__ == '__main__':
    main()
