"""Data already in device memory against the same data handed over from the host, on the MI355X: what it costs to
make the operator and to run the whole call.  One JSON line per measurement, a verdict line per expectation.

  python tools/device_data_bench.py [--rows 62500] [--cols 40000] [--npc 16]
                                    [--sparse-rows 1000000] [--sparse-cols 100000] [--nnz-per-row 100] [--m 64]
                                    [--reps 10] [--no-dense] [--no-sparse]

dense, float32 and uint8, rows x cols: operator creation (AMatrix / ByteAMatrix) and end-to-end pca(npc) from an
ndarray against the same data as a device tensor;
sparse, sparse-rows x sparse-cols with nnz-per-row entries a row, float32: the host build (rlh_spd_create: upload and
the transpose on the host threads) against the device build (rlh_spd_create_device) of the same matrix, and one
rlh_spd_apply of m vectors on each handle (HIP-event median of --reps calls after two warm-up calls).
Expectations reported: creation from a device tensor is not slower than creation from the host; a product on a
device-built sparse handle takes the time of one on a host-built handle (it holds the same arrays)."""

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
from raleigh_amd.synthetic import byte_images, sparse_data  # noqa: E402


def emit(rec):
    print(json.dumps(rec), flush=True)


def wall(f):
    _lib.synchronize()
    t0 = time.perf_counter()
    out = f()
    _lib.synchronize()
    return time.perf_counter() - t0, out


def event_median(f, reps):
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
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def dense(rows, cols, npc):
    import torch
    from raleigh_amd.interfaces import pca
    from raleigh_amd.interfaces.lra import _as_matrix_like
    A8 = byte_images(rows, cols, 32, seed=1)
    for name, H in (('uint8', A8), ('float32', A8.astype(np.float32))):
        T = torch.from_numpy(H).to('cuda')
        torch.cuda.synchronize()
        rec = {'what': 'dense', 'dtype': name, 'rows': rows, 'cols': cols, 'data_GB': H.nbytes / 1e9}
        for src, X in (('host', H), ('device', T)):
            best = None
            for _ in range(3):
                s, m = wall(lambda: _as_matrix_like(X, 'hip')[0])
                del m
                best = s if best is None else min(best, s)
            rec['create_from_%s_s' % src] = best
        for src, X in (('host', H), ('device', T)):
            np.random.seed(1)
            s, out = wall(lambda: pca(X, npc=npc))
            rec['pca_from_%s_s' % src] = s
            rec['pca_iterations_%s' % src] = int(pca.last['iterations'])
            del out
        emit(rec)
        emit({'what': 'verdict', 'expectation': 'creation from a device tensor is not slower than from the host',
              'case': 'dense ' + name, 'holds': bool(rec['create_from_device_s'] <= rec['create_from_host_s']),
              'device_s': rec['create_from_device_s'], 'host_s': rec['create_from_host_s']})
        del T
        torch.cuda.empty_cache()


def sparse(rows, cols, per_row, m, reps):
    import torch
    A = sparse_data(rows, cols, per_row, 'uniform', np.float32, seed=1)
    T = torch.sparse_csr_tensor(torch.from_numpy(A.indptr.astype(np.int64)), torch.from_numpy(A.indices.astype(np.int64)),
                                torch.from_numpy(A.data), size=A.shape).to('cuda')
    torch.cuda.synchronize()
    rec = {'what': 'sparse', 'dtype': 'float32', 'rows': rows, 'cols': cols, 'nnz': int(A.nnz), 'm': m}
    ops = {}
    for src, X in (('host', A), ('device', T)):
        best = None
        for _ in range(2):
            ops.pop(src, None)
            s, op = wall(lambda: SparseMatrix(X))
            ops[src] = op
            best = s if best is None else min(best, s)
        rec['create_from_%s_s' % src] = best
        rec['transpose_%s_s' % src] = ops[src].transpose_seconds()
    rng = np.random.default_rng(0)
    X = Vectors(rng.standard_normal((m, cols)).astype(np.float32))
    Z = Vectors(rng.standard_normal((m, rows)).astype(np.float32))
    Y, W = Vectors(rows, m, np.float32), Vectors(cols, m, np.float32)
    same = True
    for transp, (x, y) in ((False, (X, Y)), (True, (Z, W))):
        res = {}
        for src in ('host', 'device'):
            med, lo, hi = event_median(lambda: ops[src].apply(x, y, transp=transp), reps)
            rec['apply_%s_on_%s_built_s' % ('AH' if transp else 'A', src)] = med
            rec['apply_%s_on_%s_built_min_max_s' % ('AH' if transp else 'A', src)] = [lo, hi]
            res[src] = y.data()
        same = same and np.array_equal(res['host'], res['device'])
    rec['products_bit_identical'] = bool(same)
    emit(rec)
    emit({'what': 'verdict', 'expectation': 'creation from a device tensor is not slower than from the host',
          'case': 'sparse', 'holds': bool(rec['create_from_device_s'] <= rec['create_from_host_s']),
          'device_s': rec['create_from_device_s'], 'host_s': rec['create_from_host_s']})
    for o in ('A', 'AH'):
        d, h = rec['apply_%s_on_device_built_s' % o], rec['apply_%s_on_host_built_s' % o]
        emit({'what': 'verdict', 'expectation': 'a product on a device-built handle takes the time of one on a host-built '
              'handle (within 3 %)', 'case': 'sparse ' + o, 'holds': bool(abs(d - h) <= 0.03 * h), 'device_built_s': d,
              'host_built_s': h})


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--rows', type=int, default=62500)
    p.add_argument('--cols', type=int, default=40000)
    p.add_argument('--npc', type=int, default=16)
    p.add_argument('--sparse-rows', type=int, default=1000000)
    p.add_argument('--sparse-cols', type=int, default=100000)
    p.add_argument('--nnz-per-row', type=int, default=100)
    p.add_argument('--m', type=int, default=64)
    p.add_argument('--reps', type=int, default=10)
    p.add_argument('--no-dense', action='store_true')
    p.add_argument('--no-sparse', action='store_true')
    a = p.parse_args()
    _lib.lib(0)
    if not a.no_sparse:
        sparse(a.sparse_rows, a.sparse_cols, a.nnz_per_row, a.m, a.reps)
    if not a.no_dense:
        dense(a.rows, a.cols, a.npc)


if __name__ == '__main__':
    main()
