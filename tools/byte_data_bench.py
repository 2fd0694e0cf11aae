"""8-bit data operator (rlh_bytes_apply) on the MI355X against the float32 operator (rlh_dense_apply_r1) on the
SAME data converted to float32, alternating in one process: per-product time of A X and A^T Z, rates, and
end-to-end pca.  One JSON line per measurement.

  python tools/byte_data_bench.py [--shapes 62500x40000x32,62500x40000x128,62500x40000x1000,20000x20000x128]
                                  [--reps 20] [--panel 128] [--no-float] [--e2e 62500x40000]

m columns are applied in blocks of --panel (128: the block size pca uses for many components).  Rates of a product
of an M x N matrix with m vectors in t seconds: TF = 2 M N m / t (the three bfloat16 passes are NOT counted
three times); bytes of A / s = M N es / t per panel pass.  Bounds: HBM 8 TB/s for the bytes of A (small m),
bfloat16 matrix cores 2.5 PF / 3 passes (otherwise); float32 matrix cores 157 TF.
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
from raleigh_amd.algebra.hip import ByteMatrix, Matrix, Vectors  # noqa: E402


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


def paneled(op, src, dst, transp, m, panel):
    def f():
        for j in range(0, m, panel):
            w = min(panel, m - j)
            src.select(w, j)
            dst.select(w, j)
            op.apply(src, dst, transp=transp)
        src.select(m)
        dst.select(m)
    return f


def products(A8, ops, m, reps, panel):
    M, N = A8.shape
    rng = np.random.default_rng(0)
    X = Vectors(rng.standard_normal((m, N)).astype(np.float32))
    Z = Vectors(rng.standard_normal((m, M)).astype(np.float32))
    Y, W = Vectors(M, m, np.float32), Vectors(N, m, np.float32)
    passes = (m + panel - 1) // panel
    pair = {}
    for transp, (src, dst) in ((False, (X, Y)), (True, (Z, W))):
        for name, op, es in ops:                # the two paths alternate
            ts = event_times(paneled(op, src, dst, transp, m, panel), reps)
            t = float(np.median(ts))
            tf = 2.0 * M * N * m / t / 1e12
            a_bps = passes * M * N * es / t
            bound_hbm = passes * M * N * es / 8e12
            bound_mfma = 2.0 * M * N * m / (2.5e15 / 3 if name == 'bytes' else 157e12)
            emit({'what': 'product', 'path': name, 'op': 'AT*Z' if transp else 'A*X', 'rows': M, 'cols': N, 'm': m,
                  'panel': panel, 'median_ms': t * 1e3, 'min_ms': float(ts.min()) * 1e3, 'max_ms': float(ts.max()) * 1e3,
                  'TF': tf, 'A_TBps': a_bps / 1e12, 'bound': 'HBM' if bound_hbm > bound_mfma else 'MFMA',
                  'share_of_bound': max(bound_hbm, bound_mfma) / t})
            pair[name] = pair.get(name, 0.0) + t
    rec = {'what': 'pair', 'rows': M, 'cols': N, 'm': m}
    for name in pair:
        rec[name + '_pair_ms'] = pair[name] * 1e3
    if 'float32' in pair:
        rec['speedup'] = pair['float32'] / pair['bytes']
    emit(rec)


def end_to_end(A8, with_float):
    from raleigh_amd.interfaces import pca
    for name, data in (('bytes', lambda: A8), ('float32', lambda: A8.astype(np.float32))):
        if name == 'float32' and not with_float:
            continue
        t0 = time.time()
        a = data()
        t1 = time.time()
        pca(a, npc=100)
        _lib.synchronize()
        emit({'what': 'end_to_end', 'call': 'pca(npc=100)', 'path': name, 'rows': A8.shape[0], 'cols': A8.shape[1],
              'host_convert_s': t1 - t0, 'seconds': time.time() - t1, 'iterations': pca.last['iterations'],
              'operator_s': pca.last['operator_time'], 'sigma0': float(pca.last['sigma'][0])})
        del a


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--shapes', default='62500x40000x32,62500x40000x128,62500x40000x1000,20000x20000x128')
    p.add_argument('--reps', type=int, default=20)
    p.add_argument('--panel', type=int, default=128)
    p.add_argument('--no-float', action='store_true')
    p.add_argument('--e2e', default='')
    a = p.parse_args()
    _lib.lib(0)
    shapes = [tuple(int(v) for v in s.split('x')) for s in a.shapes.split(',') if s]
    held = None
    for (M, N, m) in shapes:
        if held is None or held[0] != (M, N):
            held = None
            rng = np.random.default_rng(1)
            A8 = rng.integers(0, 256, size=(M, N), dtype=np.uint8)
            t0 = time.time()
            ops = [('bytes', ByteMatrix(A8), 1)]
            _lib.synchronize()
            emit({'what': 'create', 'path': 'bytes', 'rows': M, 'cols': N, 'seconds': time.time() - t0,
                  'device_bytes': ops[0][1].device_bytes()})
            if not a.no_float:
                A32 = A8.astype(np.float32)
                t0 = time.time()
                ops.append(('float32', Matrix(A32), 4))
                _lib.synchronize()
                emit({'what': 'create', 'path': 'float32', 'rows': M, 'cols': N, 'seconds': time.time() - t0,
                      'device_bytes': int(M) * ops[1][1].lda() * 4})
                del A32
            held = ((M, N), ops)
        products(A8, held[1], m, a.reps, a.panel)
        emit({'what': 'memory', 'rows': M, 'cols': N, 'm': m, 'bytes_device_bytes': held[1][0][1].device_bytes(),
              'bytes_workspace_bytes': held[1][0][1].workspace_bytes()})
    held = None
    if a.e2e:
        M, N = (int(v) for v in a.e2e.split('x'))
        from raleigh_amd.synthetic import byte_images
        end_to_end(byte_images(M, N, 100, seed=1), not a.no_float)


if __name__ == '__main__':
    main()
