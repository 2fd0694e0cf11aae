"""A sparse operator whose matrix already lies in device memory against the same matrix handed over from the host,
on the MI355X: what it costs to make the operator, to apply it, and to run partial_hevp end to end.  One JSON line per
case.

  python tools/device_operator_bench.py [--side 215] [--m 16] [--reps 10] [--which 10] [--no-lap] [--no-fe] [--no-solve]

lap3d side^3 (float64) and the config-3 surrogate (raleigh_amd.synthetic.fe_surrogate, float64):
  * SparseSymmetricMatrix(SciPy matrix) -- canonical form, checks, mirror and layout on the host threads, upload --
    against SparseSymmetricMatrix(the same matrix as a torch.sparse_csr tensor on the GPU) -- rlh_csr_create_device;
    best of two, wall clock with the stream synchronised; the device-to-host copy a tensor user would otherwise pay
    before the host path is timed separately;
  * one product of m vectors on each handle (HIP-event median of --reps calls after two warm-up calls), with the layout
    of each: the device build offers the interleaved and the sliced layout only, so on the stencil the host-built
    handle runs its stacked 1024-row windows and the ratio of the two product times is a figure of its own;
  * partial_hevp(which) end to end both ways, operator creation included: the Laplacian with a degree-32 Chebyshev
    preconditioner of the operator itself (nothing of a tensor input visits the host), the surrogate with the
    IncompleteLU preconditioner, which is set up from the SciPy matrix either way (its set-up is not in the times)."""

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from raleigh_amd import _lib  # noqa: E402
from raleigh_amd.algebra.hip import SparseSymmetricMatrix, Vectors  # noqa: E402
from raleigh_amd.synthetic import fe_surrogate, lap3d_rows  # noqa: E402


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


def as_tensor(A):
    import torch
    T = torch.sparse_csr_tensor(torch.from_numpy(A.indptr.astype(np.int64)), torch.from_numpy(A.indices.astype(np.int64)),
                                torch.from_numpy(A.data), size=A.shape).to('cuda')
    torch.cuda.synchronize()
    return T


def run(name, A, m, reps, which, precond, solve):
    import torch
    from raleigh_amd.core.solver import Options
    from raleigh_amd.interfaces import partial_hevp
    n = A.shape[0]
    T = as_tensor(A)
    rec = {'what': name, 'dtype': str(A.dtype), 'n': n, 'nnz': int(A.nnz), 'm': m}
    ops = {}
    for src, X in (('host', A), ('device', T)):
        best = None
        for _ in range(2):
            ops.pop(src, None)
            s, op = wall(lambda: SparseSymmetricMatrix(X))
            ops[src] = op
            best = s if best is None else min(best, s)
        rec['create_from_%s_s' % src] = best
        rec['layout_%s' % src] = ops[src].layout()[0]
        rec['stacks_%s' % src] = ops[src].layout()[3]
    t0 = time.perf_counter()
    T.cpu()
    rec['tensor_to_host_copy_s'] = time.perf_counter() - t0
    rng = np.random.default_rng(0)
    x = Vectors(rng.standard_normal((m, n)))
    y = Vectors(n, m, data_type=np.float64)
    out = {}
    for src in ('host', 'device'):
        med, lo, hi = event_median(lambda: ops[src].apply(x, y), reps)
        rec['apply_on_%s_built_s' % src] = med
        rec['apply_on_%s_built_min_max_s' % src] = [lo, hi]
        out[src] = y.data()
    rec['apply_device_over_host'] = rec['apply_on_device_built_s'] / rec['apply_on_host_built_s']
    scale = float(np.max(np.abs(out['host'])))
    rec['products_max_difference_rel'] = float(np.max(np.abs(out['host'] - out['device']))) / scale
    del ops, x, y, out
    if solve:
        for src, X in (('host', A), ('device', T)):
            opt = Options()
            opt.max_iter = 3000
            np.random.seed(1)
            _lib.synchronize()
            t0 = time.perf_counter()
            lmd, vec, status = partial_hevp(X, T=precond(X), which=which, tol=1e-6, verb=-1, opt=opt)
            if src == 'device':
                torch.cuda.synchronize()
            _lib.synchronize()
            rec['hevp_from_%s_s' % src] = time.perf_counter() - t0
            rec['hevp_from_%s_solve_s' % src] = partial_hevp.last['solve_time']
            rec['hevp_from_%s_iterations' % src] = int(partial_hevp.last['iterations'])
            rec['hevp_from_%s_status' % src] = int(status)
            rec['hevp_from_%s_lmd0' % src] = float(lmd[0])
            del vec
    emit(rec)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--side', type=int, default=215)
    p.add_argument('--m', type=int, default=16)
    p.add_argument('--reps', type=int, default=10)
    p.add_argument('--which', type=int, default=10)
    p.add_argument('--no-lap', action='store_true')
    p.add_argument('--no-fe', action='store_true')
    p.add_argument('--no-solve', action='store_true')
    a = p.parse_args()
    _lib.lib(0)
    from raleigh_amd.algebra.hip.precond import ChebyshevPreconditioner, IncompleteLU, gershgorin_upper_bound
    if not a.no_lap:
        s = a.side
        A = lap3d_rows(s, s, s, 1.0, 1.01, 1.02, 0, s ** 3)
        hi = gershgorin_upper_bound(A)
        # (the preconditioner's operator is built from the argument itself: on the device for a tensor)
        run('lap3d %d^3' % s, A, a.m, a.reps, a.which,
            lambda X: ChebyshevPreconditioner(SparseSymmetricMatrix(X), hi, ratio=7000.0, degree=32), not a.no_solve)
        del A
    if not a.no_fe:
        F = fe_surrogate()
        ilu = None
        if not a.no_solve:
            ilu = IncompleteLU(F)
            ilu.factorize()
        run('config-3 surrogate', F, a.m, a.reps, a.which, lambda X: ilu, not a.no_solve)


if __name__ == '__main__':
    main()
