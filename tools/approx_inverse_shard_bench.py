"""ShardedApproximateInverse on ONE GPU with forced collectives (one rank on RCCL, the shard cut into two virtual
ranks, both halo exchanges of every application as sends to self), float64, against what the same run measures for

  application  ApproximateInverse(work=...) on the whole matrix, for each work form: the difference is the price of the
               two self-exchanges (pack, send / receive, assemble / place) on top of the same two products.  Per call:
               HIP events (rlh_timer_start / rlh_timer_stop on the stream that carries the kernels and the collectives)
               around --calls calls, and the host wall time of the same calls with the stream drained at both ends
  solve        partial_hevp(which=10, tol=1e-6) on the row-sharded operator with T = the sharded approximate inverse (each
               work form), the sharded ChebyshevPreconditioner (ratio=300, degree=10, the arguments of
               tests/test_dist_gpu.py) and T = True: iterations and seconds; and the iterations of the UNSHARDED
               ApproximateInverse on the plain operator, recorded next to them (at level 1 G is the same matrix and only
               the order of the roundings differs)

on lap3d 64^3 at levels 1 and 3 and on the config-3 FE surrogate at level 1.  Every timing is repeated --repeats times after
a warm-up and reported as fastest .. slowest; "A beats B" means A's slowest repeat is faster than B's fastest, anything
else is "no winner".  Nothing here is a threshold, and nothing here says anything about more than one GPU.

    python tools/approx_inverse_shard_bench.py [--out profiles/r18_approx_inverse_sharded.txt] [--m 16] [--calls 20]
                                               [--repeats 5] [--lap 64] [--no-resources]

--update runs another leg INSTEAD: construction against update_values on re-valued copies of the matrix taking turns in
one run (construct on A_0, update to A_1, construct on A_1, update to A_2, ...: `revalued` below is the recipe of
tests/_fsai_values_cases.py), work='native', on lap3d and the config-3 surrogate at levels 1, 2, 3 and levels=1 with
steps=4, step_size=4; host wall seconds with the stream drained at both ends, fastest .. slowest of --repeats after a
warm-up round, the comparison being the construction of the same run; construction with updatable=False next to them.

    python tools/approx_inverse_shard_bench.py --update [--out profiles/r25_approx_inverse_shard_update.txt] [--repeats 5]
"""
import argparse
import ctypes
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def resource_lines():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'kernel_resources.py'), 'fsai_apply'], capture_output=True, text=True)
    out = ['== tools/kernel_resources.py fsai_apply (-Rpass-analysis=kernel-resource-usage; scr = scratch bytes per lane, occ = waves per SIMD)']
    return out + ['   ' + ln for ln in (r.stdout.strip().splitlines() or ['(no compiler here: %s)' % r.stderr.strip()[-200:]])]


def revalued(A, seed):
    """tests/_fsai_values_cases.py's recipe: every stored off-diagonal entry of the upper triangle times a factor uniform in
    [0.5, 1), every diagonal entry times one in [1, 2), the lower triangle mirrored; the structure is unchanged and a
    diagonally dominant matrix stays so."""
    import scipy.sparse as sp
    n = A.shape[0]
    rng = np.random.default_rng(seed)
    u = sp.triu(A, format='coo')
    factor = np.where(u.row == u.col, rng.uniform(1.0, 2.0, u.nnz), rng.uniform(0.5, 1.0, u.nnz)).astype(A.real.dtype)
    up = sp.csr_matrix((u.data * factor, (u.row, u.col)), shape=(n, n))
    B = sp.csr_matrix(up + sp.triu(up, k=1).conj().T).astype(A.dtype)
    B.sort_indices()
    return B


def update_leg(args, say, span, verdict, comm):
    import scipy.sparse as sp
    from raleigh_amd import _lib
    from raleigh_amd.algebra.hip.dist import ShardedApproximateInverse
    from raleigh_amd.synthetic import lap3d_rows, fe_surrogate
    L = _lib.lib()
    side = args.lap
    lap = lambda: lap3d_rows(side, side, side, 1.0, 1.01, 1.02, 0, side ** 3)
    configs = [('levels=%d' % lv, dict(levels=lv)) for lv in (1, 2, 3)] + [('levels=1, steps=4, step_size=4', dict(steps=4, step_size=4))]

    def timed(f):
        _lib.check(L.rlh_sync())
        t0 = time.perf_counter()
        out = f()
        _lib.check(L.rlh_sync())
        return time.perf_counter() - t0, out
    for title, make in (('lap3d %d^3' % side, lap), ('config-3 FE surrogate', fe_surrogate)):
        A = sp.csr_matrix(make().astype(np.float64))
        A.sort_indices()
        n = A.shape[0]
        copies = [revalued(A, 200 + k) for k in range(args.repeats + 2)]
        say('== %s: n = %d, nnz = %d (%.1f per row)' % (title, n, A.nnz, A.nnz / n))
        for name, kw in configs:
            build, plain, update, device = [], [], [], []
            for k in range(args.repeats + 1):                  # (round 0 is the warm-up)
                tb, T = timed(lambda: ShardedApproximateInverse(copies[k], comm, work='native', updatable=True, **kw))
                tp, P = timed(lambda: ShardedApproximateInverse(copies[k], comm, work='native', **kw))
                tu, _ = timed(lambda: T.update_values(copies[k + 1]))
                sec = ctypes.c_double()
                _lib.check(L.rlh_shardvalues_info(T._plan, None, ctypes.byref(sec)))
                if k:
                    build.append(tb), plain.append(tp), update.append(tu), device.append(sec.value * 1e3)
                nnz, extra = T.nnz, T.device_bytes() - P.device_bytes()
                del T, P
            say('   %-32s nnz(G) = %d (%.1f per row); updatable=True holds %.1f MB more' % (name, nnz, nnz / n, extra / 1e6))
            say('      construction updatable=True   %s s' % span(build))
            say('      construction updatable=False  %s s' % span(plain))
            say('      update_values                 %s s (the refill of the plan: %s ms on the stream)' % (span(update), span(device, '%.3f')))
            say('      ' + verdict('update_values', 'construction (updatable=True)', update, build))
            say('      ' + verdict('construction updatable=True', 'construction updatable=False', build, plain))
            say('      fastest against fastest: construction / update = %.1f' % (min(build) / min(update)))
        say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--update', action='store_true', help='the construction-against-update leg instead of the application and the solves')
    ap.add_argument('--out', default=None)
    ap.add_argument('--m', type=int, default=16)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--lap', type=int, default=64)
    ap.add_argument('--no-resources', action='store_true', help='skip the compiler\'s resource lines (needs hipcc)')
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, 'profiles', 'r25_approx_inverse_shard_update.txt' if args.update else 'r18_approx_inverse_sharded.txt')
    import torch
    import torch.distributed as dist
    import scipy.sparse as sp
    from raleigh_amd import _lib
    from raleigh_amd.algebra.hip import Vectors
    from raleigh_amd.algebra.hip.dist import Comm, ShardedApproximateInverse, ShardedSparseMatrix, ShardedVectors
    from raleigh_amd.algebra.hip.precond import ApproximateInverse, ChebyshevPreconditioner, gershgorin_upper_bound
    from raleigh_amd.interfaces import partial_hevp
    from raleigh_amd.core.solver import Options
    from raleigh_amd.synthetic import lap3d_rows, fe_surrogate
    assert torch.cuda.is_available(), 'this tool measures on the GPU'
    L = _lib.lib()
    for key, value in (('MASTER_ADDR', '127.0.0.1'), ('MASTER_PORT', '29581'), ('RANK', '0'), ('WORLD_SIZE', '1')):
        os.environ[key] = value
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', device_id=torch.device('cuda', 0))
    comm = Comm(force_collectives=True)
    m = args.m
    out_file = open(args.out, 'w')

    def say(text=''):
        print(text, flush=True)
        out_file.write(text + '\n')
        out_file.flush()

    def span(ts, fmt='%.4f'):
        return (fmt + ' .. ' + fmt) % (min(ts), max(ts))

    def verdict(a, b, ta, tb):
        if max(ta) < min(tb):
            return '%s beats %s (slowest %.4g < fastest %.4g)' % (a, b, max(ta), min(tb))
        if max(tb) < min(ta):
            return '%s loses to %s (fastest %.4g > slowest %.4g)' % (a, b, min(ta), max(tb))
        return 'no winner between %s and %s (the ranges overlap)' % (a, b)

    if args.update:
        say('# ShardedApproximateInverse(updatable=True): construction against update_values, forced collectives at ONE rank (two virtual')
        say('# ranks: the entries across the cut are packed, sent to self and received), float64, work=native')
        say('# %s, host wall seconds with the stream drained at both ends, %d repeats after a warm-up round, fastest .. slowest;'
            % (torch.cuda.get_device_name(0), args.repeats))
        say('# re-valued copies of the matrix take turns; written by tools/approx_inverse_shard_bench.py --update')
        say('# forced at one rank: nothing here is a measurement across GPUs')
        say()
        update_leg(args, say, span, verdict, comm)
        _lib.check(L.rlh_sync())
        torch.cuda.synchronize()
        dist.destroy_process_group()
        out_file.close()
        return
    say('# ShardedApproximateInverse with forced collectives at ONE rank (two virtual ranks, sends to self), float64, m = %d' % m)
    say('# %s, %d calls per timing, %d repeats after a warm-up, fastest .. slowest; written by tools/approx_inverse_shard_bench.py'
        % (torch.cuda.get_device_name(0), args.calls, args.repeats))
    say('# forced at one rank: nothing here is a measurement across GPUs')
    say('# the unsharded solves build their operator from the SciPy matrix inside the call: their iterations are what is compared')
    say()
    side = args.lap
    lap = lambda: lap3d_rows(side, side, side, 1.0, 1.01, 1.02, 0, side ** 3)
    cases = [('lap3d %d^3, levels=1' % side, lap, 1), ('lap3d %d^3, levels=3' % side, lap, 3), ('config-3 FE surrogate, levels=1', fe_surrogate, 1)]
    works = ('native', 'float32', 'bf16')
    ms = ctypes.c_float()
    for title, make, levels in cases:
        A = sp.csr_matrix(make().astype(np.float64))
        A.sort_indices()
        n = A.shape[0]
        say('== %s: n = %d, nnz = %d (%.1f per row)' % (title, n, A.nnz, A.nnz / n))
        sharded = {w: ShardedApproximateInverse(A, comm, levels=levels, work=w) for w in works}
        whole = {w: ApproximateInverse(A, levels=levels, work=w) for w in works}
        T0 = sharded['native']
        say('   set-up  sharded: %.3f s host wall (SciPy, the device builder, the plan); nnz(G) = %d (%.1f per row, longest row %d); halo '
            'rows per application: %d of x, %d of W (%.2f %% and %.2f %% of n)'
            % (T0.setup_seconds, T0.nnz, T0.nnz / n, T0.longest_row, *T0.halo_rows(), 100.0 * T0.halo_rows()[0] / n, 100.0 * T0.halo_rows()[1] / n))
        assert T0.nnz == whole['native'].nnz
        # ---- application
        B, X = Vectors(n, m), Vectors(n, m)
        B.fill_random()
        SB, SX = ShardedVectors(n, m, np.float64, comm=comm), ShardedVectors(n, m, np.float64, comm=comm)
        SB.fill_random()
        ops = [('sharded work=%s' % w, sharded[w], SB, SX) for w in works] + [('whole   work=%s' % w, whole[w], B, X) for w in works]
        for _, op, b, x in ops:
            for _ in range(3):
                op.apply(b, x)
        _lib.check(L.rlh_sync())
        dev_ms, wall_ms = {name: [] for name, _, _, _ in ops}, {name: [] for name, _, _, _ in ops}
        for _ in range(args.repeats):
            for name, op, b, x in ops:
                _lib.check(L.rlh_sync())
                t0 = time.perf_counter()
                _lib.check(L.rlh_timer_start())
                for _ in range(args.calls):
                    op.apply(b, x)
                _lib.check(L.rlh_timer_stop(ctypes.byref(ms)))
                _lib.check(L.rlh_sync())
                wall_ms[name].append((time.perf_counter() - t0) * 1e3 / args.calls)
                dev_ms[name].append(ms.value / args.calls)
        for name, op, _, _ in ops:
            nb = op.algorithmic_bytes(m)
            say('   apply   %-24s %s ms per call on the stream, %s ms host wall; %.1f MB algorithmic -> %.0f GB/s at the fastest'
                % (name, span(dev_ms[name]), span(wall_ms[name]), nb / 1e6, nb / min(dev_ms[name]) / 1e6))
        for w in works:
            a, b = 'sharded work=%s' % w, 'whole   work=%s' % w
            say('           the two self-exchanges: +%.4f ms per call on the stream, fastest against fastest (%.0f %%); %s'
                % (min(dev_ms[a]) - min(dev_ms[b]), 100.0 * (min(dev_ms[a]) / min(dev_ms[b]) - 1), verdict(a, b, dev_ms[a], dev_ms[b])))
        # ---- solve on the row-sharded operator
        op = ShardedSparseMatrix(A, comm)
        mk = lambda nn, data_type: ShardedVectors(nn, 0, data_type, comm=comm)
        cheb = ChebyshevPreconditioner(op, gershgorin_upper_bound(A), ratio=300.0, degree=10)
        solves, its = {}, {}
        runs = [('sharded ApproximateInverse work=%s' % w, dict(T=sharded[w], operator=op, vectors=mk), None) for w in works]
        runs += [('sharded ChebyshevPreconditioner', dict(T=cheb, operator=op, vectors=mk), None),
                 ('sharded T = True (none)', dict(T=True, operator=op, vectors=mk), None)]
        runs += [('unsharded ApproximateInverse work=%s' % w, dict(T=whole[w]), A) for w in works]
        for name, kw, a in runs:
            ts, status, lmd = [], None, None
            for rep in range(args.repeats + 1):                 # (the first run is the warm-up)
                np.random.seed(1)
                opt = Options()
                opt.max_iter = 5000
                _lib.check(L.rlh_sync())
                t0 = time.perf_counter()
                lmd, x, status = partial_hevp(a, which=10, tol=1e-6, verb=-1, opt=opt, **kw)
                _lib.check(L.rlh_sync())
                if rep:
                    ts.append(time.perf_counter() - t0)
                its[name] = partial_hevp.last['iterations'] if status is not None and status >= 0 else -1
            solves[name] = ts
            say('   solve   T = %-42s %s s, %d iterations, status %d, smallest eigenvalue %.10g'
                % (name, span(ts), its[name], status, lmd[0] if lmd is not None and len(lmd) else float('nan')))
        for w in works:
            a = 'sharded ApproximateInverse work=%s' % w
            for b in ('sharded ChebyshevPreconditioner', 'sharded T = True (none)'):
                say('           ' + verdict(a, b, solves[a], solves[b]))
            say('           iterations: %d sharded, %d unsharded (work=%s)' % (its[a], its['unsharded ApproximateInverse work=%s' % w], w))
        say()
        del sharded, whole, T0, op, cheb, runs, ops, B, X, SB, SX
    _lib.check(L.rlh_sync())
    torch.cuda.synchronize()
    dist.destroy_process_group()
    if not args.no_resources:
        for ln in resource_lines():
            say(ln)
    out_file.close()


if __name__ == '__main__':
    main()
