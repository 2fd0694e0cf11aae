"""ApproximateInverse (factorised sparse approximate inverse, set up and applied on the GPU) against IncompleteLU
(host ILUT, triangular solves on the GPU) and no preconditioner, in the same run, float64 (GPU box):

  (i)  the config-3 FE surrogate (raleigh_amd/synthetic.py)      (ii) lap3d 64^3      -- the sizes of tools/ilu_bench.py
  (iii) the anisotropic 7-point Laplacian lap3d_rows(N, N, N, 1.0, 0.1, 0.01) at the --lap size (the arguments are mesh
       widths, the couplings 1, 100 and 10000: three values of |a_ij| / sqrt(a_ii a_jj), 0.495, 0.00495, 0.0000495)

  levels       --levels 1,2,3: one ApproximateInverse per level of fill (the pattern of that power of the lower triangle),
               each reported with its longest row, entries per row and truncated rows, next to IncompleteLU and no
               preconditioner
  adaptive     --adaptive LEVELS:STEPS:SIZE[,...]: one ApproximateInverse(levels=LEVELS, steps=STEPS, step_size=SIZE) each
               (the level pattern enriched on the GPU by Kaporin gradient), in the same run next to the --levels builds and
               measured the same way; the share of its set-up that the enrichment takes is what the set-up costs beyond
               that of the level pattern alone (device time, fastest against fastest)
  set-up       ApproximateInverse from a torch.sparse_csr tensor on the GPU: the device time the library reports
               (events around the whole build) and the host wall time; IncompleteLU.factorize on the same matrix
               (host wall time: ILUT on the host, then the set-up of the two triangular solves)
  application  milliseconds per call at m = 16: HIP events (rlh_timer_start / rlh_timer_stop) around --calls calls, the
               two preconditioners taking turns inside each of --repeats repeats; algorithmic GB/s at the fastest
  solve        partial_hevp(which=10, tol=1e-6) with T = ApproximateInverse, IncompleteLU, True: iterations and seconds
  work         --work native,float32,bf16: every ApproximateInverse above once more with each `work` (its own two-kernel
               application, W = G X kept in the matrix type, float32 or bfloat16), application and solve timed in the same
               run against the same build with work=None: "beats", "loses to" or "no winner" per line

  drop         --drop 0.01,0.02,...: every --levels and --adaptive build once more with each `drop` (post-filtration of the
               computed G by value, every row solved again on what is left), set-up, application and solve timed in the
               same run against the unfiltered build of the same pattern arguments -- and, with --work, each filtered
               build's plan against the unfiltered build's plan of the same work form

  prefilter    --prefilter 0.016,iii:0.01,...: every --levels and --adaptive build once more with each `prefilter` (the level
               pattern of the entries with |a_ij| >= prefilter sqrt(a_ii a_jj) alone), reported with its weak entries and
               measured like a --drop build against the build of the same pattern arguments without it (set-up,
               application, with --work each plan against the plan of the same work form, solve).  A value with a prefix
               i:, ii: or iii: is used on that matrix only; --matrices i,iii runs those matrices only

  update       --update: for every build above (and, with --work, its plan) the construction against `update_values` with
               re-valued copies of the same matrix (every off-diagonal entry of the upper triangle times a factor in
               [0.5, 1), every diagonal entry times one in [1, 2), the lower triangle mirrored: the structure stays, the
               matrix stays positive definite), taking turns in the same run: device seconds (events: the whole build /
               the whole update) and host wall seconds (with a plan: its creation / its refill included).  Then a
               sequence of five re-valued matrices solved with a fresh preconditioner each time against ONE preconditioner
               built on the first and updated for each: partial_hevp(which=10) seconds with the set-up of every step
               included, and the iterations of every step.  Stops after these lines.

Every timing is repeated --repeats times and reported as fastest .. slowest; "A beats B" means A's slowest repeat is
faster than B's fastest, anything else is "no winner".  Nothing here is a threshold.  --setup-only stops after the
set-up lines (for comparing two builds of the library on one machine).

    python tools/approx_inverse_bench.py [--out profiles/r11_approx_inverse_levels.txt] [--levels 1,2,3]
                                         [--adaptive 1:4:4,1:4:8,2:2:4] [--work native,float32,bf16] [--drop 0.01,0.02,0.05]
                                         [--prefilter i:0.016,i:0.02,iii:0.01,iii:0.1] [--matrices i,ii,iii]
                                         [--m 16] [--calls 20] [--repeats 5] [--setup-only] [--update [--sequence-repeats 5]]
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
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'kernel_resources.py'), 'fsai', 'fsai_apply'], capture_output=True,
                       text=True)
    out = ['== tools/kernel_resources.py fsai fsai_apply (-Rpass-analysis=kernel-resource-usage; scr = scratch bytes per lane)']
    return out + ['   ' + ln for ln in (r.stdout.strip().splitlines() or ['(no compiler here: %s)' % r.stderr.strip()[-200:]])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r11_approx_inverse_levels.txt'))
    ap.add_argument('--levels', default='1,2,3', help='levels of fill of ApproximateInverse, comma separated')
    ap.add_argument('--adaptive', default='', help='adaptive patterns as LEVELS:STEPS:SIZE, comma separated')
    ap.add_argument('--work', default='', help="work forms of the application ('native', 'float32', 'bf16'), comma separated")
    ap.add_argument('--drop', default='', help='post-filtration thresholds in (0, 1), comma separated')
    ap.add_argument('--prefilter', default='', help='prefiltration thresholds in (0, 1), comma separated; i:, ii: or iii: in front '
                                                    'of a value restricts it to that matrix')
    ap.add_argument('--matrices', default='i,ii,iii', help='the matrices to run, comma separated: i, ii, iii')
    ap.add_argument('--setup-only', action='store_true', help='set-up timings only')
    ap.add_argument('--update', action='store_true', help='construction against update_values, and a sequence of matrices')
    ap.add_argument('--sequence-repeats', type=int, default=None, help='repeats of the sequence of --update (default: --repeats)')
    ap.add_argument('--m', type=int, default=16)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--lap', type=int, default=64)
    ap.add_argument('--no-resources', action='store_true', help='skip the compiler\'s resource lines (needs hipcc)')
    args = ap.parse_args()
    levels = [int(v) for v in args.levels.split(',')]
    adaptive = [tuple(int(v) for v in spec.split(':')) for spec in args.adaptive.split(',') if spec]
    assert all(len(spec) == 3 for spec in adaptive), '--adaptive takes LEVELS:STEPS:SIZE'
    works = [w for w in args.work.split(',') if w]
    drops = [float(v) for v in args.drop.split(',') if v]
    prefilters = [(v.rpartition(':')[0], float(v.rpartition(':')[2])) for v in args.prefilter.split(',') if v]      # (matrix or '', value)
    assert all(tag in ('', 'i', 'ii', 'iii') for tag, _ in prefilters), '--prefilter takes values, or i:value, ii:value, iii:value'
    chosen = [v for v in args.matrices.split(',') if v]
    import torch
    import scipy.sparse as sp
    from raleigh_amd import _lib
    from raleigh_amd.algebra.hip import Vectors
    from raleigh_amd.algebra.hip.precond import ApproximateInverse, IncompleteLU
    from raleigh_amd.interfaces import partial_hevp
    from raleigh_amd.core.solver import Options
    from raleigh_amd.synthetic import lap3d_rows, fe_surrogate
    assert torch.cuda.is_available(), 'this tool measures on the GPU'
    L = _lib.lib()
    m = args.m
    out_file = open(args.out, 'w')

    def say(text=''):
        print(text, flush=True)
        out_file.write(text + '\n')
        out_file.flush()

    def span(ts, scale=1.0, fmt='%.3f'):
        return (fmt + ' .. ' + fmt) % (min(ts) * scale, max(ts) * scale)

    def beats(a, b, ta, tb):
        if max(ta) < min(tb):
            return '%s beats %s (slowest %.4g < fastest %.4g)' % (a, b, max(ta), min(tb))
        if max(tb) < min(ta):
            return '%s beats %s (slowest %.4g < fastest %.4g)' % (b, a, max(tb), min(ta))
        return 'no winner between %s and %s (the ranges overlap)' % (a, b)

    def verdict(a, b, ta, tb):
        if max(ta) < min(tb):
            return '%s beats %s (slowest %.4g < fastest %.4g)' % (a, b, max(ta), min(tb))
        if max(tb) < min(ta):
            return '%s loses to %s (fastest %.4g > slowest %.4g)' % (a, b, min(ta), max(tb))
        return 'no winner between %s and %s (the ranges overlap)' % (a, b)

    def device_tensor(M):
        out = torch.sparse_csr_tensor(torch.from_numpy(M.indptr.astype(np.int32)), torch.from_numpy(M.indices.astype(np.int32)),
                                      torch.from_numpy(M.data), size=M.shape).to('cuda')
        torch.cuda.synchronize()
        return out

    def revalued(M, seed):
        rng = np.random.default_rng(seed)
        u = sp.triu(M, format='coo')
        factor = np.where(u.row == u.col, rng.uniform(1.0, 2.0, u.nnz), rng.uniform(0.5, 1.0, u.nnz))
        up = sp.csr_matrix((u.data * factor, (u.row, u.col)), shape=M.shape)
        out = sp.csr_matrix(up + sp.triu(up, k=1).T)
        out.sort_indices()
        assert np.array_equal(out.indptr, M.indptr) and np.array_equal(out.indices, M.indices)
        return out

    def update_lines(A, t, kwargs, names):
        """--update: see the module docstring."""
        seq_repeats = args.sequence_repeats or args.repeats
        copies = [device_tensor(revalued(A, 100 + k)) for k in range(5)]

        def solve(mat, prec):
            np.random.seed(1)
            opt = Options()
            opt.max_iter = 5000
            lmd, x, status = partial_hevp(mat, T=prec, which=10, tol=1e-6, verb=-1, opt=opt)
            return partial_hevp.last['iterations'] if status is not None and status >= 0 else -1

        for kw, name in zip(kwargs, names):
            for w in [None] + works:
                label = name if w is None else '%s work=%s' % (name, w)
                build_dev, build_wall, upd_dev, upd_wall = [], [], [], []
                for r in range(args.repeats):               # construction and update take turns
                    _lib.check(L.rlh_sync())
                    t0 = time.perf_counter()
                    T = ApproximateInverse(t, work=w, **kw)
                    _lib.check(L.rlh_sync())
                    build_wall.append(time.perf_counter() - t0)
                    build_dev.append(T.setup_seconds)
                    t0 = time.perf_counter()
                    T.update_values(copies[r % len(copies)])
                    _lib.check(L.rlh_sync())
                    upd_wall.append(time.perf_counter() - t0)
                    upd_dev.append(T.update_seconds)
                    del T
                say('   update  %-42s construction device %s s, host wall %s s; update_values device %s s, host wall %s s'
                    % (label, span(build_dev, fmt='%.4f'), span(build_wall, fmt='%.4f'), span(upd_dev, fmt='%.4f'),
                       span(upd_wall, fmt='%.4f')))
                say('           ' + verdict('update_values', 'the construction', upd_dev, build_dev) + ' [device]')
                say('           ' + verdict('update_values', 'the construction', upd_wall, build_wall) + ' [host wall]')
                # ---- the sequence: a fresh preconditioner for every matrix against one that is updated
                fresh_s, kept_s, fresh_its, kept_its = [], [], None, None
                for _ in range(seq_repeats):
                    _lib.check(L.rlh_sync())
                    t0 = time.perf_counter()
                    fresh_its = [solve(c, ApproximateInverse(c, work=w, **kw)) for c in copies]
                    _lib.check(L.rlh_sync())
                    fresh_s.append(time.perf_counter() - t0)
                    t0 = time.perf_counter()
                    T = ApproximateInverse(copies[0], work=w, **kw)
                    kept_its = [solve(copies[0], T)]
                    for c in copies[1:]:
                        T.update_values(c)
                        kept_its.append(solve(c, T))
                    _lib.check(L.rlh_sync())
                    kept_s.append(time.perf_counter() - t0)
                    del T
                say('   sequence %-41s five matrices, set-up included: fresh each time %s s, iterations %s; built once and '
                    'updated %s s, iterations %s' % (label, span(fresh_s, fmt='%.4f'), fresh_its, span(kept_s, fmt='%.4f'), kept_its))
                say('           ' + verdict('built once and updated', 'fresh each time', kept_s, fresh_s) + ' [five solves with their set-ups]')

    say('# ApproximateInverse against IncompleteLU and no preconditioner, float64, m = %d' % m)
    say('# %s, %d calls per timing, %d repeats, fastest .. slowest; written by tools/approx_inverse_bench.py'
        % (torch.cuda.get_device_name(0), args.calls, args.repeats))
    say()
    side = args.lap
    cases = [('(i) config-3 FE surrogate', lambda: fe_surrogate()),
             ('(ii) lap3d %d^3' % side, lambda: lap3d_rows(side, side, side, 1.0, 1.01, 1.02, 0, side ** 3)),
             ('(iii) anisotropic lap3d %d^3 (1.0, 0.1, 0.01)' % side, lambda: lap3d_rows(side, side, side, 1.0, 0.1, 0.01, 0, side ** 3))]
    for title, make in cases:
        tag = title[1:title.index(')')]
        if tag not in chosen:
            continue
        A = sp.csr_matrix(make().astype(np.float64))
        A.sort_indices()
        n = A.shape[0]
        t = torch.sparse_csr_tensor(torch.from_numpy(A.indptr.astype(np.int32)), torch.from_numpy(A.indices.astype(np.int32)),
                                    torch.from_numpy(A.data), size=A.shape).to('cuda')
        torch.cuda.synchronize()
        say('== %s: n = %d, nnz = %d (%.1f per row)' % (title, n, A.nnz, A.nnz / n))
        # ---- set-up
        level_names = ['ApproximateInverse(levels=%d)' % lv for lv in levels]
        adaptive_names = ['ApproximateInverse(%d:%d:%d)' % spec for spec in adaptive]
        names = level_names + adaptive_names
        kwargs = [dict(levels=lv) if lv != 1 else {} for lv in levels]
        kwargs += [dict(levels=lv, steps=steps, step_size=size) for lv, steps, size in adaptive]
        plain_names = list(names)
        drop_names = []                                     # (name with drop, name of the unfiltered build)
        for kw, name in list(zip(kwargs, names)):
            for d in drops:
                kwargs.append(dict(kw, drop=d))
                names.append('%s drop=%g' % (name, d))
                drop_names.append((names[-1], name))
        for kw, name in list(zip(kwargs, names))[:len(plain_names)]:      # (measured like the --drop builds, against the same builds)
            for own, tau in prefilters:
                if own in ('', tag):
                    kwargs.append(dict(kw, prefilter=tau))
                    names.append('%s prefilter=%g' % (name, tau))
                    drop_names.append((names[-1], name))
        Ts, walls, devs = {}, {}, {}
        for kw, name in zip(kwargs, names):
            dev_s, wall_s = [], []
            T = None
            for _ in range(args.repeats):
                T = None
                t0 = time.perf_counter()
                T = ApproximateInverse(t, **kw)
                _lib.check(L.rlh_sync())
                wall_s.append(time.perf_counter() - t0)
                dev_s.append(T.setup_seconds)
            Ts[name], walls[name], devs[name] = T, wall_s, dev_s
            say('   set-up  %-29s device %s s, host wall %s s; nnz(G) = %d (%.1f per row, fill %.2f, longest row %d, '
                '%d rows cut%s), %.1f MB held' % (name, span(dev_s, fmt='%.4f'), span(wall_s, fmt='%.4f'), T.nnz, T.nnz / n, T.fill,
                                                  T.longest_row, T.truncated_rows,
                                                  (', %d entries dropped' % T.dropped_entries if T.drop else '')
                                                  + (', %d weak entries of A' % T.weak_entries if T.prefilter else ''), T.device_bytes() / 1e6))
        for dname, name in drop_names:
            say('           ' + verdict(dname, name, devs[dname], devs[name]) + ' [set-up, device]')
        for (lv, steps, size), name in zip(adaptive, adaptive_names):
            if lv in levels:
                plain = min(devs[level_names[levels.index(lv)]])
                say('           enrichment (%d steps of %d): %.0f %% of the set-up of %s (device, fastest %.4f s against %.4f s '
                    'for the level pattern alone)' % (steps, size, 100 * (1 - plain / min(devs[name])), name, min(devs[name]), plain))
        if args.setup_only:
            say()
            del T, Ts, t
            continue
        if args.update:
            del T, Ts
            update_lines(A, t, kwargs, names)
            say()
            del t
            continue
        # ---- the same builds with a plan of their own application
        work_names = []                                     # (name with work, name without)
        for kw, name in zip(kwargs, names):
            for w in works:
                wname = '%s work=%s' % (name, w)
                Ts[wname] = ApproximateInverse(t, work=w, **kw)
                work_names.append((wname, name))
                say('   plan    %-42s %.1f MB held with the plan (%.1f MB without)'
                    % (wname, Ts[wname].device_bytes() / 1e6, Ts[name].device_bytes() / 1e6))
        ilu, ilu_s = None, []
        for _ in range(args.repeats):
            ilu = None
            t0 = time.perf_counter()
            ilu = IncompleteLU(A)
            ilu.factorize()
            _lib.check(L.rlh_sync())
            ilu_s.append(time.perf_counter() - t0)
        say('   set-up  IncompleteLU.factorize        host wall %s s; fill %.2f, levels %s'
            % (span(ilu_s, fmt='%.4f'), ilu.fill, ilu.levels))
        for name in plain_names:
            say('           ' + beats(name, 'IncompleteLU', walls[name], ilu_s))
        # ---- application
        B, X = Vectors(n, m), Vectors(n, m)
        B.fill_random()
        ops = [(name, Ts[name], Ts[name].algorithmic_bytes(m)) for name in names + [wn for wn, _ in work_names]]
        ops.append(('IncompleteLU', ilu, ilu.chain().algorithmic_bytes(m)))
        for _, op, _ in ops:
            for _ in range(3):
                op.apply(B, X)
        _lib.check(L.rlh_sync())
        ms = ctypes.c_float()
        times = {name: [] for name, _, _ in ops}
        for _ in range(args.repeats):
            for name, op, _ in ops:
                _lib.check(L.rlh_timer_start())
                for _ in range(args.calls):
                    op.apply(B, X)
                _lib.check(L.rlh_timer_stop(ctypes.byref(ms)))
                times[name].append(ms.value / args.calls)
        for name, op, nb in ops:
            say('   apply   %-42s %s ms per call; %.1f MB algorithmic -> %.0f GB/s at the fastest'
                % (name, span(times[name], fmt='%.4f'), nb / 1e6, nb / min(times[name]) / 1e6))
        for name in plain_names:
            say('           ' + beats(name, 'IncompleteLU', times[name], times['IncompleteLU']))
        for wname, name in work_names:
            say('           ' + verdict(wname, name, times[wname], times[name]))
        # a filtered build against the unfiltered build of the same pattern arguments, for each form of the application
        filtered_pairs = list(drop_names) + [('%s work=%s' % (dname, w), '%s work=%s' % (name, w)) for dname, name in drop_names
                                             for w in works]
        for dname, name in filtered_pairs:
            say('           ' + verdict(dname, name, times[dname], times[name]))
        # ---- solve
        solves = {}
        for name, prec in ([(name, Ts[name]) for name in names + [wn for wn, _ in work_names]]
                           + [('IncompleteLU', ilu), ('True (none)', True)]):
            ts, its, status = [], None, None
            for _ in range(args.repeats):
                np.random.seed(1)
                opt = Options()
                opt.max_iter = 5000
                _lib.check(L.rlh_sync())
                t0 = time.perf_counter()
                lmd, x, status = partial_hevp(t, T=prec, which=10, tol=1e-6, verb=-1, opt=opt)
                _lib.check(L.rlh_sync())
                ts.append(time.perf_counter() - t0)
                its = partial_hevp.last['iterations'] if status is not None and status >= 0 else -1
            solves[name] = ts
            say('   solve   T = %-42s %s s, %d iterations, status %d, smallest eigenvalue %.10g'
                % (name, span(ts, fmt='%.4f'), its, status, lmd[0] if lmd is not None and len(lmd) else float('nan')))
        for name in plain_names:
            say('           ' + beats(name, 'IncompleteLU', solves[name], solves['IncompleteLU']))
            say('           ' + beats(name, 'no preconditioner', solves[name], solves['True (none)']))
        for wname, name in work_names:
            say('           ' + verdict(wname, name, solves[wname], solves[name]))
        for dname, name in filtered_pairs:
            say('           ' + verdict(dname, name, solves[dname], solves[name]))
        for name in level_names[1:]:
            say('           ' + beats(name, names[0], solves[name], solves[names[0]]))
        for name in adaptive_names:
            for other in level_names:
                say('           ' + beats(name, other, solves[name], solves[other]))
        # set-up and solve together: what a user who has the matrix on the GPU pays once
        both = lambda k: [a + b for a, b in zip(sorted(walls[k]), sorted(solves[k]))]
        for name in level_names[1:]:
            say('           set-up + solve: ' + beats(name, names[0], both(name), both(names[0])))
        for name in adaptive_names:
            for other in level_names:
                say('           set-up + solve: ' + beats(name, other, both(name), both(other)))
        say()
        del T, Ts, ilu, t
    if not args.no_resources and not args.setup_only:
        for ln in resource_lines():
            say(ln)
    out_file.close()


if __name__ == '__main__':
    main()
