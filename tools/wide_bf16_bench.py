"""The bfloat16 Chebyshev step on the 256-row interleaved layout (wide_cheb_bf16_kernel) against the float32 fused
step on the SAME handle (wide_spmm_kernel<float, ..., CHEB>: what these operators ran before), m = 16 (GPU box).

  (i)   lap3d 215^3, float32, the operator built from a torch.sparse_csr tensor on the GPU -- and, for orientation,
        the bfloat16 step of the host-built handle of the same matrix (1024-row windowed layout / stacks)
  (ii)  the config-3 FE surrogate (raleigh_amd/synthetic.py), row-pair form -- and the same matrix without pairs
  (iii) the band of 31 entries per row, n = 215^3, built from a tensor generated on the GPU

Timing: HIP events (rlh_timer_start / rlh_timer_stop) around --calls launches of one kernel, after a warm-up of every
kernel on every shape; the kernels of a case take turns inside each of --repeats repeats; min and max of each are
reported.  A form is worth offering if the bfloat16 step's slowest repeat beats the float32 step's fastest repeat.
Byte model: per row and vector the float32 step moves 16 B (y, p, b read, p written) and the bfloat16 step 8 B; both
stream 6 B per stored entry slot and pass over the vectors (4 B value, 2 B position).
Then partial_hevp(which=10) on (i) from the tensor, float32 against bfloat16 work blocks (reported only).

    python tools/wide_bf16_bench.py [--out profiles/r09_wide_bf16.txt] [--side 215] [--calls 200] [--repeats 5] [--no-solve]
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

EXPLORE = [{'RLH_WIDE_VS': '1'}, {'RLH_WIDE_VS': '2'}, {'RLH_WIDE_NV': '8'}, {'RLH_WIDE_WG_PER_CU': '1'}]
COEFF = (1.3, -0.3, 0.01)          # p <- 1.3 y - 0.3 p + 0.01 (b - A y): repeated on the same blocks it stays bounded


def band_tensor(n, k, torch, device='cuda'):
    """The symmetric band of 2 k + 1 entries per row (values 1 / (1 + |offset|)), float32, generated on the GPU."""
    d = torch.arange(-k, k + 1, device=device, dtype=torch.int32)
    col = torch.arange(n, device=device, dtype=torch.int32).unsqueeze(1) + d.unsqueeze(0)
    ok = (col >= 0) & (col < n)
    crow = torch.zeros(n + 1, device=device, dtype=torch.int64)
    crow[1:] = torch.cumsum(ok.sum(dim=1), 0)
    val = (1.0 / (1.0 + d.abs().to(torch.float32))).unsqueeze(0).expand(n, -1)[ok]
    return torch.sparse_csr_tensor(crow.to(torch.int32), col[ok], val, size=(n, n))


def resource_lines():
    """What the compiler made of the new kernels (tools/kernel_resources.py: the -Rpass-analysis=kernel-resource-usage
    remarks of a gfx950 compile, one line per kernel)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'kernel_resources.py'), 'spmm_wide_bf16'],
                       capture_output=True, text=True)
    out = ['== tools/kernel_resources.py spmm_wide_bf16 (-Rpass-analysis=kernel-resource-usage; v / a = vector / accumulator '
           'registers, scr = scratch bytes per lane = private_segment_fixed_size, occ = waves per SIMD)']
    return out + ['   ' + ln for ln in (r.stdout.strip().splitlines() or ['(no compiler here: %s)' % r.stderr.strip()[-200:]])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r09_wide_bf16.txt'))
    ap.add_argument('--side', type=int, default=215)
    ap.add_argument('--m', type=int, default=16)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--no-solve', action='store_true')
    ap.add_argument('--explore', action='store_true', help='also time the bf16 step under the launcher\'s tunables')
    ap.add_argument('--no-resources', action='store_true', help='skip the compiler\'s resource lines (needs hipcc)')
    args = ap.parse_args()
    import torch
    import scipy.sparse as sp
    from raleigh_amd import _lib
    from raleigh_amd.algebra.hip import Vectors, SparseSymmetricMatrix
    from raleigh_amd.algebra.hip.sparse import Bf16Block
    from raleigh_amd.synthetic import lap3d_rows, fe_surrogate
    assert torch.cuda.is_available(), 'this tool measures on the GPU'
    L = _lib.lib()
    m = args.m
    out_file = open(args.out, 'w')

    def say(text=''):
        print(text, flush=True)
        out_file.write(text + '\n')
        out_file.flush()

    def tensor_of(A, dt):
        A = sp.csr_matrix(A.astype(dt))
        return torch.sparse_csr_tensor(torch.from_numpy(A.indptr.astype(np.int32)), torch.from_numpy(A.indices.astype(np.int32)),
                                       torch.from_numpy(A.data), size=A.shape).to('cuda')

    def device_bytes(op):
        nb = ctypes.c_int64()
        _lib.check(L.rlh_csr_info(op._SparseSymmetricMatrix__op._h, None, None, None, ctypes.byref(nb)))
        return nb.value

    def time_case(title, ops):
        """ops: [(label, operator, 'f32' | 'bf16')], all on the same n.  Returns {label: (min, max) ms per call}."""
        n = ops[0][1].size()
        say('== %s: n = %d, m = %d' % (title, n, m))
        y, p, b = (Vectors(n, m, data_type=np.float32) for _ in range(3))
        for v in (y, p, b):
            v.fill_random()
        y16, p16, b16 = (Bf16Block(n, m) for _ in range(3))
        for blk, v in ((y16, y), (p16, p), (b16, b)):
            blk.pack(v, 1.0)

        def call(op, kind):
            if kind == 'f32':
                op.cheb_step(y, p, b, *COEFF)
            elif kind == 'bf16':
                op.cheb_step_bf16(m, y16, p16, b16, *COEFF)
            else:                                                    # a bf16 call under the given environment
                os.environ.update(kind)
                op.cheb_step_bf16(m, y16, p16, b16, *COEFF)
                for k in kind:
                    del os.environ[k]
        if args.explore:                                             # the launcher's tunables, read at every launch
            first_bf16 = next(o for o in ops if o[2] == 'bf16')
            for env in EXPLORE:
                ops = ops + [('  bf16 ' + ' '.join('%s=%s' % kv for kv in env.items()), first_bf16[1], env)]
        for label, op, kind in ops:
            lay = op.layout()
            say('   %-44s layout %s, %d stored slots (%.2f per row), %d stacks, handle %.1f MB, supports_bf16 %s'
                % (label, lay[0], lay[1], lay[1] / n, lay[3], device_bytes(op) / 1e6, op.supports_bf16()))
            for _ in range(3):
                call(op, kind)                                       # warm-up of this kernel on this shape
        _lib.check(L.rlh_sync())
        ms = ctypes.c_float()
        times = {label: [] for label, _, _ in ops}
        for _ in range(args.repeats):
            for label, op, kind in ops:
                _lib.check(L.rlh_timer_start())
                for _ in range(args.calls):
                    call(op, kind)
                _lib.check(L.rlh_timer_stop(ctypes.byref(ms)))
                times[label].append(ms.value / args.calls)
        out = {}
        for label, op, kind in ops:
            slots = op.layout()[1] / n
            passes = 1                                               # (asserted below: the cases here stage m vectors at once)
            model = (16 if kind == 'f32' else 8) * m + 6 * slots * passes
            lo, hi = min(times[label]), max(times[label])
            out[label] = (lo, hi)
            say('   %-44s %8.4f .. %8.4f ms per call   model %5.0f B/row -> %6.0f GB/s at the fastest'
                % (label, lo, hi, model, model * n / lo / 1e6))
        return out

    def verdict(res, f32, bf16):
        ok = res[bf16][1] < res[f32][0]
        say('   %s: slowest bf16 repeat %.4f ms %s fastest float32 repeat %.4f ms; ratio of the fastest %.2fx'
            % ('CONDITION HOLDS' if ok else 'CONDITION FAILS', res[bf16][1], '<' if ok else '>=', res[f32][0],
               res[f32][0] / res[bf16][0]))
        say()

    assert m <= 16, 'the byte model below counts ONE pass over the entries: m <= 16, images of 16 vectors that fit the LDS'
    say('# bfloat16 Chebyshev step on the interleaved layout against the float32 fused step of the same handle')
    say('# byte model: (16 | 8) B per row and vector + 6 B per stored slot, ONE pass over the entries (m = %d <= 16: the images '
        'of 16 vectors of all three cases fit the LDS, no tunable is set)' % m)
    say('# %s, %d calls per timing, %d repeats, kernels alternated; written by tools/wide_bf16_bench.py'
        % (torch.cuda.get_device_name(0), args.calls, args.repeats))
    say()
    side = args.side
    n = side ** 3
    # ---- (i)
    t0 = time.time()
    A = lap3d_rows(side, side, side, 1.0, 1.01, 1.02, 0, n)
    t64 = tensor_of(A, np.float64)
    t32 = t64.to(torch.float32)
    op_t = SparseSymmetricMatrix(t32)
    op_h = SparseSymmetricMatrix(sp.csr_matrix(A.astype(np.float32)))
    say('(set-up of (i): %.1f s)' % (time.time() - t0))
    res = time_case('(i) lap3d %d^3 float32' % side,
                    [('float32 step, from the tensor', op_t, 'f32'), ('bf16 step, from the tensor', op_t, 'bf16'),
                     ('bf16 step, host-built (orientation)', op_h, 'bf16')])
    verdict(res, 'float32 step, from the tensor', 'bf16 step, from the tensor')
    del op_h
    # ---- (ii)
    F = fe_surrogate(dtype=np.float32)
    op_f = SparseSymmetricMatrix(F)
    os.environ['RLH_WIDE_PAIR'] = '0'
    op_f1 = SparseSymmetricMatrix(F)
    del os.environ['RLH_WIDE_PAIR']
    say('row pairs taken: %s (handle %.1f MB against %.1f MB without pairs)'
        % (device_bytes(op_f) < device_bytes(op_f1), device_bytes(op_f) / 1e6, device_bytes(op_f1) / 1e6))
    res = time_case('(ii) FE surrogate float32',
                    [('float32 step, row pairs', op_f, 'f32'), ('bf16 step, row pairs', op_f, 'bf16'),
                     ('float32 step, no pairs', op_f1, 'f32'), ('bf16 step, no pairs', op_f1, 'bf16')])
    verdict(res, 'float32 step, row pairs', 'bf16 step, row pairs')
    verdict(res, 'float32 step, no pairs', 'bf16 step, no pairs')
    del op_f, op_f1
    # ---- (iii)
    op_b = SparseSymmetricMatrix(band_tensor(n, 15, torch))
    res = time_case('(iii) band of 31 entries per row', [('float32 step', op_b, 'f32'), ('bf16 step', op_b, 'bf16')])
    verdict(res, 'float32 step', 'bf16 step')
    del op_b
    # ---- end to end
    if not args.no_solve:
        from raleigh_amd.interfaces import partial_hevp
        from raleigh_amd.core.solver import Options
        from raleigh_amd.algebra.hip.precond import ChebyshevPreconditioner
        from oracle.sparse import lap3d_eigenvalues
        ana = lap3d_eigenvalues(side, side, side, 1.0, 1.01, 1.02, 10)
        hi = 4.0 * sum(((side + 1.0) / a) ** 2 for a in (1.0, 1.01, 1.02))
        say('== partial_hevp(which=10, tol=1e-6) on the tensor of (i), Chebyshev(degree 32, ratio 7000) on the float32 operator')
        for storage in (None, 'bf16', None, 'bf16'):
            np.random.seed(1)
            opt = Options()
            opt.max_iter = 5000
            T = ChebyshevPreconditioner(None, hi, ratio=7000.0, degree=32, low_precision_op=op_t, storage=storage)
            _lib.check(L.rlh_sync())
            t0 = time.perf_counter()
            lmd, x, status = partial_hevp(t64, T=T, which=10, tol=1e-6, verb=-1, opt=opt)
            _lib.check(L.rlh_sync())
            el = time.perf_counter() - t0
            err = float(np.max(np.abs(lmd[:10] - ana) / ana)) if status == 0 else float('nan')
            say('   work blocks %-8s %7.3f s, %d iterations, status %d, max relative eigenvalue error %.1e'
                % (storage or 'float32', el, partial_hevp.last['iterations'], status, err))
        say()
    # ---- what the compiler made of the kernels
    if not args.no_resources:
        for ln in resource_lines():
            say(ln)
    out_file.close()


if __name__ == '__main__':
    main()
