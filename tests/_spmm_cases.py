"""The sparse product and the fused Chebyshev step, element by element, on every kernel path: the cases shared by the
CPU tier (tests/test_spmm_cpu.py over tests/fake_lib.py: shows that NumPy / SciPy in the working precision meets every
bound below and that every exact case is exact) and the GPU tier (tests/test_spmm_gpu.py over librlhip.so).  Everything
goes through the raw C ABI: rlh_csr_create / _upper / _device, rlh_spmm(_part), rlh_spmm_cheb(_part),
rlh_spmm_cheb_bf16(_part), rlh_gather_rows(_bf16), blocks by rlh_malloc / rlh_h2d / rlh_d2h.

Harness (`run`).  Every block is a host array of m + 2 columns of ld elements, uploaded whole; the call sees the window
of m columns from column 1, rows [0, extent).
  * The result (Y; P of the fused step): the window holds NaN before the plain product and p before the fused step;
    the two guard columns and rows [n_rows, ld) hold finite values that differ from position to position and must come
    back byte for byte.  A NaN in the window afterwards is a failure.
  * The inputs (X / y, the halo block H, B): NaN in the guard columns and in the rows past the extent, so a read past
    an operand that reaches a result is seen; all of them must come back bit-identical.
  * Every call is made twice on a re-uploaded result and must give the same bits.
  * After every call rlh_spmm_last_launch names the kernel that ran; every case states the family it is meant to reach
    (kernel, template parameters) and the harness asserts that every word of it is in the report, so a quiet fall-back
    to another kernel is a failure.  (The stand-in of the CPU tier answers `fake`: the case's own target is booked.)
Alignment legs: `aligned` (16-byte base, ld a multiple of 32 elements and >= extent + 7), `unaligned` (base shifted by
one element -- 8 bytes for complex128 --, ld odd; the bfloat16 entry points must return an error), `tight` (ld ==
extent: with n_cols % 8 != 0 the stacks must not be taken), `overhang` (n_cols % 8 != 0, ld >= n_cols + 7: the stacks
are taken and stage NaN rows that must reach no result).

Bounds.  u is the unit roundoff of the type's real part (2^-24, 2^-53).  They count roundings, they are not measurements.
  * Product, per real component: |got - ref| <= (L + 2) u S.  L = real products of the component = stored entries of
    the row, times 2 for complex; S = the sum of their absolute values in the reference precision.  Every kernel forms
    the component as a chain of L fused multiply-adds from 0 (fma_acc, common.h): L roundings, each of a partial sum
    bounded by S (1 + u)^L, so (L u + O(L^2 u^2)) S, which (L + 2) u S covers while L u < 0.01 (asserted per case).
    Zero-valued padding slots add exact zeros and no rounding.
  * Fused step p' = cy y + cp p + cb (b - t), t the product above: |got - ref| <= (L + 6) u T with
    T = |cy y| + |cp p| + |cb| (|b| + S).  Roundings beyond t's L: each coefficient into the type (3, each relative to
    its own term), b - t, cb (.), cy y, cp p, and the two sums -- with contraction some of these fuse and vanish.
    Relative to T every one of them is at most u (1 + small), and a product's own rounding and its coefficient's
    rounding act on the same term of T, so the count per term is: cy y 2, cp p 2, cb (b - t) 3 + L, the two sums 2 on
    partial sums <= T; the largest weight any single term of T carries is (L + 3) + 2 = L + 5 <= L + 6.
  * bfloat16 step: |got - r| <= u_bf (|r| + E) + E, r the longdouble value on the bfloat16 inputs, E the float32 bound
    above: the float32 value lies within E of r and is rounded once, nearest even.  u_bf is bfloat16's unit roundoff:
    8 significant bits, so 2^-8 -- half a unit in the last place of 2^-7.  (2^-9 cannot hold for a correctly rounded
    result: 1 + 2^-8 is a float32, E = 0, both neighbours 1 and 1 + 2^-7 are 2^-8 away; test_spmm_cpu.py shows it on
    oracle.ops.bf16_round itself.)
The reference of a bound case is formed from the uploaded values in numpy.longdouble (64-bit mantissa asserted), real and
imaginary parts separately.  Its work, nnz * m per case, is capped at BOUND_CAP = 400 000 products, which keeps one test
function's references within a few seconds; larger cases are exact-only.

Data.  Bound cases: Gaussian (`gauss`), and Gaussian with entry (i, j) of A scaled by 2^(-3 ((i + j) mod 12))
(`graded`), so that small couplings exist whose loss a norm would not see.  Exact cases (`exact`): integers uniform in
[-2, 2] (s, c, bfloat16) or [-2^14, 2^14] (d, z) in A, X, H, y, p, b and dyadic coefficients (1.25, -0.5, 0.75;
the bfloat16 step 1.25, -0.5, 0.71875, so that results need more than 8 bits and ties occur): every partial sum in any
order is exact -- asserted per case on 32 S, 32 T against 2^23 / 2^51 (the 32: five fractional bits of the
coefficients) -- and the result must equal the float64 / complex128 SciPy value BIT FOR BIT after -0 -> +0.  That is
what sees a dropped, doubled or misplaced entry, chunk, step, vector, block or stack; the in-place fused step applied
twice to a row gives other bits, so "every row exactly once" is tested by it too.

Empty rows.  A row without entries has no own column: the builders point its padding slots at position / column 0, so
it is +0 for finite X (asserted bit for bit wherever a matrix has one) and NaN where that element is not finite;
`empty_rows_nonfinite` pins "NaN or 0, nothing else, and no other row changes" per layout.  `foreign` sets one column of
X to +Inf: rows that reference it are non-finite, every other row with at least one entry keeps the bits of the clean run.
It runs on every family: the three layouts (product and fused step), the stacks (product; complex128 fused step) and the
three kernels of the bfloat16 step (+Inf is bfloat16 0x7F80).

Families (the table of `ratios_text`; every one the target of bound and exact cases):
  sell, sell cheb             sliced ELL, all four types            RLH_SPMM_FORMAT=sell; JT / TT / TPB / CHUNK
  well, well cheb             1024-row windowed, s d                =well; EPL 1 and 16 / sizeof(T); CPS; VEC
  stack reg                   stacks, register-staged, s d          RLH_SPMM_STACK=2 at creation (d: STACK_DMA=0)
  stack dma, stack dma cheb   stacks, LDS-DMA ring, all four / z    (s: STACK_DMA=2); PAT / DPAT at creation
  wide, wide cheb             256-row interleaved, all four         =wide; NV / VS / pairs / VEC
  well bf16, stack bf16, wide bf16    the bfloat16 step on float32 handles
Shapes are named from the kernels' constants (slice 64, blocks of 256 and 1024 rows, JT tiles, NV passes, the ring's
slots), never from the workload's sizes; m always includes 0 and 1.
"""

import ctypes

import numpy as np
import scipy.sparse as sp

from oracle import ops
from _columnwise_cases import DT, KEYS, base_shift, same_bytes, unit_roundoff

REAL = {'s': np.float32, 'd': np.float64, 'c': np.float32, 'z': np.float64}
BOUND_CAP = 400000
COEF_EXACT = (1.25, -0.5, 0.75)
COEF_EXACT_BF16 = (1.25, -0.5, 0.71875)
COEF_BOUND = (1.3, -0.45, 0.7)
U_BF16 = 2.0 ** -8
FAMILIES = ['sell', 'sell cheb', 'well', 'well cheb', 'stack reg', 'stack dma', 'stack dma cheb', 'wide', 'wide cheb',
            'well bf16', 'stack bf16', 'wide bf16']
SWITCHES = ('RLH_SPMM_FORMAT', 'RLH_SPMM_JT', 'RLH_SPMM_TT', 'RLH_SPMM_TPB', 'RLH_SPMM_CHUNK', 'RLH_SPMM_WG_PER_CU',
            'RLH_SPMM_CPS', 'RLH_SPMM_VEC', 'RLH_SPMM_STACK', 'RLH_SPMM_STACK_DMA', 'RLH_SPMM_STACK_PAT',
            'RLH_SPMM_STACK_DPAT', 'RLH_SPMM_STACK_ALIGN', 'RLH_SPMM_STACK_CHEB', 'RLH_SPMM_STACK_BF16',
            'RLH_SPMM_STACK_SINGLE', 'RLH_SPMM_BF16_VPS', 'RLH_SPMM_SCHED', 'RLH_SPMM_TILE', 'RLH_WIDE_NV', 'RLH_WIDE_VS',
            'RLH_WIDE_PAIR', 'RLH_WIDE_WG_PER_CU')

assert np.finfo(np.longdouble).nmant >= 63, 'the bound cases need a 64-bit mantissa reference'


# ---------------------------------------------------------------------------------------------------- the family table
RATIOS = {}          # (type, kernel family) -> [bound cases, largest error / bound seen, exact cases]


def table_family(text):
    w = text.split()
    name = w[0]
    if name == 'stack':
        assert len(w) > 1, 'a stack case names its kernel'
        name += ' ' + w[1]
    elif len(w) > 1 and w[1] == 'bf16':
        name += ' bf16'
    return name + (' cheb' if 'cheb=1' in w else '')


def ratios_text():
    lines = ['%-5s %-18s %6s %6s  %s' % ('', 'kernel family', 'bound', 'exact', 'largest error / bound')]
    worst = 0.0
    for (key, family), (count, ratio, exact) in sorted(RATIOS.items()):
        lines.append('%-5s %-18s %6d %6d  %s' % (key, family, count, exact, '%.3f' % ratio if count else '-'))
        worst = max(worst, ratio)
    lines.append('overall largest error / bound: %.3f' % worst)
    return '\n'.join(lines)


def _reached(key, family, ratio=None):
    r = RATIOS.setdefault((key, table_family(family)), [0, 0.0, 0])
    if ratio is None:
        r[2] += 1
    else:
        r[0] += 1
        r[1] = max(r[1], ratio)


def _L():
    from raleigh_amd import _lib
    return _lib


def native():
    """Whether the library under test is librlhip.so (and not the stand-in of the CPU tier)."""
    return isinstance(_L().library(), ctypes.CDLL)


def last_launch():
    lib = _L()
    buf = ctypes.create_string_buffer(160)
    lib.check(lib.lib().rlh_spmm_last_launch(buf, 160))
    return buf.value.decode()


def check_family(report, family, tag):
    """Every word of the case's target in the library's report, the kernel name first; returns the text to book."""
    if report == 'fake':
        return family
    words = report.split()
    want = family.split()
    assert words[0] == want[0] and all(w in words for w in want), 'launched "%s", the case is meant for "%s" %s' % (report, family, tag)
    return report


# ---------------------------------------------------------------------------------------------------- matrices
def draw(key, kind, shape, seed, bf16=False):
    """Values of the working type: `exact` integers, else Gaussian (bf16: rounded to bfloat16, as float32)."""
    rng = np.random.default_rng(seed)
    if kind == 'exact':
        r = 2 if (bf16 or key in 'sc') else 1 << 14
        v = rng.integers(-r, r + 1, shape).astype(np.float64)
        if key in 'cz' and not bf16:
            v = v + 1j * rng.integers(-r, r + 1, shape)
    else:
        v = rng.standard_normal(shape)
        if key in 'cz' and not bf16:
            v = v + 1j * rng.standard_normal(shape)
    if bf16:
        return ops.bf16_round(v.astype(np.float32))
    return v.astype(DT[key])


def _finish(key, n, ncols, rows, cols, kind, seed):
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    vals = draw(key, 'exact' if kind == 'exact' else 'gauss', rows.size, seed)
    if kind == 'exact':
        vals[vals == 0] = 1                 # (a stored zero would hide the loss of its entry)
    if kind == 'graded':
        vals = (vals * (2.0 ** (-3.0 * ((rows + cols) % 12))).astype(REAL[key])).astype(DT[key])
    a = sp.csr_matrix((vals, (rows, cols)), shape=(n, ncols), dtype=DT[key])
    a.sort_indices()
    assert a.nnz == rows.size, 'duplicate entries in a test matrix'
    return a


def ragged(key, n, lens, kind, seed=1, halo=0, halo_every=3):
    """n x (n + halo): row i has lens[i % len(lens)] entries (at most n) in a band around the diagonal; with a halo block
    every `halo_every`-th non-empty row has one more entry in a halo column."""
    rows, cols = [], []
    for i in range(n):
        k = min(lens[i % len(lens)], n)
        if k == 0:
            continue
        start = min(max(i - k // 2, 0), n - k)
        rows += [i] * k
        cols += range(start, start + k)
        if halo and i % halo_every == 0:
            rows.append(i)
            cols.append(n + (i // halo_every) % halo)
    return _finish(key, n, n + halo, rows, cols, kind, seed)


def far_windows(key, n, far_of_block, kind, seed=2, halo=0, rows_per_block=1024, stride=1024):
    """Row i couples to i, i + 1 and to i + stride j (mod n), j = 1 .. far_of_block[block of i]: a block of rows stages
    its own window and that many far ones (stride = 1024: windows of about 1024 columns, 16 - 17 groups of 64 each)."""
    rows, cols = [], []
    for i in range(n):
        k = far_of_block[(i // rows_per_block) % len(far_of_block)]
        c = {i, min(i + 1, n - 1)} if k < 7 else {i}
        for j in range(1, k + 1):
            c.add((i + stride * j + i % 2) % n)        # (stride 1024: 1025 columns, 17 groups)
        if halo and i % 5 == 0 and len(c) < 8:
            c.add(n + (i // 5) % halo)
        rows += [i] * len(c)
        cols += sorted(c)
    return _finish(key, n, n + halo, rows, cols, kind, seed)


def stencil(key, nx, ny, nz, kind, seed=3):
    """The 7-point pattern on an nx x ny x nz grid (x fastest) with constant coefficients per direction -- a few dozen
    distinct rows of values, which is what the stacks' value dictionary takes; `graded` has 12 times as many.  Complex:
    Hermitian with a skew imaginary part."""
    rng = np.random.default_rng(seed)
    cx = key in 'cz'
    if kind == 'exact':
        r = 2 if key in 'sc' else 1 << 14
        co = rng.integers(1, r + 1, 4).astype(np.float64) * rng.choice([-1.0, 1.0], 4)
        im = rng.integers(1, r + 1, 3).astype(np.float64)
    else:
        co, im = rng.standard_normal(4), rng.standard_normal(3)

    def line(nn, c, s):
        off = np.full(nn - 1, c + (1j * s if cx else 0.0))
        return sp.diags([np.conj(off), off], [-1, 1], shape=(nn, nn))
    ix, iy, iz = sp.identity(nx), sp.identity(ny), sp.identity(nz)
    a = (sp.kron(iz, sp.kron(iy, line(nx, co[0], im[0]))) + sp.kron(iz, sp.kron(line(ny, co[1], im[1]), ix))
         + sp.kron(line(nz, co[2], im[2]), sp.kron(iy, ix)) + co[3] * sp.identity(nx * ny * nz))
    a = sp.csr_matrix(a).astype(DT[key])
    a.sort_indices()
    if kind == 'graded':
        rows = np.repeat(np.arange(a.shape[0]), np.diff(a.indptr))
        a.data = (a.data * (2.0 ** (-3.0 * ((rows + a.indices) % 12))).astype(REAL[key])).astype(DT[key])
    return a


def paired(key, nodes, odd, kind, seed=4):
    """Two unknowns per node, 9 nodes coupled per node: 18 entries in (nearly) every row, consecutive rows of a node share
    their column pattern (the interleaved layout's row pairs); `odd`: one more row at the end."""
    n = 2 * nodes + (1 if odd else 0)
    rows, cols = [], []
    for i in range(n):
        node = i // 2
        first = min(max(node - 4, 0), max(nodes - 9, 0))
        c = [2 * q + d for q in range(first, min(first + 9, nodes)) for d in (0, 1)]
        if i == 2 * nodes:
            c = [i - 2, i - 1, i]
        rows += [i] * len(c)
        cols += c
    return _finish(key, n, n, rows, cols, kind, seed)


# ---------------------------------------------------------------------------------------------------- handles, blocks
class Handle:
    """One operator handle built from the SciPy matrix `a` (the switches read at creation are the caller's)."""

    def __init__(self, key, a, kind, how='create', bits=32):
        lib = _L()
        L = lib.lib()
        self.key, self.a, self.kind = key, a, kind
        self.n_rows, self.n_cols = a.shape
        self.indptr = np.ascontiguousarray(a.indptr, dtype=np.int64)
        self.lens = np.diff(self.indptr)
        src = a if how == 'create' else sp.csr_matrix(sp.triu(a, format='csr'))
        src.sort_indices()
        ip = np.ascontiguousarray(src.indptr, dtype=np.int64)
        ix = np.ascontiguousarray(src.indices, dtype=np.int32)
        va = np.ascontiguousarray(src.data, dtype=DT[key])
        h = ctypes.c_void_p()
        code = lib.dtype_code(DT[key])
        if how == 'create':
            lib.check(L.rlh_csr_create(ctypes.byref(h), code, self.n_rows, self.n_cols, lib.host_ptr(ip), lib.host_ptr(ix),
                                       lib.host_ptr(va)))
        elif how == 'upper':
            lib.check(L.rlh_csr_create_upper(ctypes.byref(h), code, self.n_rows, lib.host_ptr(ip), lib.host_ptr(ix),
                                             lib.host_ptr(va)))
        else:                               # 'device' (the full matrix) / 'device_upper' (mirror_upper = 1)
            from raleigh_amd.algebra.hip.memory import DeviceBuffer
            full = how == 'device'
            s2 = a if full else src
            if not full:                    # the stored structure must be symmetric: the lower triangle with other values
                low = sp.csr_matrix(sp.tril(a, k=-1, format='csr'))
                low.data = low.data * 0 + 77
                s2 = sp.csr_matrix(src + low)
                s2.sort_indices()
            it = np.int32 if bits == 32 else np.int64
            arrs = [np.ascontiguousarray(s2.indptr, dtype=it), np.ascontiguousarray(s2.indices, dtype=it),
                    np.ascontiguousarray(s2.data, dtype=DT[key])]
            bufs = []
            for arr in arrs:
                b = DeviceBuffer(max(arr.nbytes, 16), zero=False)
                lib.check(L.rlh_h2d(b.ptr, lib.host_ptr(arr), arr.nbytes))
                bufs.append(b)
            lib.check(L.rlh_csr_create_device(ctypes.byref(h), code, self.n_rows, self.n_cols, bits, bufs[0].ptr, bufs[1].ptr,
                                              bufs[2].ptr, 0 if full else 1))
        self.h = h

    def layout(self):
        lib = _L()
        lay, stored, ratio = ctypes.c_int(-1), ctypes.c_int64(0), ctypes.c_double(0)
        lib.check(lib.lib().rlh_csr_layout(self.h, ctypes.byref(lay), ctypes.byref(stored), ctypes.byref(ratio)))
        return lay.value

    def stacks_info(self):
        """(stacks, staged elements per row unstacked, stacked) of rlh_csr_stacks."""
        lib = _L()
        st, a, b = ctypes.c_int64(0), ctypes.c_double(0), ctypes.c_double(0)
        lib.check(lib.lib().rlh_csr_stacks(self.h, ctypes.byref(st), ctypes.byref(a), ctypes.byref(b)))
        return st.value, round(a.value, 6), round(b.value, 6)

    def stacks(self):
        lib = _L()
        st, a, b = ctypes.c_int64(0), ctypes.c_double(0), ctypes.c_double(0)
        lib.check(lib.lib().rlh_csr_stacks(self.h, ctypes.byref(st), ctypes.byref(a), ctypes.byref(b)))
        return st.value

    def bf16_ready(self, n_own, ldh):
        lib = _L()
        ok = ctypes.c_int(-1)
        lib.check(lib.lib().rlh_csr_bf16_ready(self.h, n_own, ldh, ctypes.byref(ok)))
        return ok.value

    def close(self):
        if self.h is not None:
            _L().lib().rlh_csr_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


BF16_NAN = np.uint16(0x7FC0)


def _nan_of(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.uint16:
        return BF16_NAN
    return complex(np.nan, np.nan) if dtype.kind == 'c' else np.nan


def _ramp(dtype, count, which):
    """Finite values that differ from position to position."""
    dtype = np.dtype(dtype)
    k = np.arange(count, dtype=np.int64) + 977 * which
    if dtype == np.uint16:
        return (0x3F80 + k % 1021).astype(np.uint16)                 # bfloat16 bits of 1 .. about 250
    r = ((k % 8191) + 1) * 0.5
    return (r - 1j * r[::-1] if dtype.kind == 'c' else r).astype(dtype)


def leading_dimension(leg, extent, dtype, which):
    es = np.dtype(dtype).itemsize
    if leg == 'tight':
        return max(extent, 1)
    if leg == 'unaligned':
        return (extent + 3 + 2 * which) | 1
    if leg == 'overhang':
        unit = max(16 // es, 1)
        return (extent + 7 + unit - 1) // unit * unit
    return (extent + 7 + which + 31) // 32 * 32


class Blk:
    """(m + 2) columns of ld elements: the window (columns 1 .. m, rows [0, n)) holds `window` (None: NaN), everything
    else NaN (`outside` = 'nan': an input) or finite values that differ from position to position ('ramp': a result)."""

    def __init__(self, dtype, n, m, leg, which, window, outside):
        from raleigh_amd.algebra.hip.memory import DeviceBuffer
        self.dtype = np.dtype(dtype)
        self.n, self.m, self.es = n, m, self.dtype.itemsize
        self.ld = leading_dimension(leg, n, self.dtype, which)
        count = (m + 2) * self.ld
        if outside == 'nan':
            self.host = np.full((m + 2, self.ld), _nan_of(self.dtype), dtype=self.dtype)
        else:
            self.host = _ramp(self.dtype, count, which).reshape(m + 2, self.ld).copy()
        self.host[1:m + 1, :n] = _nan_of(self.dtype) if window is None else window
        self._buf = DeviceBuffer(self.host.nbytes + 32, zero=False)
        shift = base_shift(self.dtype, False) if leg == 'unaligned' else 0
        self.base = self._buf.ptr + shift
        self.upload()

    def upload(self):
        lib = _L()
        lib.check(lib.lib().rlh_h2d(self.base, lib.host_ptr(self.host), self.host.nbytes))

    def ptr(self):
        return self.base + self.ld * self.es

    def window(self):
        return self.host[1:self.m + 1, :self.n]

    def fetch(self):
        lib = _L()
        out = np.empty_like(self.host)
        lib.check(lib.lib().rlh_d2h(lib.host_ptr(out), self.base, out.nbytes))
        return out

    def unchanged(self, tag):
        assert same_bytes(self.fetch(), self.host), 'an input came back modified %s' % tag

    def result(self, tag):
        """The downloaded window; every byte outside it must be what was uploaded."""
        got = self.fetch()
        win = got[1:self.m + 1, :self.n].copy()
        got[1:self.m + 1, :self.n] = self.window()
        assert same_bytes(got, self.host), 'guard columns or rows past the result modified %s' % tag
        return win


# ---------------------------------------------------------------------------------------------------- references
def _parts(w, rtype=np.longdouble):
    w = np.asarray(w)
    if w.dtype.kind == 'c':
        return [w.real.astype(rtype), w.imag.astype(rtype)]
    return [w.astype(rtype)]


def _rowsum(contrib, indptr, n):
    """Sums of the rows' stretches of `contrib` (m, nnz) -> (m, n); empty rows give 0."""
    out = np.zeros((contrib.shape[0], n), dtype=contrib.dtype)
    nonempty = np.diff(indptr) > 0
    if nonempty.any() and contrib.shape[0]:
        out[:, nonempty] = np.add.reduceat(contrib, indptr[:-1][nonempty], axis=1)
    return out


def product_parts(h, x, avals=None):
    """Per real component of A x: (value, sum of the absolute values of its products), longdouble, (m, n_rows) each."""
    a = h.a
    av = _parts(a.data if avals is None else avals)
    xv = [p[:, a.indices] for p in _parts(x)]
    ip, n = h.indptr, h.n_rows
    if len(av) == 1:
        t = av[0][None, :] * xv[0]
        return [(_rowsum(t, ip, n), _rowsum(np.abs(t), ip, n))]
    rr, ii, ri, ir = av[0][None, :] * xv[0], av[1][None, :] * xv[1], av[0][None, :] * xv[1], av[1][None, :] * xv[0]
    return [(_rowsum(rr - ii, ip, n), _rowsum(np.abs(rr) + np.abs(ii), ip, n)),
            (_rowsum(ri + ir, ip, n), _rowsum(np.abs(ri) + np.abs(ir), ip, n))]


def reference(h, x, cheb, bf16=False):
    """(per real component: value, magnitude S or T, number of real products L of the row), all longdouble (m, n_rows).
    cheb: None or (y_own, p, b, (cy, cp, cb)) with the blocks' windows as (m, n_rows) arrays."""
    avals = h.a.data.astype(np.float32) if bf16 else None
    prod = product_parts(h, x, avals)
    L = h.lens.astype(np.longdouble)[None, :] * len(prod)
    if cheb is None:
        return [(t, s, L) for t, s in prod]
    y, p, b, (cy, cp, cb) = cheb
    cy, cp, cb = np.longdouble(cy), np.longdouble(cp), np.longdouble(cb)
    out = []
    for (t, s), yy, pp, bb in zip(prod, _parts(y), _parts(p), _parts(b)):
        out.append((cy * yy + cp * pp + cb * (bb - t), np.abs(cy * yy) + np.abs(cp * pp) + np.abs(cb) * (np.abs(bb) + s), L))
    return out


def _plus_zero(w):
    """-0 -> +0 in every real component."""
    r = np.ascontiguousarray(w).copy()
    v = r.view(REAL_OF[r.dtype.type])
    v += 0
    return r


REAL_OF = {np.float32: np.float32, np.float64: np.float64, np.complex64: np.float32, np.complex128: np.float64}


def verify(h, got, x, cheb, tag, family, bf16=False):
    """The window `got` (m, n_rows; bf16: float32 values of the stored bits) against the reference: bit for bit on exact
    data, per real component within the bound otherwise.  Books the case."""
    key = h.key
    ref = reference(h, x, cheb, bf16)
    u = unit_roundoff('s' if bf16 else key)
    rtype = np.float32 if bf16 else REAL[key]
    gp = _parts(got)
    assert not any(np.isnan(g).any() for g in gp), 'NaN in the result %s' % tag
    if h.kind == 'exact':
        limit = 2.0 ** (23 if (bf16 or key in 'sc') else 51)
        for val, mag, _ in ref:
            assert mag.size == 0 or 32 * mag.max() < limit, 'the case is not exact: magnitude %g %s' % (mag.max(), tag)
        want = [val.astype(np.float64) for val, _, _ in ref]
        if bf16:
            want = [ops.bf16_round(want[0].astype(np.float32))]
        for c, (g, w) in enumerate(zip(gp, want)):
            g, w = _plus_zero(g.astype(rtype)), _plus_zero(w.astype(rtype))
            if not same_bytes(g, w):
                bad = np.argwhere(g != w)
                j, i = bad[0]
                raise AssertionError('%d elements differ (component %d), first at (vector %d, row %d): %r, exact %r %s'
                                     % (len(bad), c, j, i, g[j, i], w[j, i], tag))
        _reached(key, family)
        return
    worst = 0.0
    for c, (g, (val, mag, L)) in enumerate(zip(gp, ref)):
        assert L.size == 0 or float(L.max()) * u < 0.01
        bound = (L + (2 if cheb is None else 6)) * u * mag
        if bf16:
            bound = U_BF16 * (np.abs(val) + bound) + bound
        err = np.abs(g.astype(np.longdouble) - val)
        bound = np.broadcast_to(bound, val.shape)
        bad = ~(err <= bound)
        if bad.any():
            j, i = np.argwhere(bad)[0]
            raise AssertionError('(vector %d, row %d, component %d): error %.3e above the bound %.3e %s'
                                 % (j, i, c, float(err[j, i]), float(bound[j, i]), tag))
        nz = bound > 0
        if nz.any():
            worst = max(worst, float((err[nz] / bound[nz]).max()))
    _reached(key, family, worst)


# ---------------------------------------------------------------------------------------------------- one case
def _bits(w):
    return ops.bf16_bits(np.ascontiguousarray(w, dtype=np.float32))


def run(h, m, family, cheb=False, bf16=False, n_own=None, leg='aligned', parts=(0,), seed=0, poison=None,
        expect_error=False, check=True):
    """One case on handle h: m vectors, the product or (cheb) the fused step, (bf16) on bfloat16 blocks; n_own < n_cols:
    columns from n_own on come from a halo block.  parts: (0,) the whole operator, or (1, 2): the two parts in turn, which
    must be disjoint and complete.  poison: (column, value) written into every vector at that column before the upload.
    Returns (window of the result as downloaded, the reports of the calls)."""
    lib = _L()
    L = lib.lib()
    key = h.key
    nr, nc = h.n_rows, h.n_cols
    n_own = nc if n_own is None else n_own
    nh = nc - n_own
    dt = np.uint16 if bf16 else DT[key]
    kind = h.kind if h.kind == 'exact' else 'gauss'
    tag = '[%s %s %dx%d m=%d n_own=%d %s %s parts=%s %s]' % (key, family, nr, nc, m, n_own, leg, h.kind, parts,
                                                            'cheb' if cheb else 'product')
    conv = _bits if bf16 else (lambda w: w)
    xs = draw(key, kind, (m, nc), 100 + seed, bf16)
    if poison is not None:
        xs[:, poison[0]] = poison[1]
    X = Blk(dt, n_own, m, leg, 0, conv(xs[:, :n_own]), 'nan')
    H = Blk(dt, nh, m, leg, 1, conv(xs[:, n_own:]), 'nan') if nh else None
    if cheb:
        ps, bs = draw(key, kind, (m, nr), 200 + seed, bf16), draw(key, kind, (m, nr), 300 + seed, bf16)
        Y = Blk(dt, nr, m, leg, 2, conv(ps), 'ramp')
        B = Blk(dt, nr, m, leg, 3, conv(bs), 'nan')
        coef = (COEF_EXACT_BF16 if bf16 else COEF_EXACT) if h.kind == 'exact' else COEF_BOUND
        ref_cheb = (xs[:, :nr], ps, bs, coef)
    else:
        Y = Blk(dt, nr, m, leg, 2, None, 'ramp')
        B, ref_cheb = None, None
    hp, hld = (H.ptr(), H.ld) if H else (None, 0)

    def call(part):
        if bf16:
            if part == 0 and H is None and nr == nc:
                rc = L.rlh_spmm_cheb_bf16(h.h, m, X.ptr(), X.ld, Y.ptr(), Y.ld, B.ptr(), B.ld, *coef)
            else:
                rc = L.rlh_spmm_cheb_bf16_part(h.h, part, m, X.ptr(), X.ld, n_own, hp, hld, Y.ptr(), Y.ld, B.ptr(), B.ld, *coef)
        elif cheb:
            if part == 0:
                rc = L.rlh_spmm_cheb(h.h, m, X.ptr(), X.ld, n_own, hp, hld, Y.ptr(), Y.ld, B.ptr(), B.ld, *coef)
            else:
                rc = L.rlh_spmm_cheb_part(h.h, part, m, X.ptr(), X.ld, n_own, hp, hld, Y.ptr(), Y.ld, B.ptr(), B.ld, *coef)
        elif part == 0:
            rc = L.rlh_spmm(h.h, m, X.ptr(), X.ld, n_own, hp, hld, Y.ptr(), Y.ld)
        else:
            rc = L.rlh_spmm_part(h.h, part, m, X.ptr(), X.ld, n_own, hp, hld, Y.ptr(), Y.ld)
        return rc

    if expect_error:
        if not native():
            return None, []                  # (the stand-in takes every alignment)
        rc = call(parts[0])
        assert rc != 0, 'the call was taken %s' % tag
        assert same_bytes(Y.result(tag), Y.window()), 'a refused call wrote %s' % tag
        return None, []

    def value(win):
        return ops.bf16_from_bits(win) if bf16 else win

    def written(win, before):
        """Per row: whether its bytes differ from `before`; a row is written in every vector or in none."""
        diff = (win.view(np.uint8).reshape(m, nr, -1) != before.view(np.uint8).reshape(m, nr, -1)).any(axis=2)
        return diff.any(axis=0), diff.all(axis=0)

    def once():
        """The calls of `parts` on the freshly uploaded result; returns (window, reports)."""
        Y.upload()
        lib.check(call(parts[0]))
        reports = [last_launch()]
        win1 = Y.result(tag)
        if parts == (0,):
            return win1, reports
        assert parts == (1, 2)
        if reports[0] == 'none':
            assert same_bytes(win1, Y.window()), 'a part with nothing to launch wrote %s' % tag
        if not cheb:
            Y.upload()                             # NaN again: the rows that part 2 leaves alone stay NaN
        lib.check(call(2))
        reports.append(last_launch())
        win2 = Y.result(tag)
        if reports[1] == 'none':
            assert same_bytes(win2, win1 if cheb else Y.window()), 'a part with nothing to launch wrote %s' % tag
        if m == 0:
            return win2, reports
        if cheb:
            # in place: after part 1 a row holds p or its final value in every vector, after part 2 the final value --
            # a row computed by both parts, or twice by one, has other bits than the reference
            is_p = ~written(win1, Y.window())[0]
            is_new = ~written(win1, win2)[0]
            assert (is_p | is_new).all(), 'part 1 left a row that is neither p nor the result %s' % tag
            return win2, reports
        any1, all1 = written(win1, Y.window())
        any2, all2 = written(win2, Y.window())
        assert (any1 == all1).all() and (any2 == all2).all(), 'a row written in some vectors only %s' % tag
        assert (any1 ^ any2).all(), 'the two parts are not disjoint and complete %s' % tag
        return np.where(any1[None, :], win1, win2), reports

    win, reports = once()
    if m == 0 or nr == 0:
        assert all(r in ('none', 'fake') for r in reports), 'something was launched for nothing %s' % tag
    live = [r for r in reports if r != 'none']
    booked = family
    if m and nr:
        assert live, 'nothing was launched %s' % tag
        for r in live:
            booked = check_family(r, family, tag)
    if check and m and nr and poison is None:
        verify(h, value(win), xs, ref_cheb, tag, booked, bf16)
    win2, reports2 = once()
    assert same_bytes(win, win2) and reports == reports2, 'the repeated call gave other bits %s' % tag
    X.unchanged(tag)
    for blk in (H, B):
        if blk is not None:
            blk.unchanged(tag)
    return value(win), reports


def empty_rows_zero(h, win):
    """Rows without entries are +0, bit for bit (finite X)."""
    empty = h.lens == 0
    if empty.any() and win.shape[0]:
        z = np.ascontiguousarray(win[:, empty])
        assert same_bytes(z, np.zeros(z.shape, dtype=z.dtype)), 'an empty row is not +0'


def foreign(h, m, family, column, **kw):
    """One column of X (or row of H) set to +Inf: rows that reference it are non-finite, every other row with at least one
    entry carries the bits of the clean run.  Some rows must reference it and some only stage it."""
    clean, _ = run(h, m, family, **kw)
    dirty, _ = run(h, m, family, poison=(column, np.inf), check=False, **kw)
    a = h.a.tocsr()
    refs = np.zeros(h.n_rows, dtype=bool)
    refs[np.repeat(np.arange(h.n_rows), h.lens)[a.indices == column]] = True
    others = ~refs & (h.lens > 0)
    assert refs.any() and others.any()
    assert not np.isfinite(dirty[:, refs]).any(), 'a row that references the poisoned column is finite'
    assert same_bytes(np.ascontiguousarray(dirty[:, others]), np.ascontiguousarray(clean[:, others])), \
        'the poisoned column reached a row that does not reference it (%s)' % family
    return clean, dirty


def empty_rows_nonfinite(h, m, family, **kw):
    """TODAY'S BEHAVIOUR, pinned: with a non-finite element at position 0 an empty row is NaN or 0, nothing else, and no
    row that does not reference column 0 changes."""
    assert (h.lens == 0).any()
    clean, dirty = None, None
    clean, _ = run(h, m, family, **kw)
    dirty, _ = run(h, m, family, poison=(0, np.inf), check=False, **kw)
    a = h.a.tocsr()
    refs = np.zeros(h.n_rows, dtype=bool)
    refs[np.repeat(np.arange(h.n_rows), h.lens)[a.indices == 0]] = True
    empty = h.lens == 0
    e = dirty[:, empty]
    ok = np.isnan(e) | (e == 0)
    assert ok.all(), 'an empty row is neither NaN nor 0'
    keep = ~refs & ~empty
    assert same_bytes(np.ascontiguousarray(dirty[:, keep]), np.ascontiguousarray(clean[:, keep])), 'another row changed'


# ---------------------------------------------------------------------------------------------------- the families
def clear(delenv):
    for name in SWITCHES:
        delenv(name, raising=False)


KINDS = ('gauss', 'graded', 'exact')


def handles(key, build, kinds=KINDS, **kw):
    """One handle per kind of data of the matrix `build(kind)`."""
    for kind in kinds:
        a = build(kind)
        with Handle(key, a, 'exact' if kind == 'exact' else 'bound', **kw) as h:
            yield kind, h


def fits(h, m):
    return h.kind == 'exact' or h.a.nnz * m <= BOUND_CAP


# ---- sliced ELL
SELL_N = [1, 63, 64, 65, 129, 300]
SELL_M = [0, 1, 4, 5, 8, 9, 16, 17, 32, 33]
SELL_LENS = [3, 1, 5, 0, 2, 7, 1]          # slice widths 5 and 7: no multiple of TT = 4, 8


def sell_lens(n):
    """Rows 64 .. 127 empty (a whole slice) where the matrix has them."""
    return [0 if 64 <= i < 128 else SELL_LENS[i % len(SELL_LENS)] for i in range(max(n, 1))]


def sell_family(key, m, cheb, jt_cap=16, tt=1, tpb=1):
    """The instantiation spmm_impl / launch_spmm document for these switches."""
    cx = key in 'cz'
    if m <= 4 or jt_cap <= 4:
        jt = 4
    elif m <= 8 or jt_cap <= 8:
        jt = 8
    elif m <= 16 or cx or jt_cap <= 16 or cheb:
        jt = 16
    else:
        jt = 32
    ntiles = (m + jt - 1) // jt
    t = 4 if ntiles >= 4 else (2 if ntiles >= 2 else 1)
    if t > tpb:
        t = 2 if tpb >= 2 else 1
    return 'sell jt=%d tt=%d tpb=%d cheb=%d' % (jt, 8 if tt >= 8 else (4 if tt >= 4 else 1), t, 1 if cheb else 0)


def sell(key, setenv, delenv, ns=SELL_N):
    clear(delenv)
    setenv('RLH_SPMM_FORMAT', 'sell')
    setenv('RLH_SPMM_CHUNK', '1')
    for n in ns:
        for halo in (0, 8):
            if halo and n not in (65, 300):
                continue
            for kind, h in handles(key, lambda kind: ragged(key, n, sell_lens(n), kind, halo=halo)):
                assert h.layout() in (0, 1)             # (the stand-in reports 1 for every handle)
                n_own = n if halo else None
                for cheb in (False, True):
                    for m in SELL_M:
                        win, _ = run(h, m, sell_family(key, m, cheb), cheb=cheb, n_own=n_own)
                        if not cheb and m:
                            empty_rows_zero(h, win)
                    if n != 300 or kind == 'gauss' or not halo:
                        continue
                    # every tile, register group and waves-per-slice instantiation, on the matrix of five slices
                    for jt in (4, 8, 16, 32):
                        for tt in (1, 4, 8):
                            for tpb in (1, 2, 4):
                                setenv('RLH_SPMM_JT', str(jt))
                                setenv('RLH_SPMM_TT', str(tt))
                                setenv('RLH_SPMM_TPB', str(tpb))
                                for m in (5, 17, 33):
                                    run(h, m, sell_family(key, m, cheb, jt, tt, tpb), cheb=cheb, n_own=n_own,
                                        leg='unaligned' if tt == 4 else 'aligned')
                    for name in ('RLH_SPMM_JT', 'RLH_SPMM_TT', 'RLH_SPMM_TPB'):
                        delenv(name, raising=False)
                if n == 300:
                    run(h, 9, sell_family(key, 9, False), n_own=n_own, leg='unaligned')
                    run(h, 9, sell_family(key, 9, True), cheb=True, n_own=n_own, leg='tight')
                    if halo:                           # the sliced layout: part 1 is empty, part 2 is everything
                        _, rep = run(h, 5, sell_family(key, 5, False), n_own=n_own, parts=(1, 2))
                        assert rep[0] in ('none', 'fake')
                        _, rep = run(h, 5, sell_family(key, 5, True), cheb=True, n_own=n_own, parts=(1, 2))
                        assert rep[0] in ('none', 'fake')


# ---- 1024-row windowed
WELL_N = [1, 100, 1023, 1024, 1025, 2051]
WELL_LENS = [3, 5, 1, 8, 2, 4, 7, 3]


def well_family(key, cheb, epl=None):
    return 'well epl=%d cheb=%d' % ((16 // np.dtype(DT[key]).itemsize) if epl is None else epl, 1 if cheb else 0)


def well(key, setenv, delenv, ns=WELL_N):
    """Bands of up to 8 entries.  A block's staging groups come in eights (512 columns): at n = 1, 100, 1023 and 1025 they
    reach past the last column and the element-wise staging is taken (EPL = 1); at 1024 and 2051 they lie inside (the far
    windows are moved left) and the 16-byte staging runs.  Steps: RLH_SPMM_CPS = 1 with m = 1 .. 6 and = 2 with m = 9, 12
    walk one to six steps (nine: a short last one) through the one-register-set pipeline (EPL = 1, and the float64 fused
    step) at n = 100 and through the two-set one at n = 2051, whose last block is ragged (element-wise epilogue of the
    fused step; whole blocks: the lane-pair epilogue, m odd and even)."""
    assert key in 'sd'
    clear(delenv)
    setenv('RLH_SPMM_FORMAT', 'well')
    setenv('RLH_SPMM_STACK', '0')
    for n in ns:
        lens = WELL_LENS if n > 1 else [1]
        if n == 2051:
            lens = [0 if 1024 <= i < 1030 else WELL_LENS[i % 8] for i in range(n)]       # a few empty rows
        for kind, h in handles(key, lambda kind: ragged(key, n, lens, kind)):
            assert h.layout() == 1
            epl = None if n in (1024, 2051) else 1        # (else a block's whole groups reach past the last column)
            for cheb in (False, True):
                for m in (0, 1, 2, 3, 8, 9, 17):
                    if fits(h, m):
                        win, _ = run(h, m, well_family(key, cheb, epl), cheb=cheb)
                        if not cheb and m:
                            empty_rows_zero(h, win)
                if n in (2051, 100) and kind != 'graded':
                    for cps, ms in ((1, (1, 2, 3, 4, 5, 6)), (2, (9, 12))):
                        setenv('RLH_SPMM_CPS', str(cps))
                        for m in ms:
                            run(h, m, well_family(key, cheb, epl), cheb=cheb, leg='unaligned' if m % 2 else 'aligned')
                    delenv('RLH_SPMM_CPS', raising=False)
                if n == 2051 and kind != 'graded':
                    setenv('RLH_SPMM_VEC', '0')
                    for m in (4, 5):
                        run(h, m, well_family(key, cheb, 1), cheb=cheb)
                    delenv('RLH_SPMM_VEC', raising=False)
                    run(h, 5, well_family(key, cheb, epl), cheb=cheb, leg='tight')


def well_windows(key, setenv, delenv):
    """Blocks that stage 24, 40, 72 and 120 groups (own window + 1, 3, 6 far windows of a 9216-column matrix): 5, 3, 1 and 1
    vectors per step.  One more window (136 groups > 128) and the builder declines: float32 runs in the interleaved
    layout, float64 in the sliced one (the image of its 256-row blocks no longer fits the LDS either)."""
    clear(delenv)
    setenv('RLH_SPMM_FORMAT', 'well')
    setenv('RLH_SPMM_STACK', '0')
    n = 9216
    for kind, h in handles(key, lambda kind: far_windows(key, n, [0, 1, 3, 6, 2, 6, 0, 3, 1], kind), kinds=('gauss', 'exact')):
        assert h.layout() == 1
        for cheb in (False, True):
            for m in (1, 2, 4, 7, 16):
                if fits(h, m):
                    run(h, m, well_family(key, cheb), cheb=cheb)
    for kind, h in handles(key, lambda kind: far_windows(key, n, [7], kind), kinds=('exact',)):
        if native():
            # (float64: the image of the 256-row blocks does not fit the LDS either, the sliced layout runs)
            assert h.layout() == (2 if key == 's' else 0)
            run(h, 3, 'wide k=1 vec cheb=0' if key == 's' else sell_family(key, 3, False))


def well_halo(key, setenv, delenv):
    """A halo block and the two parts: n_own a multiple of EPL (the 16-byte staging stays) and not (EPL = 1)."""
    clear(delenv)
    setenv('RLH_SPMM_FORMAT', 'well')
    setenv('RLH_SPMM_STACK', '0')
    full = 16 // np.dtype(DT[key]).itemsize
    for n, epl in ((2048, full), (2051, 1)):
        for kind, h in handles(key, lambda kind: far_windows(key, n, [0, 0, 0], kind, halo=64), kinds=('gauss', 'exact')):
            assert h.layout() == 1
            for cheb in (False, True):
                for m in (1, 4, 5):
                    run(h, m, well_family(key, cheb, epl), cheb=cheb, n_own=n)
                    run(h, m, well_family(key, cheb, epl), cheb=cheb, n_own=n, parts=(1, 2))
    # no halo column at all: part 2 has nothing to launch
    for kind, h in handles(key, lambda kind: ragged(key, 1025, WELL_LENS, kind), kinds=('exact',)):
        for cheb in (False, True):
            _, rep = run(h, 3, well_family(key, cheb, 1), cheb=cheb, parts=(1, 2))
            assert rep[1] in ('none', 'fake')


# ---- interleaved 256-row
WIDE_N = [1, 255, 256, 257, 600]
WIDE_LENS = [0, 1, 8, 9, 16, 17, 24, 25, 32, 33, 40, 65]      # entry chunks 1 .. 9


def wide_lens(n):
    """Row lengths on the chunk boundaries, block by block a different longest row; rows 256 .. 511 empty in n = 600."""
    out = []
    for i in range(n):
        if n == 600 and 256 <= i < 512:
            out.append(0)
        else:
            out.append(WIDE_LENS[(i + i // 7) % len(WIDE_LENS)])
    return out


def wide_nvs(key):
    return (8, 16, 32) if key in 'sd' else (4, 8, 16)


def wide(key, setenv, delenv, ns=WIDE_N):
    clear(delenv)
    setenv('RLH_SPMM_FORMAT', 'wide')
    for n in ns:
        lens = wide_lens(n) if n > 1 else [1]
        for kind, h in handles(key, lambda kind: ragged(key, n, lens, kind)):
            assert h.layout() in (2, 1)
            for cheb in (False, True):
                c = 'cheb=%d' % cheb
                # 16-byte staging where every 16-column group lies inside the column range: n = 256 (16 whole groups) and
                # 600 (far windows moved left); at 1, 255 and 257 a group reaches past the last column: element-wise
                stage = 'vec' if n in (256, 600) else 'elem'
                nv0 = wide_nvs(key)[0]
                for m in (0, 1, 2):
                    win, _ = run(h, m, 'wide nv=%d vs=1 k=1 %s %s' % (nv0, stage, c), cheb=cheb)
                    if not cheb and m:
                        empty_rows_zero(h, win)
                if n not in (257, 600):
                    continue
                for nv in wide_nvs(key):
                    setenv('RLH_WIDE_NV', str(nv))
                    for vs in (1, 2):
                        if nv == wide_nvs(key)[0] and vs == 2:
                            continue                     # (the smallest pass has one set of threads only)
                        setenv('RLH_WIDE_VS', str(vs))
                        for m in (nv - 1, nv, nv + 1):
                            if fits(h, m):
                                run(h, m, 'wide nv=%d vs=%d k=1 %s %s' % (nv, vs, stage, c), cheb=cheb,
                                    leg='unaligned' if m == nv else 'aligned')
                    delenv('RLH_WIDE_VS', raising=False)
                delenv('RLH_WIDE_NV', raising=False)
                setenv('RLH_SPMM_VEC', '0')
                run(h, 5, 'wide k=1 elem ' + c, cheb=cheb)
                delenv('RLH_SPMM_VEC', raising=False)
                run(h, 5, 'wide nv=8 vs=1 k=1 %s %s' % (stage, c), cheb=cheb, leg='tight')


def wide_windows(key, setenv, delenv):
    """Blocks of 256 rows that stage their own window and 4 or 3 far ones of about 258 columns, 300 columns apart (no hole
    is bridged): 85 and 68 groups of 16 columns, 1360 and 1088 staged columns -- more 16-byte units per vector than the
    workgroup has threads (a second trip of the staging loop) for every type, in odd and even counts."""
    clear(delenv)
    setenv('RLH_SPMM_FORMAT', 'wide')
    for kind, h in handles(key, lambda kind: far_windows(key, 2100, [4, 3], kind, rows_per_block=256, stride=300),
                           kinds=('gauss', 'exact')):
        if native():
            assert h.layout() == 2
        for cheb in (False, True):
            for m in (1, 3, wide_nvs(key)[0] + 1):
                run(h, m, 'wide k=1 vec cheb=%d' % cheb, cheb=cheb)
        setenv('RLH_SPMM_VEC', '0')
        run(h, 3, 'wide k=1 elem cheb=0')
        delenv('RLH_SPMM_VEC', raising=False)


def wide_halo(key, setenv, delenv):
    clear(delenv)
    setenv('RLH_SPMM_FORMAT', 'wide')
    full = 16 // np.dtype(DT[key]).itemsize
    for n in (512, 515):
        # n_own = 515 is no multiple of a 16-byte piece (complex128: one element is one): element-wise staging
        # (complex128 too: the windows moved left to end on column 539 do not start on multiples of 8)
        stage = ' elem' if n == 515 else ' vec'
        for kind, h in handles(key, lambda kind: ragged(key, n, [3, 9, 1, 17, 2], kind, halo=24), kinds=('gauss', 'exact')):
            for cheb in (False, True):
                fam = 'wide k=1%s cheb=%d' % (stage, cheb)
                for m in (1, 5):
                    run(h, m, fam, cheb=cheb, n_own=n)
                    run(h, m, fam, cheb=cheb, n_own=n, parts=(1, 2))


def wide_pairs(key, setenv, delenv):
    """Row pairs (wide_k = 2), n even and odd, and the same matrix with RLH_WIDE_PAIR=0."""
    assert key in 'sd'
    clear(delenv)
    setenv('RLH_SPMM_FORMAT', 'wide')
    for odd in (False, True):
        for pair in (1, 0):
            setenv('RLH_WIDE_PAIR', str(pair))
            for kind, h in handles(key, lambda kind: paired(key, 300, odd, kind), kinds=('gauss', 'exact')):
                for cheb in (False, True):
                    for m in (1, 7, 8, 9, 17):
                        if fits(h, m):
                            run(h, m, 'wide k=%d vec cheb=%d' % (2 if pair else 1, cheb), cheb=cheb)


# ---- stacks
def stack_family(key, cheb=False, dma=None, how='pat dtab'):
    if dma is None:
        dma = key != 's'
    if not dma:
        return 'stack reg'
    if key == 'z':
        how = 'vals idx'
    return 'stack dma %s cheb=%d' % (how, 1 if cheb else 0)


STACK_M = (0, 1, 2, 3, 4, 5, 8, 9)


def without_rows(a, rows):
    """The matrix with these rows emptied."""
    a = a.tolil()
    for r in rows:
        a.rows[r], a.data[r] = [], []
    a = sp.csr_matrix(a)
    a.sort_indices()
    return a


def stacks(key, setenv, delenv, grids=((16, 16, 12), (16, 16, 20), (16, 16, 17))):
    """lap3d-patterned operators of 3, 5 and 4.25 row blocks (planes of 256 rows: blocks pair one plane of blocks apart; an
    odd count leaves a stack of one; 16 x 16 x 17 has a ragged last block).  The first grid's exact matrix has a few empty
    rows in two of its blocks (+0, bit for bit)."""
    clear(delenv)
    setenv('RLH_SPMM_FORMAT', 'well')
    setenv('RLH_SPMM_STACK', '2')
    for grid in grids:
        def build(kind):
            a = stencil(key, *grid, kind)
            # (complex128 keeps every row: its stacked fused step needs the diagonal stored in every row)
            return without_rows(a, [5, 6, 1500, 2047]) if kind == 'exact' and grid == grids[0] and key != 'z' else a
        for kind, h in handles(key, build):
            if last_launch() != 'fake':
                assert h.stacks() > 0, 'the stacks were not built'
            legs = [({}, stack_family(key))]
            if key == 's':
                legs.append(({'RLH_SPMM_STACK_DMA': '2'}, stack_family(key, dma=True)))
            if key == 'd':
                legs.append(({'RLH_SPMM_STACK_DMA': '0'}, stack_family(key, dma=False)))
            for env, fam in legs:
                for name, value in env.items():
                    setenv(name, value)
                for m in STACK_M:
                    if fits(h, m):
                        win, _ = run(h, m, fam, leg='unaligned' if m == 3 else 'aligned')
                        if m:
                            empty_rows_zero(h, win)
                if key in 'sd':
                    setenv('RLH_SPMM_STACK_PAT', '0')
                    if 'dma' in fam:
                        run(h, 5, stack_family(key, dma=True, how='vals idx'))
                    delenv('RLH_SPMM_STACK_PAT', raising=False)
                for name in env:
                    delenv(name, raising=False)
            if key == 'z':
                setenv('RLH_SPMM_STACK_CHEB', '2')
                for m in (1, 2, 3, 5):
                    run(h, m, stack_family(key, cheb=True), cheb=True)
                delenv('RLH_SPMM_STACK_CHEB', raising=False)
            if key in 'sd' and grid == grids[0]:
                # RLH_SPMM_STACK=0 at call time: the unstacked kernel on the same handle, and the same bits
                a, _ = run(h, 5, stack_family(key))
                setenv('RLH_SPMM_STACK', '0')
                b, _ = run(h, 5, well_family(key, False))
                setenv('RLH_SPMM_STACK', '2')
                assert same_bytes(a, b), 'stacked and unstacked kernels differ'


def stacks_dictionaries(key, setenv, delenv):
    """The dictionary with explicit positions (RLH_SPMM_STACK_DPAT=0 at creation) and explicit entries (_PAT=0)."""
    assert key in 'sdc'
    clear(delenv)
    setenv('RLH_SPMM_FORMAT', 'well')
    setenv('RLH_SPMM_STACK', '2')
    if key == 's':
        setenv('RLH_SPMM_STACK_DMA', '2')
    for name, how in (('RLH_SPMM_STACK_DPAT', 'pat idx'), ('RLH_SPMM_STACK_PAT', 'vals idx')):
        setenv(name, '0')
        for kind, h in handles(key, lambda kind: stencil(key, 16, 16, 12, kind), kinds=('graded', 'exact')):
            for m in (1, 4, 5):
                run(h, m, stack_family(key, dma=True, how=how))
        delenv(name, raising=False)


def with_halo(key, a, rows, halo, kind):
    """`a` (n x n) with `halo` more columns: row rows[k] gets one entry in halo column k mod halo."""
    n = a.shape[0]
    v = draw(key, 'exact' if kind == 'exact' else 'gauss', len(rows), 9)
    v[v == 0] = 1
    far = sp.csr_matrix((v, (np.asarray(rows), np.arange(len(rows)) % halo)), shape=(n, halo), dtype=DT[key])
    out = sp.csr_matrix(sp.hstack([sp.csr_matrix(a), far], format='csr'), dtype=DT[key])
    out.sort_indices()
    return out


def stacks_halo(key, setenv, delenv):
    """A halo block and the parts: the LDS-DMA kernel only; with RLH_SPMM_STACK_DMA=0 the unstacked kernel runs."""
    clear(delenv)
    setenv('RLH_SPMM_FORMAT', 'well')
    setenv('RLH_SPMM_STACK', '2')
    n = 16 * 16 * 12
    # rows of the first plane (at most 6 entries) reference the halo
    for kind, h in handles(key, lambda kind: with_halo(key, stencil(key, 16, 16, 12, kind), np.arange(0, 256, 5), 64, kind),
                           kinds=('gauss', 'exact')):
        # (the rows with a halo entry have position tuples of their own: no position dictionary, explicit positions)
        fam = stack_family(key, dma=True, how='pat idx')
        for m in (1, 4, 5):
            run(h, m, fam, n_own=n)
            run(h, m, fam, n_own=n, parts=(1, 2))
        if key in 'sd':
            setenv('RLH_SPMM_STACK_DMA', '0')
            run(h, 4, well_family(key, False), n_own=n)
            delenv('RLH_SPMM_STACK_DMA', raising=False)
        if key == 'z':                                     # the stacked fused step (every row stores its diagonal, <= 7 entries)
            setenv('RLH_SPMM_STACK_CHEB', '2')
            for m in (1, 3):
                run(h, m, stack_family(key, cheb=True), cheb=True, n_own=n)
                run(h, m, stack_family(key, cheb=True), cheb=True, n_own=n, parts=(1, 2))
            delenv('RLH_SPMM_STACK_CHEB', raising=False)
        if key == 's':                                     # the bfloat16 step on the stacks: n_own and ldh multiples of 8
            for m in (1, 9):
                run(h, m, 'stack bf16 vps=2 pat idx', cheb=True, bf16=True, n_own=n)
                run(h, m, 'stack bf16 vps=2 pat idx', cheb=True, bf16=True, n_own=n, parts=(1, 2))


LEGS_SEEN = []       # (case, type, leg, report): what the overhang / tight / recut legs launched, printed by their tests


def stacks_overhang(key, setenv, delenv):
    """A grid whose column count is no multiple of 8 (15 x 15 x 15 = 3375): `overhang` (ld >= n_cols + 7) takes the stacks,
    which stage up to 7 NaN rows past the vectors; `tight` (ld == n_cols) must not take them.  (The plane of 225 rows is
    smaller than a block: RLH_SPMM_STACK_ALIGN changes nothing here -- stacks_recut has the grid for it.)"""
    clear(delenv)
    setenv('RLH_SPMM_FORMAT', 'well')
    setenv('RLH_SPMM_STACK', '2')
    for kind, h in handles(key, lambda kind: stencil(key, 15, 15, 15, kind), kinds=('gauss', 'exact')):
        if native():
            assert h.stacks() > 0, 'the stacks were not built'
        _, over = run(h, 5, 'stack reg' if key == 's' else stack_family(key, dma=True), leg='overhang')
        # (3375 columns hold every block's whole groups: both unstacked layouts stage by 16-byte pieces)
        _, tight = run(h, 5, well_family(key, False) if key in 'sd' else 'wide nv=8 k=1 vec cheb=0', leg='tight')
        if native():
            assert over[0].split()[0] == 'stack' and tight[0].split()[0] != 'stack'
        LEGS_SEEN.append(('overhang 15^3 ' + kind, key, 'overhang', over[0]))
        LEGS_SEEN.append(('overhang 15^3 ' + kind, key, 'tight', tight[0]))


def stacks_recut(key, setenv, delenv):
    """A grid whose plane is more than a block and no whole number of blocks (40 x 40 x 5: planes of 1600 rows).  With
    RLH_SPMM_STACK_ALIGN=0 the rows are cut into uniform blocks of 1024; with =2 plane by plane, two blocks of 800 rows per
    plane, block j of a plane stacked on block j of the next, the fifth plane's blocks as stacks of one: members of unequal
    row counts whose ranges are no multiples of 1024, and the owner / part split over them.  The two handles must differ
    (rlh_csr_stacks); both run the product, whole, with a halo block and in parts; complex128 the stacked fused step."""
    assert key in 'dcz'
    clear(delenv)
    setenv('RLH_SPMM_FORMAT', 'well')
    setenv('RLH_SPMM_STACK', '2')
    grid, n = (40, 40, 5), 8000
    info = {}
    for align in ('0', '2'):
        setenv('RLH_SPMM_STACK_ALIGN', align)
        for halo in (0, 64):
            def build(kind):
                a = stencil(key, *grid, kind)
                return with_halo(key, a, np.arange(0, 1600, 7), halo, kind) if halo else a
            for kind, h in handles(key, build, kinds=('gauss', 'exact')):
                if native():
                    info[(align, halo)] = h.stacks_info()
                    assert info[(align, halo)][0] > 0, 'the stacks were not built'
                fam = stack_family(key, dma=True, how='pat idx' if halo else 'pat dtab')     # (as in stacks_halo)
                if not halo:
                    for m in (1, 2, 3, 5):
                        _, rep = run(h, m, fam, leg='unaligned' if m == 3 else 'aligned')
                    if key == 'z':
                        setenv('RLH_SPMM_STACK_CHEB', '2')
                        for m in (1, 3):
                            run(h, m, stack_family(key, cheb=True), cheb=True)
                        delenv('RLH_SPMM_STACK_CHEB', raising=False)
                else:
                    for m in (1, 4):
                        run(h, m, fam, n_own=n)
                        _, rep = run(h, m, fam, n_own=n, parts=(1, 2))
                LEGS_SEEN.append(('recut 40x40x5 align=%s halo=%d %s' % (align, halo, kind), key, 'stacks %r' % (info.get((align, halo)),),
                                  ' | '.join(rep)))
    if native():
        for halo in (0, 64):
            assert info[('0', halo)] != info[('2', halo)], 'RLH_SPMM_STACK_ALIGN=2 did not recut the blocks: %r' % (info,)


def legs_text():
    return '\n'.join('%-40s %s %-9s %s' % row for row in LEGS_SEEN)


# ---- the bfloat16 step
BF16_M = (1, 7, 8, 9, 15, 16, 17)


def bf16_step(setenv, delenv):
    key = 's'
    clear(delenv)
    # the unstacked windowed kernel
    setenv('RLH_SPMM_FORMAT', 'well')
    setenv('RLH_SPMM_STACK', '0')
    for kind, h in handles(key, lambda kind: ragged(key, 2051, WELL_LENS, kind), kinds=('gauss', 'exact')):
        assert h.bf16_ready(2051, 0) == 1
        for m in BF16_M:
            run(h, m, 'well bf16', cheb=True, bf16=True)
        run(h, 3, 'well bf16', cheb=True, bf16=True, leg='unaligned', expect_error=True)
    # the stacks, two and one vectors per step, and the unstacked kernel on the same handle
    setenv('RLH_SPMM_STACK', '2')
    for kind, h in handles(key, lambda kind: stencil(key, 16, 16, 12, kind), kinds=('gauss', 'exact')):
        for vps in (2, 1):
            setenv('RLH_SPMM_BF16_VPS', str(vps))
            for m in BF16_M:
                run(h, m, 'stack bf16 vps=%d pat dtab' % vps, cheb=True, bf16=True)
        delenv('RLH_SPMM_BF16_VPS', raising=False)
        setenv('RLH_SPMM_STACK_BF16', '0')
        run(h, 9, 'well bf16', cheb=True, bf16=True)
        delenv('RLH_SPMM_STACK_BF16', raising=False)
        run(h, 3, 'stack bf16', cheb=True, bf16=True, leg='unaligned', expect_error=True)
    # the interleaved layout, single rows and row pairs
    setenv('RLH_SPMM_FORMAT', 'wide')
    delenv('RLH_SPMM_STACK', raising=False)
    for build, k in ((lambda kind: ragged(key, 600, wide_lens(600), kind), 1), (lambda kind: paired(key, 300, False, kind), 2)):
        for kind, h in handles(key, build, kinds=('gauss', 'exact')):
            assert h.bf16_ready(h.n_cols, 0) == 1
            for m in BF16_M:
                run(h, m, 'wide bf16 k=%d vec' % k, cheb=True, bf16=True)
            run(h, 3, 'wide bf16', cheb=True, bf16=True, leg='unaligned', expect_error=True)
    # halo and parts: n_own and ldh multiples of 8
    for fmt, fam in (('well', 'well bf16'), ('wide', 'wide bf16 k=1 vec')):
        setenv('RLH_SPMM_FORMAT', fmt)
        setenv('RLH_SPMM_STACK', '0')
        for kind, h in handles(key, lambda kind: far_windows(key, 2048, [0, 0], kind, halo=64), kinds=('gauss', 'exact')):
            ldh = leading_dimension('aligned', 64, np.uint16, 1)
            assert h.bf16_ready(2048, ldh) == 1
            for m in (1, 8, 9):
                run(h, m, fam, cheb=True, bf16=True, n_own=2048)
                run(h, m, fam, cheb=True, bf16=True, n_own=2048, parts=(1, 2))
    # the sliced layout is not taken, and rlh_csr_bf16_ready says so
    setenv('RLH_SPMM_FORMAT', 'sell')
    for kind, h in handles(key, lambda kind: ragged(key, 300, SELL_LENS, kind), kinds=('exact',)):
        if last_launch() != 'fake':
            assert h.bf16_ready(300, 0) == 0
            run(h, 3, 'sell', cheb=True, bf16=True, expect_error=True)


# ---- the grid-stride second trip (exact only: one more unit than the launch has workgroups)
def second_trip(key, family, cu, setenv, delenv):
    clear(delenv)
    if family == 'sell':
        setenv('RLH_SPMM_FORMAT', 'sell')
        setenv('RLH_SPMM_WG_PER_CU', '1')
        setenv('RLH_SPMM_CHUNK', '1')
        n = 64 * 4 * ((cu + 7) // 8 * 8 + 1)               # four slices per workgroup, the grid a multiple of 8
        build = lambda kind: ragged(key, n, [2, 1, 3], kind)
        fams = [sell_family(key, 2, False), sell_family(key, 2, True)]
    elif family == 'wide':
        setenv('RLH_SPMM_FORMAT', 'wide')
        setenv('RLH_WIDE_WG_PER_CU', '1')
        build = lambda kind: ragged(key, 256 * (cu + 1), [2, 1, 3], kind)
        fams = ['wide k=1 vec cheb=0', 'wide k=1 vec cheb=1']
    elif family == 'well':
        setenv('RLH_SPMM_FORMAT', 'well')
        setenv('RLH_SPMM_STACK', '0')
        build = lambda kind: ragged(key, 1024 * (cu + 1), [2, 1, 3], kind)
        fams = [well_family(key, False), well_family(key, True)]
    else:
        setenv('RLH_SPMM_FORMAT', 'well')
        setenv('RLH_SPMM_STACK', '2')
        build = lambda kind: stencil(key, 32, 32, 2 * (cu + 1), kind)
        fams = [stack_family(key)]
    for kind, h in handles(key, build, kinds=('exact',)):
        for fam in fams:
            _, rep = run(h, 2, fam, cheb='cheb=1' in fam)
            if rep[0] != 'fake':
                words = dict(w.split('=') for w in rep[0].split() if '=' in w)
                units = int(words['len']) if family != 'sell' else (int(words['len']) + 3) // 4
                assert units > int(words['grid']), 'no second trip: %s' % rep[0]


# ---- rlh_gather_rows / _bf16
GATHER_N = [0, 1, 255, 256, 257]


def gather(key, bf16=False):
    lib = _L()
    L = lib.lib()
    from raleigh_amd.algebra.hip.memory import DeviceBuffer
    dt = np.uint16 if bf16 else DT[key]
    n = 300
    for nidx in GATHER_N:
        for m in (0, 1, 3):
            for leg in ('aligned', 'unaligned'):
                if bf16 and leg == 'unaligned':
                    continue
                rng = np.random.default_rng(nidx + m)
                idx = np.ascontiguousarray(rng.integers(0, n, nidx), dtype=np.int64)       # unsorted, repeats
                if nidx > 2:
                    idx[1] = idx[0]
                xs = draw(key, 'gauss', (m, n), 7, bf16)
                X = Blk(dt, n, m, leg, 0, _bits(xs) if bf16 else xs, 'nan')
                O = Blk(dt, nidx, m, leg, 1, None, 'ramp')
                d_idx = DeviceBuffer(max(idx.nbytes, 16), zero=False)
                if nidx:
                    lib.check(L.rlh_h2d(d_idx.ptr, lib.host_ptr(idx), idx.nbytes))
                if bf16:
                    lib.check(L.rlh_gather_rows_bf16(nidx, d_idx.ptr, m, X.ptr(), X.ld, O.ptr(), O.ld))
                else:
                    lib.check(L.rlh_gather_rows(lib.dtype_code(dt), nidx, d_idx.ptr, m, X.ptr(), X.ld, O.ptr(), O.ld))
                win = O.result('[gather %s nidx=%d m=%d %s]' % (key, nidx, m, leg))
                assert same_bytes(win, np.ascontiguousarray(X.window()[:, idx])), 'gathered rows differ'
                X.unchanged('[gather]')


# ---- constructors: the upper triangle and the device arrays give the bits of the host-built handle
def constructors(key, setenv, delenv, fmt):
    clear(delenv)
    setenv('RLH_SPMM_FORMAT', fmt)

    def herm(kind):
        a = stencil(key, 9, 8, 7, kind)
        return a
    a = herm('exact')
    with Handle(key, a, 'exact') as h0:
        want, _ = run(h0, 5, sell_family(key, 5, False) if fmt == 'sell' else 'wide nv=8 vs=1 k=1 vec cheb=0', seed=5)
    hows = [('upper', 32)]
    if last_launch() != 'fake':
        hows += [('device', 32), ('device', 64), ('device_upper', 32), ('device_upper', 64)]
    for how, bits in hows:
        with Handle(key, a, 'exact', how=how, bits=bits) as h:
            got, _ = run(h, 5, sell_family(key, 5, False) if fmt == 'sell' else 'wide nv=8 vs=1 k=1 vec cheb=0', seed=5)
            assert same_bytes(got, want), 'the handle of %s (%d-bit indices) gives other bits' % (how, bits)


# ---- foreign columns and empty rows, per layout
def foreign_columns(key, fmt, setenv, delenv):
    clear(delenv)
    setenv('RLH_SPMM_FORMAT', fmt)
    setenv('RLH_SPMM_STACK', '0')
    n = 1100
    lens = [1, 3, 5, 2, 4]
    for kind, h in handles(key, lambda kind: ragged(key, n, lens, kind, halo=16), kinds=('gauss',)):
        for cheb in (False, True):
            # (the windows moved left to end on column 1115 do not start on multiples of 8: with a halo block the staging
            # of both windowed layouts is element-wise)
            f = {'sell': sell_family(key, 3, cheb), 'well': well_family(key, cheb, 1), 'wide': 'wide k=1 elem cheb=%d' % cheb}[fmt]
            foreign(h, 3, f, 517, cheb=cheb, n_own=n)
            if not cheb:
                foreign(h, 3, f, n + 3, cheb=cheb, n_own=n)        # a row of the halo block


def foreign_columns_stacks(key, setenv, delenv):
    clear(delenv)
    setenv('RLH_SPMM_FORMAT', 'well')
    setenv('RLH_SPMM_STACK', '2')
    for kind, h in handles(key, lambda kind: stencil(key, 16, 16, 12, kind), kinds=('gauss',)):
        foreign(h, 3, 'stack reg' if key == 's' else stack_family(key, dma=True), 1500)
        if key == 'z':
            setenv('RLH_SPMM_STACK_CHEB', '2')
            foreign(h, 3, stack_family(key, cheb=True), 1500, cheb=True)
            delenv('RLH_SPMM_STACK_CHEB', raising=False)


def foreign_columns_bf16(setenv, delenv):
    """The +Inf column (bfloat16 0x7F80) through the three kernels of the bfloat16 step."""
    key = 's'
    clear(delenv)
    setenv('RLH_SPMM_FORMAT', 'well')
    setenv('RLH_SPMM_STACK', '0')
    for kind, h in handles(key, lambda kind: ragged(key, 2051, [1, 3, 5, 2, 4], kind), kinds=('gauss',)):
        foreign(h, 3, 'well bf16', 1517, cheb=True, bf16=True)
    setenv('RLH_SPMM_STACK', '2')
    for kind, h in handles(key, lambda kind: stencil(key, 16, 16, 12, kind), kinds=('gauss',)):
        foreign(h, 3, 'stack bf16 vps=2 pat dtab', 1500, cheb=True, bf16=True)
    setenv('RLH_SPMM_FORMAT', 'wide')
    delenv('RLH_SPMM_STACK', raising=False)
    for kind, h in handles(key, lambda kind: ragged(key, 600, [1, 3, 9, 2, 17], kind), kinds=('gauss',)):
        foreign(h, 3, 'wide bf16 k=1 vec', 317, cheb=True, bf16=True)


def empty_rows_pinned(key, fmt, setenv, delenv):
    """One clearly named pin per layout of what an empty row is when position 0 is not finite."""
    clear(delenv)
    setenv('RLH_SPMM_FORMAT', fmt)
    setenv('RLH_SPMM_STACK', '0')
    n = 300
    lens = [2, 0, 3, 1]
    for kind, h in handles(key, lambda kind: ragged(key, n, lens, kind), kinds=('gauss',)):
        fam = {'sell': sell_family(key, 3, False), 'well': well_family(key, False, 1), 'wide': 'wide k=1 vec cheb=0'}[fmt]
        empty_rows_nonfinite(h, 3, fam)
