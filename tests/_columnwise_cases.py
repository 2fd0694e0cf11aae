"""Column-wise kernels, element by element, shared by the CPU tier (tests/fake_lib.py: shows that NumPy in the
working precision meets every bound below) and the GPU tier (librlhip.so): axpy, column axpy, linear combination,
scaling, copy / gather of columns, conjugation, precision conversion, bfloat16 packing, dots, transposed dots,
largest modulus and row gather, through the raw C ABI.

Harness.  Every operand is a host array of m + 2 columns of ld elements filled with values that differ from
position to position.  It is uploaded whole, the entry point runs on the window of m columns that starts at
column 1, rows [0, n), and the whole array is downloaded again: the window is held to the operation's bound
against the same operation done in float64 / complex128 on the uploaded values, and every other byte -- the two
guard columns, rows n .. ld - 1 of every column, the read-only operands -- must be what was uploaded.

Shapes.  One workgroup is 256 lanes x 16 bytes: 1024 / 512 / 512 / 256 elements of s / d / c / z, so the row
counts below are one short of, one past and several times a workgroup for every type, 4099 leaves a ragged last
workgroup far from the first, and 66001 x 17 is swept several times by the capped grid of RLH_ROW_BLOCKS_PER_CU=1.
Leading dimensions: n rounded up to 32 elements (16-byte aligned columns: the vector paths), or about n + 3 with
the base shifted by one element (8 bytes for complex128), so that no column is 16-byte aligned (the scalar paths);
every operand of a call has its own.

Bounds.  u is the unit roundoff of the type's real part, |.| the modulus.  They count roundings and are not
measurements:
  * copy, copy_cols, conj, convert, bf16 pack / unpack, gather_rows: bit-exact;
  * scale (multiply): real bit-exact against x * T(s) (one rounding either way); complex 4 u |s| |x| (rounding s
    to the type: u; a complex product: sqrt(5) u without fused operations, less with them);
  * scale (divide): 3 u |x / s| real, 6 u |x / s| complex (the library multiplies by a reciprocal formed in double:
    its rounding to the type, then the product);
  * axpy, axpy_cols, lincomb: 2 u (|a| |x| + |y|) real -- the product and the sum, or one fused operation and the
    rounding of the coefficient to the type -- and 8 u (|a| |x| + |y|) complex;
  * dots: (n + 2) u sum |x| |y| per entry (n additions, the product, the final rounding); transposed dots the same
    with the number of vectors m in place of n;
  * absmax: exact.
"""

import ctypes

import numpy as np

from oracle import ops

DT = {'s': np.float32, 'd': np.float64, 'c': np.complex64, 'z': np.complex128}
WIDE = {'s': np.float64, 'd': np.float64, 'c': np.complex128, 'z': np.complex128}
KEYS = ['s', 'd', 'c', 'z']

ROWS = [1, 3, 255, 257, 511, 513, 1023, 1025, 4099, 66001]
COLS = [1, 3, 17]
SHAPES = [(n, m) for n in ROWS for m in COLS]
# copies move 16-byte words and a tail of 0 - 3 dwords: n * es % 16 = 0, 4, 8 and 12 for every element size
COPY_SHAPES = SHAPES + [(n, m) for n in (1024, 1026) for m in (1, 3)]
SWEEP_SHAPE = (66001, 17)                  # the capped grid of RLH_ROW_BLOCKS_PER_CU=1 loops over it
MANY_ROWS = [8, 24, 33]
MANY_COLS = [32768, 32769, 65535, 65536, 70001]
MANY_SHAPES = [(n, m) for n in MANY_ROWS for m in MANY_COLS]
MANY_KEYS = ['s', 'z']


def unit_roundoff(key):
    return float(np.finfo(np.float32 if key in 'sc' else np.float64).eps) / 2


# ---------------------------------------------------------------------------------------------------- harness
_POOL = {}


def _pool(dtype, count):
    """`count` values that differ from position to position: one seeded draw per type, shared by every operand."""
    dtype = np.dtype(dtype)
    have = _POOL.get(dtype)
    if have is None or have.size < count:
        size = max(count, 1 << 22)
        rng = np.random.default_rng(20240 + dtype.num)
        if dtype.kind == 'u':
            have = rng.integers(0, 1 << (8 * dtype.itemsize), size, dtype=np.uint64).astype(dtype)
        elif dtype.kind == 'c':
            have = (rng.standard_normal(size) + 1j * rng.standard_normal(size)).astype(dtype)
        else:
            have = rng.standard_normal(size).astype(dtype)
        have.setflags(write=False)
        _POOL[dtype] = have
    return have


def leading_dimension(n, dtype, aligned, which=0):
    """ld of operand number `which`: 16-byte aligned columns, or columns that are not (complex128: always a multiple
    of 16 bytes, the base is shifted instead)."""
    es = np.dtype(dtype).itemsize
    if aligned:
        return (n + 31) // 32 * 32 + 32 * which
    ld = n + 3 + 2 * which
    while es < 16 and ld * es % 16 == 0:
        ld += 1
    return ld


def base_shift(dtype, aligned):
    es = np.dtype(dtype).itemsize
    return 0 if aligned else min(es, 8)


def same_bytes(a, b):
    """Bit-for-bit equality of two C-contiguous arrays of one shape and type (-0.0 != 0.0, NaN == the same NaN)."""
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


class Block:
    """(m + 2) columns of ld elements on the host (one column per ROW of `host`) and on the device."""

    def __init__(self, dtype, n, m, ld, shift=0, which=0):
        from raleigh_amd import _lib
        from raleigh_amd.algebra.hip.memory import DeviceBuffer
        self.dtype = np.dtype(dtype)
        self.n, self.m, self.ld, self.es = n, m, ld, self.dtype.itemsize
        assert ld >= n
        count = (m + 2) * ld
        off = 1013 * which + 7
        self.host = _pool(self.dtype, count + off)[off:off + count].reshape(m + 2, ld).copy()
        self._buf = DeviceBuffer(self.host.nbytes + 16)
        self.base = self._buf.ptr + shift
        self.upload()

    def upload(self):
        from raleigh_amd import _lib
        _lib.check(_lib.lib().rlh_h2d(self.base, _lib.host_ptr(self.host), self.host.nbytes))

    def set_window(self, values):
        self.host[1:self.m + 1, :self.n] = values
        self.upload()

    def ptr(self, column=1):
        """Device address of a column (1: the first of the window)."""
        return self.base + column * self.ld * self.es

    def window(self):
        return self.host[1:self.m + 1, :self.n]

    def wide(self):
        w = self.window()
        return w.astype(np.complex128 if self.dtype.kind == 'c' else np.float64)

    def fetch(self):
        from raleigh_amd import _lib
        out = np.empty_like(self.host)
        _lib.check(_lib.lib().rlh_d2h(_lib.host_ptr(out), self.base, out.nbytes))
        return out

    def check_unchanged(self, what=''):
        assert same_bytes(self.fetch(), self.host), 'read-only operand modified %s' % what

    def check(self, want, bound=None, what=''):
        """The whole downloaded array: the window against `want` (bit for bit, or |got - want| <= bound element by
        element), every other byte as uploaded.  Returns the window."""
        got = self.fetch()
        win = got[1:self.m + 1, :self.n].copy()
        rest = got
        rest[1:self.m + 1, :self.n] = self.window()
        assert same_bytes(rest, self.host), 'guard columns or padding rows modified %s' % what
        if bound is None:
            want = np.ascontiguousarray(np.broadcast_to(want, win.shape), dtype=self.dtype)
            if not same_bytes(win, want):
                bad = np.argwhere(win.view(np.uint8).reshape(win.shape + (-1,)).astype(np.int16)
                                  != want.view(np.uint8).reshape(win.shape + (-1,)))
                raise AssertionError('%d bytes differ, first at (column, row) %s %s' % (len(bad), tuple(bad[0][:2]), what))
        else:
            err = np.abs(win.astype(want.dtype) - want)
            bad = ~(err <= bound)                                # (a NaN fails too)
            if bad.any():
                j, i = np.argwhere(bad)[0]
                raise AssertionError('(column %d, row %d): error %.3e above the bound %.3e %s'
                                     % (j, i, err[j, i], np.broadcast_to(bound, err.shape)[j, i], what))
        return win


def operands(key, n, m, aligned, count, dtypes=None):
    """`count` blocks for one call, every one with its own leading dimension."""
    out = []
    for i in range(count):
        dt = DT[key] if dtypes is None else dtypes[i]
        out.append(Block(dt, n, m, leading_dimension(n, dt, aligned, i), base_shift(dt, aligned), which=i))
    return out


def _lib_and_code(key):
    from raleigh_amd import _lib
    return _lib, _lib.lib(), _lib.dtype_code(DT[key])


def coefficients(key, m, seed, nonzero_imag=True):
    """m coefficients of the working type (complex ones with a non-zero imaginary part)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.25, 2.0, m) * rng.choice([-1.0, 1.0], m)
    if key in 'cz':
        c = c + 1j * rng.uniform(0.25, 2.0, m) * rng.choice([-1.0, 1.0], m)
    return np.ascontiguousarray(c.astype(DT[key]))


def _tag(op, key, n, m, aligned):
    return '[%s %s n=%d m=%d %s]' % (op, key, n, m, 'aligned' if aligned else 'unaligned')


# ---------------------------------------------------------------------------------------------------- operations
def axpy_alpha(key):
    """A coefficient of rlh_axpy that every type holds exactly: the bound's two roundings are then the product and
    the sum (NumPy) or the one fused operation (the kernel)."""
    return complex(0.3125, -1.75) if key in 'cz' else -0.3125


def axpy(key, n, m, aligned):
    """rlh_axpy: Y += alpha X with alpha given in double.  Once with a coefficient that the type holds exactly, under
    the bound of the module's header, and once with one that it does not.  For the real types three roundings may
    then add up: |fl(T(alpha) x + y) - (alpha x + y)| <= u |alpha| |x| (alpha rounded to the type) + u |alpha| |x| (the
    product; absent when fused) + u |alpha x + y| (the sum) <= 2 u (|alpha| |x| + |y|) + u |alpha| |x|.  The complex
    bound has room for the coefficient's rounding: u + sqrt(5) u for the product, u for the sum."""
    _lib, L, code = _lib_and_code(key)
    u = unit_roundoff(key)
    cx = key in 'cz'
    for alpha, extra in ((axpy_alpha(key), 0), (complex(0.3, -1.7) if cx else -0.3, 0 if cx else 1)):
        x, y = operands(key, n, m, aligned, 2)
        a = np.array([np.real(alpha), np.imag(alpha)], dtype=np.float64)
        _lib.check(L.rlh_axpy(code, n, m, _lib.host_ptr(a), x.ptr(), x.ld, y.ptr(), y.ld))
        want = y.wide() + alpha * x.wide()
        ax = abs(alpha) * np.abs(x.wide())
        bound = (8 if cx else 2) * u * (ax + np.abs(y.wide())) + extra * u * ax
        y.check(want, bound, _tag('axpy(%r)' % (alpha,), key, n, m, aligned))
        x.check_unchanged(_tag('axpy', key, n, m, aligned))


def axpy_cols(key, n, m, aligned):
    _lib, L, code = _lib_and_code(key)
    x, y = operands(key, n, m, aligned, 2)
    s = coefficients(key, m, 11)
    _lib.check(L.rlh_axpy_cols(code, n, m, _lib.host_ptr(s), x.ptr(), x.ld, y.ptr(), y.ld))
    u = unit_roundoff(key)
    sw = s.astype(WIDE[key])[:, None]
    want = y.wide() + sw * x.wide()
    bound = (8 if key in 'cz' else 2) * u * (np.abs(sw) * np.abs(x.wide()) + np.abs(y.wide()))
    y.check(want, bound, _tag('axpy_cols', key, n, m, aligned))
    x.check_unchanged(_tag('axpy_cols', key, n, m, aligned))


def lincomb(key, n, m, aligned, alias):
    """rlh_lincomb_cols: Out = a A + b B with Out distinct (alias None), Out == A ('a') or Out == B ('b')."""
    _lib, L, code = _lib_and_code(key)
    a_blk, b_blk, o_blk = operands(key, n, m, aligned, 3)
    out = {None: o_blk, 'a': a_blk, 'b': b_blk}[alias]
    a, b = coefficients(key, m, 12), coefficients(key, m, 13)
    _lib.check(L.rlh_lincomb_cols(code, n, m, _lib.host_ptr(a), a_blk.ptr(), a_blk.ld, _lib.host_ptr(b), b_blk.ptr(),
                                  b_blk.ld, out.ptr(), out.ld))
    u = unit_roundoff(key)
    aw, bw = a.astype(WIDE[key])[:, None], b.astype(WIDE[key])[:, None]
    want = aw * a_blk.wide() + bw * b_blk.wide()
    # (the two terms play |a| |x| and |y| of the axpy bound: a product, then a fused or separate multiply-add)
    bound = (8 if key in 'cz' else 2) * u * (np.abs(aw) * np.abs(a_blk.wide()) + np.abs(bw) * np.abs(b_blk.wide()))
    tag = _tag('lincomb(out=%s)' % (alias or 'other'), key, n, m, aligned)
    out.check(want, bound, tag)
    for blk in (a_blk, b_blk, o_blk):
        if blk is not out:
            blk.check_unchanged(tag)


def scale(key, n, m, aligned, multiply):
    _lib, L, code = _lib_and_code(key)
    x, = operands(key, n, m, aligned, 1)
    s = coefficients(key, m, 14).astype(WIDE[key]) * 1.1         # doubles that the type does not hold exactly
    if not multiply:
        s[m // 2] = 0                                            # divide: this column comes back untouched
    sd = np.ascontiguousarray(s).view(np.float64)
    _lib.check(L.rlh_scale_cols(code, n, m, _lib.host_ptr(sd), 1 if multiply else 0, x.ptr(), x.ld))
    u = unit_roundoff(key)
    tag = _tag('scale(%s)' % ('multiply' if multiply else 'divide'), key, n, m, aligned)
    if multiply:
        if key in 'sd':
            x.check(x.window() * s.astype(DT[key])[:, None], None, tag)
        else:
            want = s[:, None] * x.wide()
            x.check(want, 4 * u * np.abs(want), tag)
    else:
        nz = s != 0
        want = x.wide()
        want[nz] = want[nz] / s[nz, None]
        bound = (6 if key in 'cz' else 3) * u * np.abs(want)
        bound[~nz] = 0.0                                         # (exactly the uploaded values)
        win = x.check(want, bound, tag)
        assert same_bytes(win[~nz], x.window()[~nz]), 'column with a zero divisor modified ' + tag


def copy(key, n, m, aligned):
    _lib, L, code = _lib_and_code(key)
    x, y = operands(key, n, m, aligned, 2)
    _lib.check(L.rlh_copy(code, n, m, x.ptr(), x.ld, y.ptr(), y.ld))
    y.check(x.window(), None, _tag('copy', key, n, m, aligned))
    x.check_unchanged()


def copy_cols(key, n, m, aligned):
    """rlh_copy_cols: repeated, descending indices that also point outside the destination's window (the source's
    guard columns 0 and m + 1 count from the start of its storage); then once inside one allocation."""
    _lib, L, code = _lib_and_code(key)
    x, y = operands(key, n, m, aligned, 2)
    ind = np.ascontiguousarray(m + 1 - (np.arange(m) * (m + 2)) // m, dtype=np.int64)     # m + 1 downwards
    if m > 2:
        ind[1], ind[-1] = ind[0], 0
    tag = _tag('copy_cols', key, n, m, aligned)
    _lib.check(L.rlh_copy_cols(code, n, m, _lib.host_ptr(ind), x.ptr(0), x.ld, y.ptr(), y.ld))
    y.check(x.host[ind, :n], None, tag)
    x.check_unchanged(tag)
    # source and destination in one allocation, disjoint columns: 2 m + 2 columns, the first m + 1 are the source
    big = Block(DT[key], n, 2 * m, leading_dimension(n, DT[key], aligned, 2), base_shift(DT[key], aligned), which=3)
    src = np.ascontiguousarray((np.arange(m)[::-1] * 3) % (m + 1), dtype=np.int64)
    _lib.check(L.rlh_copy_cols(code, n, m, _lib.host_ptr(src), big.ptr(0), big.ld, big.ptr(m + 1), big.ld))
    want = big.window().copy()                                   # columns 1 .. 2 m of the storage
    want[m:] = big.host[src, :n]
    big.check(want, None, tag + ' one allocation')


def conj(key, n, m, aligned):
    _lib, L, code = _lib_and_code(key)
    x, = operands(key, n, m, aligned, 1)
    _lib.check(L.rlh_conj(code, n, m, x.ptr(), x.ld))
    x.check(np.conj(x.window()), None, _tag('conj', key, n, m, aligned))


CONVERSIONS = [('s', 'd'), ('d', 's'), ('c', 'z'), ('z', 'c')]


def convert(src, dst, n, m, aligned):
    _lib, L, code = _lib_and_code(src)
    x, y = operands(src, n, m, aligned, 2, dtypes=[DT[src], DT[dst]])
    _lib.check(L.rlh_convert(code, _lib.dtype_code(DT[dst]), n, m, x.ptr(), x.ld, y.ptr(), y.ld))
    y.check(x.window().astype(DT[dst]), None, _tag('convert to %s' % dst, src, n, m, aligned))
    x.check_unchanged()


# inputs whose product with the scale 0.75 lies exactly half way between two bfloat16 numbers:
# 1.359375 * 0.75 = 1 + 5 / 256 (the even neighbour is below: 0x3F82), 1.390625 * 0.75 = 1 + 11 / 256 (above: 0x3F86)
BF16_TIES = np.array([1.359375, 1.390625, -1.359375, -1.390625, 0.0, 1.0])
BF16_TIE_BITS = np.array([0x3F82, 0x3F86, 0xBF82, 0xBF86, 0x0000, 0x3F40], dtype=np.uint16)


def bf16(key, n, m, aligned):
    """rlh_bf16_pack (from float32 and float64, scale 0.75, ties included) and rlh_bf16_unpack."""
    assert key in 'sd'
    _lib, L, code = _lib_and_code(key)
    x, h, y = operands(key, n, m, aligned, 3, dtypes=[DT[key], np.uint16, DT[key]])
    vals = x.window().copy()
    vals *= (10.0 ** ((np.arange(vals.size) % 31) - 15)).reshape(vals.shape).astype(DT[key])   # a wide range of exponents
    flat = vals.reshape(-1)
    k = min(flat.size, BF16_TIES.size)
    flat[flat.size - k:] = BF16_TIES[:k]                          # (the last rows of the last column)
    x.set_window(vals)
    tag = _tag('bf16', key, n, m, aligned)
    _lib.check(L.rlh_bf16_pack(code, n, m, x.ptr(), x.ld, 0.75, h.ptr(), h.ld))
    want = ops.bf16_bits(np.float32(0.75) * x.window().astype(np.float32))
    assert np.array_equal(want.reshape(-1)[flat.size - k:], BF16_TIE_BITS[:k])
    bits = h.check(want, None, tag + ' pack')
    x.check_unchanged(tag)
    h.host[1:m + 1, :n] = bits                                    # what the device now holds
    _lib.check(L.rlh_bf16_unpack(code, n, m, h.ptr(), h.ld, y.ptr(), y.ld))
    y.check((bits.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(DT[key]), None, tag + ' unpack')
    h.check_unchanged(tag)


def dots(key, n, m, aligned, same=False):
    """rlh_dots to a device buffer with guard elements and to the host."""
    _lib, L, code = _lib_and_code(key)
    x, y = operands(key, n, m, aligned, 2)
    if same:
        y = x
    out = Block(DT[key], m, 1, m + 5, which=5)
    h = np.zeros((m,), dtype=DT[key])
    _lib.check(L.rlh_dots(code, n, m, x.ptr(), x.ld, y.ptr(), y.ld, out.ptr(), _lib.host_ptr(h)))
    u = unit_roundoff(key)
    want = np.einsum('ir,ir->i', np.conj(y.wide()), x.wide())
    bound = (n + 2) * u * np.einsum('ir,ir->i', np.abs(y.wide()), np.abs(x.wide()))
    tag = _tag('dots', key, n, m, aligned)
    win = out.check(want[None, :], bound[None, :], tag)
    assert same_bytes(win[0], h), 'device and host results differ ' + tag
    x.check_unchanged(tag)
    y.check_unchanged(tag)


def dots_transp(key, n, m, aligned):
    _lib, L, code = _lib_and_code(key)
    x, y = operands(key, n, m, aligned, 2)
    out = Block(DT[key], n, 1, n + 5, which=5)
    _lib.check(L.rlh_dots_transp(code, n, m, x.ptr(), x.ld, y.ptr(), y.ld, out.ptr()))
    u = unit_roundoff(key)
    want = np.einsum('ir,ir->r', np.conj(y.wide()), x.wide())
    bound = (m + 2) * u * np.einsum('ir,ir->r', np.abs(y.wide()), np.abs(x.wide()))
    tag = _tag('dots_transp', key, n, m, aligned)
    win = out.check(want[None, :], bound[None, :], tag)
    if m == 0:
        assert not win.any()
    x.check_unchanged(tag)
    y.check_unchanged(tag)


def absmax(key, n, m, aligned):
    """rlh_absmax: the extreme value in the last row of the last column (complex: in its imaginary part), then
    nowhere in the window but just outside it."""
    _lib, L, code = _lib_and_code(key)
    x, = operands(key, n, m, aligned, 1)
    tag = _tag('absmax', key, n, m, aligned)
    out = ctypes.c_double()
    big = -1234.5
    x.host[m + 1, :] *= 1e3                                      # larger values in the guard column after the window
    x.host[m, n:] *= 1e3                                         # and in the padding rows of the last column
    x.host[m, n - 1] = complex(1.0, big) if key in 'cz' else big
    x.upload()
    _lib.check(L.rlh_absmax(code, n, m, x.ptr(), x.ld, ctypes.byref(out)))
    assert out.value == abs(big), tag
    x.host[m, n - 1] = 0
    x.upload()
    _lib.check(L.rlh_absmax(code, n, m, x.ptr(), x.ld, ctypes.byref(out)))
    w = x.window()
    assert out.value == float(max(np.abs(w.real).max(), np.abs(w.imag).max())), tag
    x.check_unchanged(tag)


def _index_buffer(idx):
    from raleigh_amd import _lib
    from raleigh_amd.algebra.hip.memory import DeviceBuffer
    buf = DeviceBuffer(idx.nbytes)
    _lib.check(_lib.lib().rlh_h2d(buf.ptr, _lib.host_ptr(idx), idx.nbytes))
    return buf


GATHER_COUNTS = [1, 257, 5000]


def gather_rows(key, nidx, m, aligned, n=4099):
    """rlh_gather_rows (key 'h': rlh_gather_rows_bf16 on 16-bit words): unsorted, repeated indices, ldo > nidx."""
    from raleigh_amd import _lib
    L = _lib.lib()
    dt = np.uint16 if key == 'h' else DT[key]
    x = Block(dt, n, m, leading_dimension(n, dt, aligned, 0), base_shift(dt, aligned), which=0)
    o = Block(dt, nidx, m, leading_dimension(nidx, dt, aligned, 1), base_shift(dt, aligned), which=1)
    assert o.ld > nidx
    rng = np.random.default_rng(nidx)
    idx = rng.integers(0, n, nidx, dtype=np.int64)
    idx[0] = n - 1
    if nidx > 2:
        idx[-1], idx[nidx // 2] = 0, idx[nidx // 2 - 1]
    ib = _index_buffer(idx)
    if key == 'h':
        _lib.check(L.rlh_gather_rows_bf16(nidx, ib.ptr, m, x.ptr(), x.ld, o.ptr(), o.ld))
    else:
        _lib.check(L.rlh_gather_rows(_lib.dtype_code(dt), nidx, ib.ptr, m, x.ptr(), x.ld, o.ptr(), o.ld))
    tag = _tag('gather_rows', key, nidx, m, aligned)
    o.check(x.window()[:, idx], None, tag)
    x.check_unchanged(tag)


# ---------------------------------------------------------------------------------------------------- part 2
def many_ld(n, which=0):
    """16-byte aligned columns with padding rows after every one (n = 8, 24, 33 -> 12, 28, 36 and so on)."""
    return (n + 3) // 4 * 4 + 4 * (which + 1)


def many_operands(key, n, m, count, dtypes=None):
    out = []
    for i in range(count):
        dt = DT[key] if dtypes is None else dtypes[i]
        ld = many_ld(n, i) * (2 if np.dtype(dt).itemsize == 2 else 1)
        out.append(Block(dt, n, m, ld, which=i))
    return out


def many_vectors(key, n, m):
    """Every entry point that takes a number of columns, on a block of m short vectors: same references and bounds
    as above, whole arrays compared (guard columns, padding rows)."""
    _lib, L, code = _lib_and_code(key)
    u = unit_roundoff(key)
    cx = key in 'cz'
    tag = _tag('many', key, n, m, True)
    x, y, o = many_operands(key, n, m, 3)
    xw, yw = x.wide(), y.wide()
    # dots, absmax
    h = np.zeros((m,), dtype=DT[key])
    _lib.check(L.rlh_dots(code, n, m, x.ptr(), x.ld, y.ptr(), y.ld, None, _lib.host_ptr(h)))
    want = np.einsum('ir,ir->i', np.conj(yw), xw)
    bound = (n + 2) * u * np.einsum('ir,ir->i', np.abs(yw), np.abs(xw))
    err = np.abs(h.astype(WIDE[key]) - want)
    assert np.all(err <= bound), 'dots: column %d %s' % (int(np.argmax(err - bound)), tag)
    dev = Block(DT[key], m, 1, m + 5, which=5)
    _lib.check(L.rlh_dots(code, n, m, x.ptr(), x.ld, y.ptr(), y.ld, dev.ptr(), None))
    assert same_bytes(dev.check(want[None, :], bound[None, :], tag + ' dots')[0], h)
    out = ctypes.c_double()
    for col in (m - 1, 32767, 0):
        save = x.host[col + 1, n - 1]
        x.host[col + 1, n - 1] = complex(1.0, -77.25) if cx else -77.25
        x.upload()
        _lib.check(L.rlh_absmax(code, n, m, x.ptr(), x.ld, ctypes.byref(out)))
        assert out.value == 77.25, 'absmax: extreme value in column %d %s' % (col, tag)
        x.host[col + 1, n - 1] = save
    x.upload()
    # axpy, axpy_cols, lincomb (distinct and in place)
    alpha = axpy_alpha(key)
    a2 = np.array([np.real(alpha), np.imag(alpha)], dtype=np.float64)
    k = 8 if cx else 2
    _lib.check(L.rlh_axpy(code, n, m, _lib.host_ptr(a2), x.ptr(), x.ld, y.ptr(), y.ld))
    win = y.check(yw + alpha * xw, k * u * (abs(alpha) * np.abs(xw) + np.abs(yw)), tag + ' axpy')
    y.host[1:m + 1, :n] = win
    yw = y.wide()
    s = coefficients(key, m, 21)
    sw = s.astype(WIDE[key])[:, None]
    _lib.check(L.rlh_axpy_cols(code, n, m, _lib.host_ptr(s), x.ptr(), x.ld, y.ptr(), y.ld))
    win = y.check(yw + sw * xw, k * u * (np.abs(sw) * np.abs(xw) + np.abs(yw)), tag + ' axpy_cols')
    y.host[1:m + 1, :n] = win
    yw = y.wide()
    b = coefficients(key, m, 22)
    bw = b.astype(WIDE[key])[:, None]
    want = sw * xw + bw * yw
    bound = k * u * (np.abs(sw) * np.abs(xw) + np.abs(bw) * np.abs(yw))
    _lib.check(L.rlh_lincomb_cols(code, n, m, _lib.host_ptr(s), x.ptr(), x.ld, _lib.host_ptr(b), y.ptr(), y.ld,
                                  o.ptr(), o.ld))
    o.check(want, bound, tag + ' lincomb')
    _lib.check(L.rlh_lincomb_cols(code, n, m, _lib.host_ptr(s), x.ptr(), x.ld, _lib.host_ptr(b), y.ptr(), y.ld,
                                  y.ptr(), y.ld))
    win = y.check(want, bound, tag + ' lincomb in place')
    y.host[1:m + 1, :n] = win
    x.check_unchanged(tag)
    # scale: multiply, divide with a zero divisor in the last panel
    sc = coefficients(key, m, 23).astype(WIDE[key]) * 1.1
    _lib.check(L.rlh_scale_cols(code, n, m, _lib.host_ptr(np.ascontiguousarray(sc).view(np.float64)), 1, y.ptr(), y.ld))
    if cx:
        want = sc[:, None] * y.wide()
        win = y.check(want, 4 * u * np.abs(want), tag + ' scale multiply')
    else:
        win = y.check(y.window() * sc.astype(DT[key])[:, None], None, tag + ' scale multiply')
    y.host[1:m + 1, :n] = win
    sc[m - 2] = 0
    _lib.check(L.rlh_scale_cols(code, n, m, _lib.host_ptr(np.ascontiguousarray(sc).view(np.float64)), 0, y.ptr(), y.ld))
    nz = sc != 0
    want = y.wide()
    want[nz] = want[nz] / sc[nz, None]
    bound = (6 if cx else 3) * u * np.abs(want)
    bound[~nz] = 0.0
    y.check(want, bound, tag + ' scale divide')
    # copy, copy_cols (every column from the far end of the source, guard columns included), conj
    _lib.check(L.rlh_copy(code, n, m, x.ptr(), x.ld, o.ptr(), o.ld))
    o.check(x.window(), None, tag + ' copy')
    ind = np.ascontiguousarray(m + 1 - np.arange(m), dtype=np.int64)
    ind[1] = ind[0]
    _lib.check(L.rlh_copy_cols(code, n, m, _lib.host_ptr(ind), x.ptr(0), x.ld, o.ptr(), o.ld))
    o.check(x.host[ind, :n], None, tag + ' copy_cols')
    if cx:
        _lib.check(L.rlh_conj(code, n, m, x.ptr(), x.ld))
        x.check(np.conj(x.window()), None, tag + ' conj')
        x.upload()
    else:
        x.check_unchanged(tag)
    del y, o
    # convert, bf16 pack / unpack (real blocks), gather_rows
    other = {'s': 'd', 'z': 'c'}[key]
    c, = many_operands(key, n, m, 1, dtypes=[DT[other]])
    _lib.check(L.rlh_convert(code, _lib.dtype_code(DT[other]), n, m, x.ptr(), x.ld, c.ptr(), c.ld))
    c.check(x.window().astype(DT[other]), None, tag + ' convert')
    del c
    if not cx:
        h16, back = many_operands(key, n, m, 2, dtypes=[np.uint16, DT[key]])
        _lib.check(L.rlh_bf16_pack(code, n, m, x.ptr(), x.ld, 0.75, h16.ptr(), h16.ld))
        bits = h16.check(ops.bf16_bits(np.float32(0.75) * x.window().astype(np.float32)), None, tag + ' bf16 pack')
        _lib.check(L.rlh_bf16_unpack(code, n, m, h16.ptr(), h16.ld, back.ptr(), back.ld))
        back.check((bits.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(DT[key]), None, tag + ' bf16 unpack')
        idx16 = np.array([n - 1, 0, n // 2, n // 2, 1], dtype=np.int64)
        ib = _index_buffer(idx16)
        g16 = Block(np.uint16, idx16.size, m, 8, which=2)
        h16.host[1:m + 1, :n] = bits
        _lib.check(L.rlh_gather_rows_bf16(idx16.size, ib.ptr, m, h16.ptr(), h16.ld, g16.ptr(), g16.ld))
        g16.check(bits[:, idx16], None, tag + ' gather_rows_bf16')
        del h16, back, g16
    idx = np.array([n - 1, 0, n // 2, n // 2, 1, n - 1, 2], dtype=np.int64)
    ib = _index_buffer(idx)
    g = Block(DT[key], idx.size, m, 12, which=4)
    _lib.check(L.rlh_gather_rows(code, idx.size, ib.ptr, m, x.ptr(), x.ld, g.ptr(), g.ld))
    g.check(x.window()[:, idx], None, tag + ' gather_rows')
    x.check_unchanged(tag)


def many_rows_through_the_classes(key):
    """A 70001 x 24 C-ordered data matrix: Matrix.dots / absmax, AMatrix.frobenius2 / scale, and scale, add, copy
    and zero on the shallow view of its rows."""
    from raleigh_amd.algebra.hip import Matrix, Vectors
    from raleigh_amd.algebra.dense_matrix import AMatrix
    rows, cols = 70001, 24
    u = unit_roundoff(key)
    cx = key in 'cz'
    a = _pool(DT[key], rows * cols + 3)[3:rows * cols + 3].reshape(rows, cols).copy()
    a[rows - 1, cols - 1] = complex(0.5, -99.0) if cx else -99.0
    aw = a.astype(WIDE[key])
    want = np.einsum('ir,ir->i', np.conj(aw), aw)
    bound = (cols + 2) * u * np.abs(want)
    d = Matrix(a).dots()
    assert d.shape == (rows,) and d.dtype == DT[key]
    assert np.all(np.abs(d.astype(WIDE[key]) - want) <= bound)
    assert Matrix(a).absmax() == 99.0
    A = AMatrix(a)
    assert A.scale() == 99.0
    # (a sum of 70001 terms formed on the host in the working precision: 70001 u on top of the row bounds)
    assert abs(A.frobenius2() - float(np.sum(want.real))) <= (rows + cols + 2) * u * float(np.sum(want.real))
    v = A.as_vectors()
    assert v.nvec() == rows and v.dimension() == cols
    w = Vectors(cols, rows, data_type=DT[key])
    v.copy(w)
    assert same_bytes(w.data(), a)
    s = coefficients(key, rows, 31).astype(WIDE[key]) * 1.1
    s[rows - 3] = 0
    w.scale(s)
    got = w.data().astype(WIDE[key])
    nz = s != 0
    ref = aw.copy()
    ref[nz] = ref[nz] / s[nz, None]
    assert np.all(np.abs(got - ref) <= (6 if cx else 3) * u * np.abs(ref))
    assert same_bytes(w.data()[rows - 3], a[rows - 3])
    w.scale(s, multiply=True)
    cur = got
    got = w.data().astype(WIDE[key])
    ref = s[:, None] * cur
    assert np.all(np.abs(got - ref) <= 4 * u * np.abs(ref))
    cur = got
    alpha = axpy_alpha(key)
    w.add(v, alpha)
    got = w.data().astype(WIDE[key])
    k = 8 if cx else 2
    assert np.all(np.abs(got - (cur + alpha * aw)) <= k * u * (abs(alpha) * np.abs(aw) + np.abs(cur)))
    cur = got
    t = coefficients(key, rows, 32)
    w.add(v, t)
    got = w.data().astype(WIDE[key])
    tw = t.astype(WIDE[key])[:, None]
    assert np.all(np.abs(got - (cur + tw * aw)) <= k * u * (np.abs(tw) * np.abs(aw) + np.abs(cur)))
    w.zero()
    assert not w.data().any()
    assert same_bytes(v.data(), a)                     # the data matrix itself was only read


def gram_keeps_its_limit():
    """rlh_gram refuses more than 32768 vectors in a window with its own message, before anything is launched (the
    pointers are never looked at)."""
    import pytest
    from raleigh_amd import _lib
    L = _lib.lib()
    for mx, my in ((32769, 1), (1, 32769), (70001, 70001)):
        with pytest.raises(_lib.RlhError, match='rlh_gram: more than 32768 vectors in a window'):
            _lib.check(L.rlh_gram(0, 8, mx, None, 8, my, None, 8, None, None))
