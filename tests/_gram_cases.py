"""The Gram kernels behind rlh_gram / rlh_gram_multi, entry by entry, shared by the CPU tier (tests/fake_lib.py: shows
that NumPy in the working precision meets every bound below and that every exact case is exact) and the GPU tier
(librlhip.so, every dispatch path of gram_impl / gram_multi_impl in raleigh_amd/csrc/gram.hip), through the raw C ABI.

Harness.  Every operand is a host array of m + 2 columns of ld elements, uploaded whole; the call sees the window of m
columns that starts at column 1, rows [0, n).  Rows n .. ld - 1 of every column and the two guard columns hold NaN, so
an entry that reads past n or past the window comes back non-finite (columns that a kernel clamps to the window's last
one are legitimate: the entries they feed are never written out).  The result goes to a device buffer with 8 guard
elements of a fixed byte pattern before and after its my * mx entries, which must come back untouched.  Every case
makes the call twice -- with d_out and h_out, and with h_out alone (results of at most 1 MiB: the finalize kernel then
writes into mapped host memory) -- and requires the three results to be the same bits (the reduction order is fixed, so
this is also the repeatability check), and the operands to be bit-identical after the calls.  Alignment legs as in
_columnwise_cases: 16-byte aligned columns with ld a multiple of 32 elements, or no column 16-byte aligned (complex128:
the base shifted by 8 bytes); every operand has its own ld.  A self-Gram passes the same pointer, ld and width on both
sides; the overlapping case takes Y one column later in the same block, which is NOT a self-Gram.

Two kinds of input.
  * Rounding bound on full-mantissa data (Gaussian; Gaussian with column j scaled by 2^(-3 (j mod 12)) -- exact, small
    entries next to large ones; all-positive, where S = |G| and the bound is a relative one).  The reference is formed
    from the uploaded values in numpy.longdouble (64-bit mantissa, asserted), real and imaginary parts separately:
    Re G_ij = sum(y_r x_r + y_i x_i), Im G_ij = sum(y_r x_i - y_i x_r).  Every real component of every entry is held to
        |got - ref| <= (L + 2) u S,
    u the unit roundoff of the type's real part, L the number of real products in the component (n real, 2 n complex)
    and S the sum of their absolute values formed in the reference precision.  This is the project's dots bound: a sum
    of L products in ANY order has the error (1 + u)^(L) - 1 relative to S to first order -- every product is rounded
    once and then passes through at most L - 1 additions -- L u S; one more u S covers the second-order terms for
    L u < 0.01 and one the final rounding of gram_finalize's double-precision combination to the working type (the
    double-precision sums of the partials themselves add 2^-53 per level, far below u for s / c and inside the same
    L u S count for d / z since the partials replace additions, they do not add any).  Fused multiply-adds only remove
    roundings.  The bound is derived, never measured; n * mx * my of these cases is capped (the reference costs about
    6 ns per product).
  * Exact data, where the loops run deep: integers uniform in [-2, 2] (s, c) or [-2^14, 2^14] (d, z).  Every product and
    every partial sum in any order is then an integer below 2^24 / 2^52 (asserted on sum |.| of the reference, per
    case), hence exactly representable, and the kernel's result must equal a float64 BLAS reference BIT FOR BIT, through
    h_out and d_out, on every leg (so all legs agree with the default leg bit for bit, too).  This is what catches a
    dropped, doubled or misplaced row or tile, a wrongly mirrored tile, or a partial stored in a narrower type, however
    long n is.  (The reference is normalised to +0: an accumulator that starts at +0 never becomes -0.)

Shapes.  v = real-view width (m, or 2 m complex).  The streaming kernel's tile is 32 rows (d, z) or 64 (s, c) and its
workgroup has 16 / 8 / 4 waves at <= 16 / <= 32 / more staged columns; the workgroup kernel's chunk is 512 / sizeof(real)
rows (64 or 128), twice / four times that in MODE 3 / 4, 256 bytes per column in the 128 x 128 quadrant panel, and 32
complex rows in gram_z_dma_kernel (which needs n >= 2048).  Widths sit on every boundary of pick_tiles and the dispatch
(8 | 9, 16 | 17, 32 | 33, 64 | 65, 128 | 129); short rows are 1, 3, one less than / equal to / one more than every tile
or chunk, waves x tile + 1, 4099, and around the DMA kernel's threshold and its second sweep.  Deep rows (exact only) are
computed from the CU count: tile (3 G + G / 2) + 5 per streaming wave shape (waves own 3 and 4 tiles, ragged tail),
chunk (3 G + G / 2 + 1) + 3 for the two-register-set loops of MODE 1 / 2 (G = 8 CU, the residency cap, or CU under
RLH_GRAM_WG_PER_CU=1), chunk (2 * 8 CU + 1) + 1 for the grid-stride loops of MODE 0 / 3 / 4 and the quadrant kernels.

route() below restates the dispatch conditions of gram_impl; it only names the kernel family that a case reaches (for
the error / bound table that every test prints) and the panel side inside which gram_finalize mirrors a self-Gram (the
one place where exact Hermitian symmetry is guaranteed and therefore asserted).  It never changes a check.
"""

import ctypes
import os

import numpy as np

from _columnwise_cases import DT, KEYS, base_shift, leading_dimension, same_bytes, unit_roundoff

LD = np.longdouble
REAL = {'s': np.float32, 'd': np.float64, 'c': np.float32, 'z': np.float64}
NC = {'s': 1, 'd': 1, 'c': 2, 'z': 2}
TILE = {'s': 64, 'd': 32, 'c': 64, 'z': 32}          # rows per tile of the streaming kernel
CHUNK = {'s': 128, 'd': 64, 'c': 128, 'z': 64}       # rows per chunk of the workgroup kernel (MODE 0 / 1 / 2)
GUARD = 8
BOUND_KINDS = ['gauss', 'scaled', 'positive']
KINDS = BOUND_KINDS + ['exact']

# (mx, my) of the two-operand requests and m of the self requests: real types, then complex counts
WIDTHS_REAL = [(1, 1), (8, 8), (9, 1), (1, 9), (16, 16), (17, 16), (16, 17), (32, 32), (33, 32), (32, 33), (33, 33),
               (48, 20), (9, 33), (16, 64), (64, 64), (64, 1), (65, 9), (9, 65), (65, 64), (64, 65), (65, 33), (100, 20), (20, 100), (128, 128), (129, 128),
               (129, 40), (200, 150), (257, 130)]
SELF_REAL = [1, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 200]
WIDTHS_CPLX = [(1, 1), (4, 4), (5, 1), (1, 5), (5, 4), (4, 5), (8, 8), (9, 8), (8, 9), (16, 16), (17, 16), (16, 17),
               (17, 17), (24, 10), (8, 17), (5, 32), (32, 32), (32, 1), (33, 4), (4, 33), (33, 32), (32, 33), (33, 33), (33, 17), (50, 10), (10, 50),
               (64, 64), (65, 64), (64, 65), (64, 33), (65, 20), (100, 75), (129, 65)]
SELF_CPLX = [1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 100]
OVERLAP = {'s': 20, 'd': 20, 'c': 10, 'z': 10}


def widths(key):
    return WIDTHS_REAL if key in 'sd' else WIDTHS_CPLX


def self_widths(key):
    return SELF_REAL if key in 'sd' else SELF_CPLX


def short_rows(key):
    t, c = TILE[key], CHUNK[key]
    rows = {1, 3, 4099}
    for b in (t, c, 2 * c, 4 * c, 16 * t, 8 * t, 4 * t):
        rows.update((b - 1, b, b + 1) if b <= 4 * c else (b + 1,))
    return sorted(rows)


def dma_rows(cu):
    return [2047, 2048, 2049, 2079, 2080, 2081, 32 * cu + 33]


def is_dma_width(key, mx, my):
    return key == 'z' and 32 < mx <= 64 and 32 < my <= 64


# ---------------------------------------------------------------------------------------------------- dispatch model
def _env(name, default):
    v = os.environ.get(name)
    return default if v is None or v == '' else int(v)


def pick_tiles(v):
    return 1 if v <= 16 else (2 if v <= 32 else 4)


def route(key, n, mx, my, same, aligned):
    """(kernel family, panel side of gram_finalize's mirror) that rlh_gram reaches under the present environment."""
    vx, vy = mx * NC[key], my * NC[key]
    PI, PJ = pick_tiles(vy), pick_tiles(vx)
    npi, npj = -(-vy // (16 * PI)), -(-vx // (16 * PJ))
    if _env('RLH_GRAM_STREAM', 1) and aligned and vx <= 64 and vy <= 64 and (vx > 8 or vy > 8):
        return 'stream', (16 if vx <= 16 else (32 if vx <= 32 else 64))
    pipe, rows_cap = _env('RLH_GRAM_PIPE', 1), _env('RLH_GRAM_ROWS', 4)
    mode = 0
    if aligned and pipe != 0:
        if same and npi == 1 and npj == 1 and PI == PJ and PI <= 2:
            mode = 2
        elif not same and pipe >= 2 and PI * PJ <= 4:
            mode = 1
        elif PI <= 2 and PJ <= 2 and rows_cap >= 2:
            mode = 4 if (PI * PJ == 1 and rows_cap >= 4) else 3
    if key == 'z' and _env('RLH_GRAM_ZDMA', 1) and aligned and not same and is_dma_width(key, mx, my) and n >= 2048:
        return 'dma', None
    quad = os.environ.get('RLH_GRAM_QUAD', '1')[:1] != '0'
    if aligned and (vx > 64 or vy > 64) and vx > 32 and vy > 32 and quad:
        return ('quad128 symmetric' if same and vx <= 128 else 'quad128'), 128
    if aligned and 32 < vx <= 64 and 32 < vy <= 64 and quad:
        return ('quad64 symmetric' if same else 'quad64'), 64
    return 'mode %d%s' % (mode, '' if aligned else ' unaligned'), (16 * PI if PI == PJ else None)


RATIOS = {}          # (type, kernel family) -> largest error / bound seen
HERMITIAN = {}       # (type, kernel family) -> [self-Grams, exactly Hermitian ones, ones with a real diagonal]


def ratios_text():
    lines = ['largest error / bound: ' + ', '.join('%s %s %.3f' % (k[0], k[1], r) for k, r in sorted(RATIOS.items()))]
    if HERMITIAN:
        lines.append('self-Grams (exactly Hermitian, real diagonal) of all: '
                     + ', '.join('%s %s (%d, %d) of %d' % (k[0], k[1], h[1], h[2], h[0]) for k, h in sorted(HERMITIAN.items())))
    return '\n'.join(lines)


# ---------------------------------------------------------------------------------------------------- data
_POOLS = {}


def _pool(key, exact):
    k = (REAL[key], exact)
    if k not in _POOLS:
        rng = np.random.default_rng(777 + int(exact) + 2 * np.dtype(REAL[key]).itemsize)
        size = 1 << 22
        if exact:
            lim = 2 if key in 'sc' else 1 << 14
            p = rng.integers(-lim, lim + 1, size).astype(REAL[key])
        else:
            p = rng.standard_normal(size).astype(REAL[key])
        p.setflags(write=False)
        _POOLS[k] = p
    return _POOLS[k]


def values(key, kind, m, n, which=0):
    """The (m, n) values of a window (one column of the block per row), of the working type."""
    nc = NC[key]
    count = m * n * nc
    pool = _pool(key, kind == 'exact')
    off = (1013 * which + 7 + 131 * m + 17 * n) % 65521
    v = pool[off:off + count] if off + count <= pool.size else np.resize(pool, off + count)[off:]
    v = v.reshape(m, n * nc).copy()
    if kind == 'scaled':
        v *= (2.0 ** (-3.0 * (np.arange(m) % 12)))[:, None].astype(REAL[key])
    elif kind == 'positive':
        np.abs(v, out=v)
    return v.view(DT[key]) if nc == 2 else v


def _lib():
    from raleigh_amd import _lib as L
    return L


class Block:
    """(m + 2) columns of ld elements on the host (one column per ROW of `host`) and on the device: the window's values
    in columns 1 .. m, rows [0, n), NaN everywhere else."""

    def __init__(self, key, n, m, aligned, which, vals):
        from raleigh_amd.algebra.hip.memory import DeviceBuffer
        L = _lib()
        self.dtype = np.dtype(DT[key])
        self.n, self.m, self.es = n, m, self.dtype.itemsize
        self.ld = leading_dimension(max(n, 1), self.dtype, aligned, which)
        nan = complex(np.nan, np.nan) if NC[key] == 2 else np.nan
        self.host = np.full((m + 2, self.ld), nan, dtype=self.dtype)
        self.host[1:m + 1, :n] = vals
        self._buf = DeviceBuffer(self.host.nbytes + 16, zero=False)
        self.base = self._buf.ptr + base_shift(self.dtype, aligned)
        L.check(L.lib().rlh_h2d(self.base, L.host_ptr(self.host), self.host.nbytes))

    def ptr(self, column=1):
        return self.base + column * self.ld * self.es

    def window(self, first=1, count=None):
        return self.host[first:first + (self.m if count is None else count), :self.n]

    def check_unchanged(self, what=''):
        L = _lib()
        out = np.empty_like(self.host)
        L.check(L.lib().rlh_d2h(L.host_ptr(out), self.base, out.nbytes))
        assert same_bytes(out, self.host), 'operand modified ' + what


class Result:
    """A device buffer of `count` result entries between two runs of GUARD elements of the byte 0xA5."""

    def __init__(self, key, count):
        from raleigh_amd.algebra.hip.memory import DeviceBuffer
        L = _lib()
        self.dtype, self.count = np.dtype(DT[key]), count
        self.host = np.frombuffer(b'\xa5' * ((count + 2 * GUARD) * self.dtype.itemsize), dtype=self.dtype)
        self._buf = DeviceBuffer(self.host.nbytes, zero=False)
        L.check(L.lib().rlh_h2d(self._buf.ptr, L.host_ptr(self.host), self.host.nbytes))

    def ptr(self):
        return self._buf.ptr + GUARD * self.dtype.itemsize

    def fetch(self, what=''):
        L = _lib()
        out = np.empty_like(self.host)
        L.check(L.lib().rlh_d2h(L.host_ptr(out), self._buf.ptr, out.nbytes))
        assert same_bytes(out[:GUARD], self.host[:GUARD]), 'elements in front of the result modified ' + what
        assert same_bytes(out[GUARD + self.count:], self.host[GUARD + self.count:]), 'elements after the result modified ' + what
        return out[GUARD:GUARD + self.count].copy()

    def untouched(self, what=''):
        L = _lib()
        out = np.empty_like(self.host)
        L.check(L.lib().rlh_d2h(L.host_ptr(out), self._buf.ptr, out.nbytes))
        assert same_bytes(out, self.host), 'result buffer written to ' + what


# ---------------------------------------------------------------------------------------------------- references
def _parts(w, dtype):
    return (w.real.astype(dtype), w.imag.astype(dtype)) if np.iscomplexobj(w) else (w.astype(dtype), None)


def reference(xw, yw, dtype):
    """Real components (Re, Im or None) of G = conj(Y) X^T and the sums S of the absolute values of their products, all
    formed in `dtype` from the (m, n) windows xw, yw."""
    xr, xi = _parts(xw, dtype)
    yr, yi = _parts(yw, dtype)
    if xi is None:
        return [(yr @ xr.T, np.abs(yr) @ np.abs(xr).T)]
    axr, axi, ayr, ayi = np.abs(xr), np.abs(xi), np.abs(yr), np.abs(yi)
    return [(yr @ xr.T + yi @ xi.T, ayr @ axr.T + ayi @ axi.T), (yr @ xi.T - yi @ xr.T, ayr @ axi.T + ayi @ axr.T)]


def verify(key, got, xw, yw, kind, tag, family):
    """`got` (my, mx) against the reference of the windows: bit for bit on exact data, the rounding bound otherwise."""
    n = xw.shape[1]
    comps = [got.real, got.imag] if NC[key] == 2 else [got]
    if kind == 'exact':
        ref = reference(xw, yw, np.float64)
        for c, (g, s) in zip(comps, ref):
            assert s.size == 0 or s.max() < (2.0 ** 24 if key in 'sc' else 2.0 ** 52), 'the data is not exact ' + tag
            want = np.ascontiguousarray((g + 0.0).astype(REAL[key]))
            have = np.ascontiguousarray(c)
            if not same_bytes(have, want):
                bad = np.argwhere(~(have == want))
                raise AssertionError('%d entries differ from the exact result, first (i, j) = %s: %r for %r %s'
                                     % (len(bad), tuple(bad[0]), have[tuple(bad[0])], want[tuple(bad[0])], tag))
        return
    assert np.finfo(LD).nmant >= 63, 'numpy.longdouble is no wider than float64 here'
    u = unit_roundoff(key)
    L = n * NC[key]
    for c, (g, s) in zip(comps, reference(xw, yw, LD)):
        err = np.abs(c.astype(LD) - g)
        bound = (L + 2) * LD(u) * s
        bad = ~(err <= bound)
        if bad.any():
            i, j = np.argwhere(bad)[0]
            raise AssertionError('entry (%d, %d): error %.3e above the bound %.3e %s' % (i, j, err[i, j], bound[i, j], tag))
        pos = bound > 0
        if pos.any():
            r = float((err[pos] / bound[pos]).max())
            RATIOS[(key, family)] = max(RATIOS.get((key, family), 0.0), r)


def check_mirror(key, got, side, tag, family):
    """A self-Gram on Gaussian data: entries below the diagonal tiles of a panel are copies that gram_finalize takes from
    the mirrored entry (complex: RR, II swap places and RI, IR swap with their signs: the conjugate) -- asserted; whether
    the whole result is exactly Hermitian with a real diagonal is only recorded."""
    m = got.shape[0]
    h = HERMITIAN.setdefault((key, family), [0, 0, 0])
    h[0] += 1
    h[1] += int(np.array_equal(got, np.conj(got.T)))
    h[2] += int(not np.any(np.diagonal(got).imag)) if NC[key] == 2 else 1
    if side is None or not isinstance(_lib().library(), ctypes.CDLL):      # (the stand-in of the CPU tier mirrors nothing)
        return
    v = np.arange(m) * NC[key]
    panel, tile = v // side, (v % side) // 16
    served = (panel[:, None] == panel[None, :]) & (tile[:, None] > tile[None, :])
    mirrored = np.conj(got.T)
    assert np.array_equal(got[served], mirrored[served]), 'mirrored entries differ from their originals ' + tag


# ---------------------------------------------------------------------------------------------------- one request
def _tag(key, n, mx, my, aligned, kind, form):
    env = ' '.join('%s=%s' % (k[9:], v) for k, v in sorted(os.environ.items()) if k.startswith('RLH_GRAM_'))
    return '[gram %s n=%d mx=%d my=%d %s %s %s %s]' % (key, n, mx, my, 'aligned' if aligned else 'unaligned', kind, form, env)


def call_gram(key, n, x, xcol, mx, y, ycol, my, tag, small=1 << 20):
    """rlh_gram with d_out and h_out, then (small results) with h_out alone: the same bits three times, guards intact."""
    L = _lib()
    lib, code = L.lib(), L.dtype_code(DT[key])
    res = Result(key, my * mx)
    h1 = np.full((my, mx), 7, dtype=DT[key])
    L.check(lib.rlh_gram(code, n, mx, x.ptr(xcol), x.ld, my, y.ptr(ycol), y.ld, res.ptr(), L.host_ptr(h1)))
    dev = res.fetch(tag).reshape(my, mx)
    assert same_bytes(dev, h1), 'd_out and h_out differ ' + tag
    if h1.nbytes <= small:
        h2 = np.full((my, mx), 7, dtype=DT[key])
        L.check(lib.rlh_gram(code, n, mx, x.ptr(xcol), x.ld, my, y.ptr(ycol), y.ld, None, L.host_ptr(h2)))
        assert same_bytes(h2, h1), 'a repeated call (h_out alone) gives other bits ' + tag
    return h1


def gram(key, n, mx, my, aligned=True, kind='exact', form='two'):
    """One request: form 'two' (distinct blocks), 'self' (the same window on both sides) or 'overlap' (Y one column later
    in X's block)."""
    tag = _tag(key, n, mx, my, aligned, kind, form)
    if form == 'two':
        x = Block(key, n, mx, aligned, 0, values(key, kind, mx, n, 0))
        y = Block(key, n, my, aligned, 1, values(key, kind, my, n, 1))
        xw, yw, ycol = x.window(), y.window(), 1
    else:
        assert mx == my
        extra = 1 if form == 'overlap' else 0
        x = y = Block(key, n, mx + extra, aligned, 0, values(key, kind, mx + extra, n, 0))
        xw, yw, ycol = x.window(1, mx), x.window(1 + extra, mx), 1 + extra
    got = call_gram(key, n, x, 1, mx, y, ycol, my, tag)
    x.check_unchanged(tag)
    if y is not x:
        y.check_unchanged(tag)
    family, side = route(key, n, mx, my, form == 'self', aligned)
    verify(key, got, xw, yw, kind, tag, family)
    if form == 'self' and kind == 'gauss':
        check_mirror(key, got, side, tag, family)
    return got


BOUND_CAP = {'s': 1000000, 'd': 1000000, 'c': 500000, 'z': 500000}    # n * mx * my of a bound case (cost of the reference)


def requests(key, only=None):
    """(mx, my, form) of the short legs; `only(mx, my, form)` restricts them."""
    out = [(mx, my, 'two') for mx, my in widths(key)] + [(m, m, 'self') for m in self_widths(key)]
    out.append((OVERLAP[key], OVERLAP[key], 'overlap'))
    return [r for r in out if only is None or only(*r)]


def short(key, aligned, cu, only=None, rows=None):
    """Every request at every short row count: exact data always; one of the three full-mantissa data sets, in turn, where
    the reference is affordable, always at one row more than a tile, and at 2048 and 2081 rows where the DMA kernel runs."""
    turn = 0
    for mx, my, form in requests(key, only):
        ns = list(rows or short_rows(key))
        if is_dma_width(key, mx, my) and rows is None:
            ns += dma_rows(cu)
        for n in ns:
            gram(key, n, mx, my, aligned, 'exact', form)
            if n * mx * my <= BOUND_CAP[key] or n == TILE[key] + 1 or (is_dma_width(key, mx, my) and n in (2048, 2081)):
                gram(key, n, mx, my, aligned, BOUND_KINDS[turn % 3], form)
                turn += 1


def narrow(mx, my, form):
    """Requests that the workgroup kernel serves with 64 real columns or fewer on both sides (what RLH_GRAM_STREAM=0 and
    the once-per-process switches change)."""
    return max(mx, my) <= 64


# ---------------------------------------------------------------------------------------------------- deep rows
def deep_stream(key, cu):
    """A wave of the streaming kernel owns 3 and 4 tiles, ragged tail: one case per wave shape (16, 8, 4 waves)."""
    t = TILE[key]
    shapes = {'s': [(16, 9, 9, 'self'), (8, 9, 1, 'two'), (4, 17, 1, 'two')],
              'd': [(16, 9, 9, 'self'), (8, 9, 1, 'two'), (4, 17, 1, 'two')],
              'c': [(8, 5, 1, 'two')], 'z': [(8, 5, 1, 'two')]}[key]
    for waves, mx, my, form in shapes:
        G = cu * waves
        gram(key, t * (3 * G + G // 2) + 5, mx, my, True, 'exact', form)


def deep_pipelined(key, cu, per_cu, shapes):
    """The two-register-set loop of MODE 1 / 2 and the three-way tail behind it: more than three full chunks per workgroup."""
    G = per_cu * cu
    n = CHUNK[key] * (3 * G + G // 2 + 1) + 3
    for mx, my, form in shapes:
        gram(key, n, mx, my, True, 'exact', form)


def deep_strided(key, cu, chunk, mx, my, form, aligned=True):
    """The grid-stride loop of MODE 0 / 3 / 4 and of the quadrant kernels: more than two sweeps of the largest grid."""
    gram(key, chunk * (2 * 8 * cu + 1) + 1, mx, my, aligned, 'exact', form)


def mode2_widths(key):
    return [(m, m, 'self') for m in ([8] if key in 'sd' else [4])]


# ---------------------------------------------------------------------------------------------------- rlh_gram_multi
class Segments:
    """A window made of blocks side by side, every block with its own leading dimension."""

    def __init__(self, key, n, ms, aligned, kind, first, shared=None):
        self.blocks = [shared[k] if shared and k in shared else Block(key, n, m, aligned, first + k, values(key, kind, m, n, first + k))
                       for k, m in enumerate(ms)]
        self.ptrs = (ctypes.c_void_p * len(ms))(*[b.ptr() for b in self.blocks])
        self.lds = np.array([b.ld for b in self.blocks], dtype=np.int64)
        self.ms = np.array(ms, dtype=np.int64)
        self.total = int(sum(ms))

    def window(self):
        return np.concatenate([b.window() for b in self.blocks], axis=0)


def call_multi(key, n, xs, ys, tag):
    L = _lib()
    lib, code = L.lib(), L.dtype_code(DT[key])
    res = Result(key, ys.total * xs.total)
    h1 = np.full((ys.total, xs.total), 7, dtype=DT[key])
    args = (code, n, len(xs.blocks), xs.ptrs, L.host_ptr(xs.lds), L.host_ptr(xs.ms), len(ys.blocks), ys.ptrs,
            L.host_ptr(ys.lds), L.host_ptr(ys.ms))
    L.check(lib.rlh_gram_multi(*args, res.ptr(), L.host_ptr(h1)))
    assert same_bytes(res.fetch(tag).reshape(h1.shape), h1), 'd_out and h_out differ ' + tag
    h2 = np.full_like(h1, 7)
    L.check(lib.rlh_gram_multi(*args, None, L.host_ptr(h2)))
    assert same_bytes(h2, h1), 'a repeated call (h_out alone) gives other bits ' + tag
    for b in xs.blocks + ys.blocks:
        b.check_unchanged(tag)
    return h1


def multi(key, n, mxs, mys, aligned=True, kind='exact', singles=False):
    """[Y_0 | Y_1 | ..]^H [X_0 | X_1 | ..]: every entry against the reference of the concatenated windows (so the stacked
    result equals the stacked results of single calls -- exactly on exact data, within the bound otherwise; `singles`
    makes those calls, too, and compares)."""
    tag = '[gram_multi %s n=%d mx=%s my=%s %s %s]' % (key, n, mxs, mys, 'aligned' if aligned else 'unaligned', kind)
    xs = Segments(key, n, mxs, aligned, kind, 0)
    ys = Segments(key, n, mys, aligned, kind, len(mxs))
    got = call_multi(key, n, xs, ys, tag)
    verify(key, got, xs.window(), ys.window(), kind, tag, 'multi')
    if singles:
        r0 = 0
        for yb in ys.blocks:
            c0 = 0
            for xb in xs.blocks:
                part = call_gram(key, n, xb, 1, xb.m, yb, 1, yb.m, tag + ' single')
                if kind == 'exact':
                    assert same_bytes(part, np.ascontiguousarray(got[r0:r0 + yb.m, c0:c0 + xb.m])), 'stacked result differs from the single calls ' + tag
                else:
                    verify(key, part, xb.window(), yb.window(), kind, tag + ' single', 'multi')
                c0 += xb.m
            r0 += yb.m
    return got


def multi_shapes(key):
    """(segments of X, segments of Y): 2, 3 and 4 per side, widths of 1, boundaries that are no multiples of 16."""
    if key in 'sd':
        return {'stream': [([7, 9], [1, 15]), ([1, 14, 17], [5, 16, 1]), ([3, 1, 20, 8], [16, 1, 30, 17]), ([20, 10], [9, 5]),
                           ([9, 5], [20, 10]), ([7, 8], [30, 20])],
                'split': [([20], [40, 33, 70]), ([130], [1, 64]), ([33], [3, 1, 40, 20])],
                'kernel': [([40, 1, 33], [17, 50]), ([16, 17, 1, 40], [1, 30, 31, 9]), ([3, 5], [7, 1]), ([100, 30], [5]),
                           ([40, 30], [20, 10])]}
    return {'stream': [([3, 5], [1, 7]), ([1, 6, 9], [2, 8, 1]), ([3, 1, 12, 8], [8, 1, 15, 8]), ([10, 5], [5, 2]), ([5, 2], [10, 5]),
                       ([3, 4], [15, 10])],
            'split': [([10], [20, 17, 35]), ([65], [1, 32]), ([17], [3, 1, 20, 10])],
            'kernel': [([20, 1, 17], [9, 25]), ([8, 9, 1, 20], [1, 15, 16, 5]), ([3, 1], [2, 1]), ([50, 15], [3]), ([20, 15], [10, 5])]}


def multi_all(key, aligned):
    t = TILE[key]
    for group in multi_shapes(key).values():
        for mxs, mys in group:
            for n in (3, t + 1, 4099):
                multi(key, n, mxs, mys, aligned, 'exact', singles=(n == t + 1))
            multi(key, 3, mxs, mys, aligned, 'gauss')
            multi(key, t + 1, mxs, mys, aligned, 'scaled', singles=True)
            multi(key, CHUNK[key] + 1, mxs, mys, aligned, 'positive')


def shared_block(key, n, kind='exact'):
    """[Y | X]^H X with X of 20 real columns at the column offsets 0, 16, 32 (the X block is found in the Y window and
    staged once) and 24 (it is not): the same bits as the request made with a copy of X."""
    assert key in 'sd'
    mx = 20
    for off in (0, 16, 32, 24):
        mys = [mx, 20] if off == 0 else [off, mx]
        at = 0 if off == 0 else 1
        tag = '[gram_multi shared %s n=%d offset %d %s]' % (key, n, off, kind)
        xs = Segments(key, n, [mx], True, kind, 0)
        ys = Segments(key, n, mys, True, kind, 1, shared={at: xs.blocks[0]})
        got = call_multi(key, n, xs, ys, tag)
        verify(key, got, xs.window(), ys.window(), kind, tag, 'multi shared')
        copy = Block(key, n, mx, True, 5, xs.blocks[0].window())
        yc = Segments(key, n, mys, True, kind, 1, shared={at: copy})
        assert same_bytes(yc.window(), ys.window())
        other = call_multi(key, n, xs, yc, tag + ' copy')
        if kind == 'exact':
            assert same_bytes(got, other), 'aliased and copied X give different bits ' + tag
        else:
            verify(key, other, xs.window(), yc.window(), kind, tag + ' copy', 'multi shared')


def reduction_batch(key):
    """ReductionBatch.gram of stacked windows and of single blocks through the Vectors class, exact data."""
    from raleigh_amd.algebra.hip import Vectors
    n = 4099
    x, y, z = (values(key, 'exact', m, n, w) for w, m in enumerate((20, 33, 1)))
    X, Y, Z = Vectors(x.copy()), Vectors(y.copy()), Vectors(z.copy())
    rb = X.reduction_batch()
    rb.gram([X], [Y, X])
    rb.gram([X, Z], [Z, Y, X])
    rb.gram([Y], [Y])
    g1, g2, g3 = rb.run()
    tag = '[reduction batch %s]' % key
    verify(key, g1, x, np.concatenate([y, x]), 'exact', tag, 'multi')
    verify(key, g2, np.concatenate([x, z]), np.concatenate([z, y, x]), 'exact', tag, 'multi')
    verify(key, g3, y, y, 'exact', tag, 'multi')


# ---------------------------------------------------------------------------------------------------- wide windows
def wide(key, mx, my, form='two'):
    """n = 40 and thousands of columns: many panels, the grid's first dimension capped by the workspace."""
    n = 40
    tag = _tag(key, n, mx, my, True, 'exact', form)
    x = Block(key, n, mx, True, 0, values(key, 'exact', mx, n, 0))
    y = x if form == 'self' else Block(key, n, my, True, 1, values(key, 'exact', my, n, 1))
    got = call_gram(key, n, x, 1, mx, y, 1, my, tag)
    verify(key, got, x.window(), y.window(), 'exact', tag, route(key, n, mx, my, form == 'self', True)[0])
    x.check_unchanged(tag)


SELF_FITS, SELF_REFUSED = 2688, 3457       # float64: 21 x 21 and 28 x 28 panels of 128 x 128 doubles (55 and 98 MiB)


def workspace_refusal():
    """More 128 x 128 panels than the 96 MiB workspace holds even with one workgroup each: refused with its message,
    nothing written, and the library works afterwards."""
    import pytest
    L = _lib()
    m, n = SELF_REFUSED, 40
    x = Block('d', n, m, True, 0, values('d', 'exact', m, n, 0))
    res = Result('d', m * m)
    with pytest.raises(L.RlhError, match='exceeds the reduction workspace'):
        L.check(L.lib().rlh_gram(L.dtype_code(np.float64), n, m, x.ptr(), x.ld, m, x.ptr(), x.ld, res.ptr(), None))
    res.untouched('by a refused call')
    x.check_unchanged()
    gram('d', 40, 65, 33)


# ---------------------------------------------------------------------------------------------------- degenerate
def degenerate(key):
    L = _lib()
    lib, code = L.lib(), L.dtype_code(DT[key])
    for aligned in (True, False):
        for mx, my in ((1, 1), (9, 5), (70, 40)):
            got = gram(key, 0, mx, my, aligned, 'exact')           # n = 0: zeros, guards intact
            assert not got.any()
        got = multi(key, 0, [3, 1], [2, 9], aligned, 'exact')
        assert not got.any()
    x = Block(key, 5, 3, True, 0, values(key, 'exact', 3, 5, 0))
    for mx, my in ((0, 3), (3, 0), (0, 0)):                        # nothing to compute: nothing written, nothing read
        res = Result(key, 4)
        h = np.full((4,), 7, dtype=DT[key])
        L.check(lib.rlh_gram(code, 5, mx, x.ptr() if mx else None, x.ld, my, x.ptr() if my else None, x.ld, res.ptr(), L.host_ptr(h)))
        res.untouched('by an empty request')
        assert np.all(h == 7)


def refusals():
    """Every RLH_REQUIRE of the two entry points, once, with its message; the library works afterwards."""
    import pytest
    L = _lib()
    lib = L.lib()
    x = Block('d', 5, 3, True, 0, values('d', 'exact', 3, 5, 0))
    h = np.zeros((9,))
    hp, p, ld = L.host_ptr(h), x.ptr(), x.ld

    def refused(message, *args):
        with pytest.raises(L.RlhError, match=message):
            L.check(lib.rlh_gram(*args))

    refused('rlh_gram: unknown dtype 7', 7, 5, 3, p, ld, 3, p, ld, None, hp)
    refused('rlh_gram: negative size', 1, -1, 3, p, ld, 3, p, ld, None, hp)
    refused('rlh_gram: negative size', 1, 5, -3, p, ld, 3, p, ld, None, hp)
    refused('rlh_gram: negative size', 1, 5, 3, p, ld, -3, p, ld, None, hp)
    refused('rlh_gram: more than 32768 vectors in a window', 1, 5, 32769, p, ld, 3, p, ld, None, hp)
    refused('rlh_gram: more than 32768 vectors in a window', 1, 5, 3, p, ld, 32769, p, ld, None, hp)
    refused('rlh_gram: null block pointer', 1, 5, 3, None, ld, 3, p, ld, None, hp)
    refused('rlh_gram: null block pointer', 1, 5, 3, p, ld, 3, None, ld, None, hp)
    refused('rlh_gram: leading dimension smaller than n', 1, 5, 3, p, 4, 3, p, ld, None, hp)
    refused('rlh_gram: leading dimension smaller than n', 1, 5, 3, p, ld, 3, p, 4, None, hp)
    refused('rlh_gram: no output buffer', 1, 5, 3, p, ld, 3, p, ld, None, None)

    ptrs = (ctypes.c_void_p * 5)(p, p, p, p, p)
    holes = (ctypes.c_void_p * 2)(p, None)
    lds = np.full((5,), ld, dtype=np.int64)
    short_ld = np.array([ld, 4], dtype=np.int64)
    ms = np.array([1, 2, 1, 1, 1], dtype=np.int64)
    zero = np.array([1, 0], dtype=np.int64)
    many = np.array([32768, 1], dtype=np.int64)
    lp, mp = L.host_ptr(lds), L.host_ptr(ms)

    def refused_multi(message, *args):
        with pytest.raises(L.RlhError, match=message):
            L.check(lib.rlh_gram_multi(*args))

    refused_multi('rlh_gram_multi: unknown dtype -1', -1, 5, 2, ptrs, lp, mp, 2, ptrs, lp, mp, None, hp)
    for nx, ny in ((0, 2), (5, 2), (2, 0), (2, 5)):
        refused_multi('rlh_gram_multi: 1 to 4 blocks per window', 1, 5, nx, ptrs, lp, mp, ny, ptrs, lp, mp, None, hp)
    refused_multi('rlh_gram_multi: bad arguments', 1, -1, 2, ptrs, lp, mp, 2, ptrs, lp, mp, None, hp)
    for hole in range(6):
        args = [ptrs, lp, mp, ptrs, lp, mp]
        args[hole] = None
        refused_multi('rlh_gram_multi: bad arguments', 1, 5, 2, *args[:3], 2, *args[3:], None, hp)
    for bad in ((holes, lp, mp), (ptrs, L.host_ptr(short_ld), mp), (ptrs, lp, L.host_ptr(zero))):
        refused_multi('rlh_gram_multi: bad block 1 of the right window', 1, 5, 2, *bad, 2, ptrs, lp, mp, None, hp)
        refused_multi('rlh_gram_multi: bad block 1 of the left window', 1, 5, 2, ptrs, lp, mp, 2, *bad, None, hp)
    refused_multi('rlh_gram_multi: more than 32768 vectors in a window', 1, 5, 2, ptrs, lp, L.host_ptr(many), 1, ptrs, lp, mp, None, hp)
    refused_multi('rlh_gram_multi: more than 32768 vectors in a window', 1, 5, 1, ptrs, lp, mp, 2, ptrs, lp, L.host_ptr(many), None, hp)
    refused_multi('rlh_gram_multi: no output buffer', 1, 5, 2, ptrs, lp, mp, 2, ptrs, lp, mp, None, None)
    x.check_unchanged()
    gram('d', 5, 3, 3)
    multi('d', 5, [1, 2], [2, 1])


# ---------------------------------------------------------------------------------------------------- child legs
# The switches below are read once per process (function-local statics of gram_impl / gram_blocks_per_cu), so each leg
# runs in a child process of its own: tests/_gram_child.py <leg>, with the leg's variables in its environment.
def _all_keys(fn):
    for key in KEYS:
        fn(key)


def _leg_pipe2(cu):                 # MODE 1 for every two-operand request of at most 4 tiles; MODE 2 as by default
    _all_keys(lambda key: short(key, True, cu, narrow))
    deep_pipelined('d', cu, 8, [(16, 16, 'two'), (32, 32, 'two')])
    deep_pipelined('s', cu, 8, [(32, 16, 'two')])


def _leg_pipe0(cu):                 # MODE 0 where MODE 1 - 4 ran
    _all_keys(lambda key: short(key, True, cu, narrow))
    deep_strided('d', cu, 64, 16, 16, 'self')


def _leg_rows1(cu):                 # MODE 0 in place of MODE 3 / 4
    _all_keys(lambda key: short(key, True, cu, narrow))
    deep_strided('d', cu, 64, 17, 1, 'two')


def _leg_rows2(cu):                 # MODE 3 in place of MODE 4
    _all_keys(lambda key: short(key, True, cu, narrow))
    deep_strided('d', cu, 128, 3, 2, 'two')


def _leg_zdma0(cu):                 # the quadrant panels where the DMA kernel ran
    short('z', True, cu, lambda mx, my, form: is_dma_width('z', mx, my) and form == 'two', rows=dma_rows(cu) + [4099])


def _leg_wg1_pipe2(cu):             # one workgroup per CU: G = CU in the two-register-set loops
    for key in KEYS:
        short(key, True, cu, narrow, rows=[TILE[key] + 1, 4099])
        deep_pipelined(key, cu, 1, [(m * 2 // NC[key], m2 * 2 // NC[key], 'two') for m, m2 in ((8, 8), (16, 8), (16, 16))]
                       + [(m * 2 // NC[key], m * 2 // NC[key], 'self') for m in (4, 8, 16)])


def _leg_wg1(cu):
    for key in KEYS:
        short(key, True, cu, lambda mx, my, form: max(mx, my) * NC[key] > 64 or max(mx, my) * NC[key] <= 8,
              rows=[1, CHUNK[key] + 1, 4099])
        deep_pipelined(key, cu, 1, mode2_widths(key))
    deep_strided('d', cu, 32, 65, 33, 'two')


LEGS = {
    'pipe2': ({'RLH_GRAM_STREAM': '0', 'RLH_GRAM_PIPE': '2'}, _leg_pipe2),
    'pipe0': ({'RLH_GRAM_STREAM': '0', 'RLH_GRAM_PIPE': '0'}, _leg_pipe0),
    'rows1': ({'RLH_GRAM_STREAM': '0', 'RLH_GRAM_ROWS': '1'}, _leg_rows1),
    'rows2': ({'RLH_GRAM_STREAM': '0', 'RLH_GRAM_ROWS': '2'}, _leg_rows2),
    'zdma0': ({'RLH_GRAM_ZDMA': '0'}, _leg_zdma0),
    'wg1_pipe2': ({'RLH_GRAM_WG_PER_CU': '1', 'RLH_GRAM_STREAM': '0', 'RLH_GRAM_PIPE': '2'}, _leg_wg1_pipe2),
    'wg1': ({'RLH_GRAM_WG_PER_CU': '1'}, _leg_wg1),
}


def run_child(leg, cu, timeout=600, fake=False, env_override=None):
    """Starts tests/_gram_child.py for one leg as a fresh process (one at a time, its own time limit, never retried) and
    returns the completed process."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if not k.startswith('RLH_GRAM_')}
    env.update(LEGS[leg][0])
    env.update(env_override or {})
    here = os.path.dirname(os.path.abspath(__file__))
    cmd = [sys.executable, os.path.join(here, '_gram_child.py'), leg, '--cu', str(cu)] + (['--fake'] if fake else [])
    return subprocess.run(cmd, env=env, timeout=timeout,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
