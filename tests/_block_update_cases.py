"""The block update behind rlh_block_update / rlh_block_update2 / rlh_block_update2x2, element by element, shared by the
CPU tier (tests/fake_lib.py: shows that NumPy in the working precision meets every bound below and that every exact case
is exact) and the GPU tier (librlhip.so, every kernel family that launch_update of raleigh_amd/csrc/update.hip reaches),
through the raw C ABI.

Harness.  Every operand is a Block of _columnwise_cases (m + 2 columns of its own ld, uploaded whole); the call sees the
window of m columns that starts at column 1 (or further in: WINDOW_COLUMNS), rows [0, n).  In the sources the guard columns
and rows n .. ld - 1 hold NaN, so a value read past the window that reaches a stored element comes back non-finite (the
kernels' clamped re-reads of the last valid row or column are legitimate: they multiply zero padding of Q or are never
stored).  A result block holds NaN outside its window as well, and for beta = 0 inside it, too: it must come back finite.
After the call the result's guard columns and padding rows must be the uploaded bytes (the test of Block.check, for a
window at any column) and every source bit-identical to what was uploaded.  Every call is made twice, the second time on
re-uploaded results, and must give the same bits.  Alignment legs: every operand 16-byte aligned; none (the convention of
_columnwise_cases: complex128 with its base shifted by 8 bytes); 'mixed' -- sources aligned, results not (complex types:
the matrix-core kernel with unaligned stores; real types: one row per lane); 'mixed_x2' -- only X2 unaligned.  The host
coefficient matrices are C-ordered, F-ordered or a window of a larger host array (row stride > m).

Two kinds of input.
  * Rounding bound on full-mantissa data (Gaussian; Gaussian with column j scaled by 2^(-3 (j mod 12))), alpha = 0.3 or
    0.3 - 0.7j.  The reference is formed from the uploaded values in numpy.longdouble (64-bit mantissa, asserted), real and
    imaginary parts separately.  Every real component of every result element is held to
        |got - ref| <= (L + 4) u S,
    u the unit roundoff of the real part, L the number of real products summed into the component (k + k2 real,
    2 (k + k2) complex, one more for beta = 1) and S the sum of the absolute values of those products in the reference
    precision, alpha expanded into them (a complex coefficient component counts as |a0 q_r| + |a1 q_i| or
    |a0 q_i| + |a1 q_r|), plus |Out0| for beta = 1.  L products summed in ANY order cost L u S, with or without fused
    operations and on either matrix-core shape; two more u cover forming alpha q (the library rounds a double-precision
    product once; the NumPy stand-in rounds alpha and the product to the working type), one the final rounding and one
    the second-order terms for L u < 0.01.  Derived, never measured; n (k + k2) m of these cases is capped (BOUND_CAP).
  * Exact data: integers uniform in [-2, 2] (s, c) or [-2^14, 2^14] (d, z) in X, Q and Out0, alpha one of 1, -0.5 and
    (complex) 1 - 2j.  Every product and partial sum in any order is then a multiple of 1/2 below 2^23 / 2^51 (asserted on
    the reference's S, per case), hence exact, and the result must equal a float64 BLAS reference BIT FOR BIT (normalised
    to +0) on every leg and kernel family.  This is what catches a dropped, doubled or misplaced k-step, row, tile or
    column however large the case; all large cases are exact-only.
One more bit-for-bit relation: RLH_UPDATE_NT=1 is a template parameter of the same arithmetic, so its result on bound data
equals the default one (nt_equals_default).

Shapes.  Row counts are chosen per kernel (stream_rows, MFMA_ROWS, VALU_ROWS) and coefficient shapes per dispatch limit;
pairings() gives every row count of a kernel one shape of each family that the kernel has under the leg's environment
(stream KS8 / KS16 / KS32, mfma KS8 / KS16 / KS32, valu JT x RV) and every shape three row counts, never the full product.
The CPU tier asserts that coverage family by family.

route() restates the dispatch of launch_update and the two-pass split of rlh_block_update2x2.  It names the kernel family
that a case reaches, for the table that every test prints and for the pairing of rows with shapes; it never changes what
a case checks.
"""

import os

import numpy as np

from _columnwise_cases import DT, KEYS, Block, base_shift, leading_dimension, operands, same_bytes, unit_roundoff
from _gram_cases import LD, NC, REAL, values

ES = {'s': 4, 'd': 8, 'c': 8, 'z': 16}

# ---------------------------------------------------------------------------------------------------- geometry
TR = {'s': 64, 'd': 32}                 # block_update_stream_kernel: TR = 16 * V rows of a tile, V = 16 / sizeof(R)
STREAM_WG_TILES = 32                    # ... 4 waves x kUpdTilesPerWave = 8 tiles of a workgroup
MFMA_TILE = 16                          # block_update_mfma_kernel: a wave takes 16 rows, a workgroup 4 waves
KS_MAX = 32                             # kMfmaUpdKS: k-steps of 4 columns that the register sets hold
LDS_STREAM, LDS_MFMA = 64 * 1024, 160 * 1024      # update_stream_ok / launch_update: coefficients in the LDS
RVMAX = {'s': 4, 'd': 2, 'c': 2, 'z': 1}          # launch_update: RVMAX = 16 / sizeof(T) rows per lane ...
RV_BYTES = 512                                    # ... where RVMAX * JT * sizeof(T) <= 512 (else one row per lane)
SLOT = 1 << 20                          # kRingSlotBytes (common.h): one staging slot of coefficients
KMAX = 1024                             # block_update_impl: rows of Q per launch at the most
NT_BYTES = 192 << 20                    # update_nt: operands beyond this take the non-temporal instantiation

COMMON_ROWS = [1, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4099]
# block_update_kernel: a wave owns 64 RV rows and a workgroup 256 RV, RV = 1, 2 or 4: one short of, equal to and one past
# both (RV = 2: 127 - 129 are not among the common rows), and one n with every residue of n mod RV past a workgroup
VALU_ROWS = sorted(set(COMMON_ROWS) | {b * rv + d for rv in (1, 2, 4) for b in (64, 256) for d in (-1, 0, 1)}
                   | {256 * rv + 1 + r for rv in (2, 4) for r in range(rv)})
# block_update_mfma_kernel: a wave takes a tile of 16 rows and a workgroup 4 waves (all among the common rows)
MFMA_ROWS = COMMON_ROWS


def stream_rows(key):
    """1, 2, 3 and 8 tiles per wave (4, 5 | 8, 9 | 12, 13 | 31, 32 tiles of a workgroup) with a ragged last tile before
    and after; a second workgroup of one wave."""
    t = TR[key]
    rows = {i * t + d for i in (1, 4, 5, 8, 9, 12, 13, 31, 32) for d in (-1, 0, 1)}
    return sorted(rows | {STREAM_WG_TILES * t + 1, (STREAM_WG_TILES + 1) * t + 1})


# (k, m) of one source.  Real: both sides of k >= 8 and m >= 8, the three KS sets (k <= 32, 64, 128) and k = 129, the LDS
# limit (d: (128, 64) | (128, 65); s: (128, 128) | (128, 129)), every JT (m = 8 | 9, 16 | 17, 32 | 33, 64 | 65) with two
# and three panels and float64's 64-column panel
REAL_SHAPES = [(1, 1), (3, 7), (4, 9), (5, 16), (7, 8), (8, 7), (8, 8), (9, 9), (12, 17), (13, 100), (16, 16), (16, 1),
               (17, 129), (31, 33), (32, 32), (33, 31), (63, 15), (64, 64), (64, 49), (65, 48), (127, 47), (128, 64),
               (128, 65), (128, 128), (128, 129), (129, 8), (129, 33), (300, 9), (300, 65), (9, 63), (32, 65)]
# complex: both sides of k >= 16 and m >= 16, the KS sets, the LDS limit (z: (128, 80) | (128, 81); c: (128, 160) |
# (128, 161)), JT = 8 and 16 with several panels
CPLX_SHAPES = [(1, 1), (3, 7), (8, 8), (9, 9), (15, 16), (16, 15), (16, 16), (17, 17), (31, 33), (32, 32), (33, 31),
               (63, 16), (64, 64), (65, 48), (127, 47), (128, 64), (128, 80), (128, 81), (128, 160), (128, 161), (129, 16),
               (129, 33), (300, 17), (5, 65), (13, 100), (12, 129)]
# (k1, k2) of two sources: k1 no multiple of 4 (zero rows between the two coefficient blocks), a sum of 7 | 8, and 33
# k-steps ((124, 5), (128, 1)), one past what the matrix-core kernels take
TWO_SOURCES = [(1, 1), (3, 4), (3, 5), (5, 3), (7, 1), (4, 4), (16, 16), (17, 15), (30, 34), (64, 64), (65, 63), (100, 28),
               (124, 5), (128, 1)]
TWO_SOURCE_WIDTHS = [1, 8, 9, 16, 17, 32, 33, 48, 64, 65, 100]
# (ma, mb) of two results: the split inside and on a 16-column tile and a JT panel
TWO_RESULTS = [(1, 1), (4, 4), (7, 9), (8, 8), (10, 27), (16, 16), (17, 33), (32, 32), (33, 31), (50, 60), (64, 64)]
TWO_RESULT_SOURCES = [(4, 4), (16, 16), (17, 15), (30, 34), (64, 64), (3, 5)]
WINDOW_COLUMNS = (3, 6)                 # first column of a window inside a wider block
BOUND_CAP = {'s': 500000, 'd': 500000, 'c': 150000, 'z': 150000}     # n (k + k2) m of a bound case
ALIGNMENTS = {                          # 16-byte aligned: (X1, X2, results)
    'aligned': (True, True, True), 'unaligned': (False, False, False),
    'mixed': (True, True, False), 'mixed_x2': (True, False, True)}


def shapes(key):
    return REAL_SHAPES if key in 'sd' else CPLX_SHAPES


def shape_rows(key, valu=False):
    """Rows that every coefficient shape meets: below a tile, ragged in the middle, one that starts a second workgroup."""
    if valu or key in 'cz':
        return [15, 4099, 256 * RVMAX[key] + 1] if valu else [15, 4099, 4 * MFMA_TILE + 1]
    return [TR[key] - 1, 4099, STREAM_WG_TILES * TR[key] + 1]


def family_rows(key, family):
    """The row counts chosen for the kernel behind a family name of route()."""
    if family.startswith('stream'):
        return sorted(set(COMMON_ROWS + stream_rows(key)))
    return MFMA_ROWS if family.startswith('mfma') else VALU_ROWS


def pairings(key, shape_list, per_shape, align='aligned', form='one'):
    """(n, shape) of a leg: the shapes are grouped by the kernel family that route() names under the present
    environment, and every row count chosen for a family's kernel meets one shape of that family, in turn -- so a row
    of the streaming kernel meets three shapes there, one for each of KS8 / KS16 / KS32, the complex rows likewise,
    and a row of the VALU kernel one shape for every JT it has.  Every shape meets the rows of `per_shape`.  Never
    the full product.  (route() chooses which cases run; it never changes what a case checks.)"""
    groups = {}
    for shape in shape_list:
        k1, k2 = (shape[0], 0) if form == 'one' else shape[0]
        groups.setdefault(route(key, 4099, k1, k2, shape[1], align, form), []).append(shape)
    out = {(n, shape) for shape in shape_list for n in per_shape}
    for family, members in groups.items():
        out |= {(n, members[i % len(members)]) for i, n in enumerate(family_rows(key, family))}
    return sorted(out)


# ---------------------------------------------------------------------------------------------------- dispatch model
def _env(name, default):
    v = os.environ.get(name)
    return default if v is None or v == '' else int(v)


def panel(key, m):
    """JT of block_update_impl / block_update2_impl."""
    if m <= 8:
        return 8
    if m <= 16 or key in 'cz':
        return 16
    return 64 if key == 'd' and m > 32 else 32


def chunk_rows(key, m):
    """kmax of block_update_impl: rows of Q whose padded block fits a staging slot."""
    jt = panel(key, m)
    return min(SLOT // ((m + jt - 1) // jt * jt * ES[key]) // 4 * 4, KMAX)


def route(key, n, k, k2, m, alignment, form, beta=0):
    """The kernel family that the request reaches under the present environment (m: (ma, mb) for form '2x2')."""
    ax1, ax2, aout = ALIGNMENTS[alignment]
    suffix = ''
    if form == '2x2':
        ma, mb = m
        m = ma + mb
        ks = (k + 3) // 4 + (k2 + 3) // 4
        both, worst = (m + 15) // 16 * ks * 64 * ES[key], (max(ma, mb) + 15) // 16 * ks * 64 * ES[key]
        if key in 'cz' and ks <= KS_MAX and both > LDS_MFMA and worst <= LDS_MFMA:
            m, suffix = ma, ' two passes'
    if form == 'one':
        k2 = 0
        if k > chunk_rows(key, m):
            k, suffix = chunk_rows(key, m), ' k-chunked'
    jt = panel(key, m)
    ks = ((k + 3) // 4 + (k2 + 3) // 4) if k2 > 0 else (k + 3) // 4
    lds = (m + 15) // 16 * ks * 64 * ES[key]
    src = ax1 and (ax2 or k2 == 0)
    nt_env = os.environ.get('RLH_UPDATE_NT')
    nt = (int(nt_env) != 0) if nt_env else n * (k + k2 + (2 if beta else 1) * m) * ES[key] > NT_BYTES
    kset = 8 if ks <= 8 else (16 if ks <= 16 else 32)
    if key in 'cz':
        if _env('RLH_UPDATE_MFMA', 1) and k + k2 >= 16 and m >= 16 and ks <= KS_MAX and lds <= LDS_MFMA and src:
            return 'mfma KS%d%s%s' % (kset, '' if aout else ' unaligned results', suffix)
    elif _env('RLH_UPDATE_STREAM', 1) and k + k2 >= 8 and m >= 8 and ks <= KS_MAX and lds <= LDS_STREAM and src and aout:
        return 'stream KS%d%s%s' % (kset, ' NT' if nt else '', suffix)
    rv = 1
    if RVMAX[key] > 1 and RVMAX[key] * jt * ES[key] <= RV_BYTES and _env('RLH_UPDATE_RV', 1) and src and aout:
        rv = RVMAX[key]
    return 'valu JT%d RV%d%s%s' % (jt, rv, ' NT' if nt and rv > 1 else '', suffix)


RATIOS = {}          # (type, kernel family) -> [cases, largest error / bound seen]


def ratios_text():
    lines = ['%-2s %-36s %6s  %s' % ('', 'kernel family', 'cases', 'largest error / bound')]
    for (key, family), (count, ratio) in sorted(RATIOS.items()):
        lines.append('%-2s %-36s %6d  %.3f' % (key, family, count, ratio))
    return '\n'.join(lines)


def _reached(key, family, ratio=0.0):
    r = RATIOS.setdefault((key, family), [0, 0.0])
    r[0] += 1
    r[1] = max(r[1], ratio)


# ---------------------------------------------------------------------------------------------------- harness
def _lib():
    from raleigh_amd import _lib as L
    return L


def _nan(key):
    return complex(np.nan, np.nan) if NC[key] == 2 else np.nan


class Operand:
    """The window of m columns at column `col` of a Block of m + 2 col columns: `vals` (m, n) in the window (None: NaN),
    NaN everywhere else."""

    def __init__(self, key, n, m, aligned, which, vals=None, col=1):
        dt = np.dtype(DT[key])
        self.n, self.m, self.col = n, m, col
        self.blk = Block(dt, n, m + 2 * (col - 1), leading_dimension(max(n, 1), dt, aligned, which), base_shift(dt, aligned),
                         which=which)
        self.ld = self.blk.ld
        self.fill(vals, _nan(key))

    def fill(self, vals, rest):
        self.blk.host[...] = rest
        if vals is not None:
            self.blk.host[self.col:self.col + self.m, :self.n] = vals
        self.blk.upload()

    def ptr(self, shift=0):
        return self.blk.ptr(self.col + shift)

    def window(self):
        return self.blk.host[self.col:self.col + self.m, :self.n]

    def upload(self):
        self.blk.upload()

    def unchanged(self, what=''):
        self.blk.check_unchanged(what)

    def result(self, what=''):
        """The downloaded window; every other byte of the block must be what was uploaded (as Block.check)."""
        got = self.blk.fetch()
        c, m, n = self.col, self.m, self.n
        win = got[c:c + m, :n].copy()
        got[c:c + m, :n] = self.window()
        assert same_bytes(got, self.blk.host), 'guard columns or padding rows of the result modified ' + what
        return win


def coefficients(key, kind, k, m, layout, which):
    """A k x m host matrix of the working type: C-ordered, F-ordered or a window of a larger array."""
    q = values(key, kind, k, m, which)
    if layout == 'F':
        return np.asfortranarray(q)
    if layout == 'window':
        big = np.full((k + 2, m + 5), _nan(key), dtype=DT[key])
        big[1:k + 1, 2:m + 2] = q
        return big[1:k + 1, 2:m + 2]
    assert layout == 'C'
    return np.ascontiguousarray(q)


def _strides(q):
    return (q.strides[0] // q.itemsize, q.strides[1] // q.itemsize)


def alpha_of(key, kind, turn):
    if kind == 'exact':
        return ([1.0, -0.5, complex(1, -2)] if key in 'cz' else [1.0, -0.5])[turn % (3 if key in 'cz' else 2)]
    return complex(0.3, -0.7) if key in 'cz' else 0.3


# ---------------------------------------------------------------------------------------------------- references
def _parts(w, dtype):
    return (w.real.astype(dtype), w.imag.astype(dtype)) if np.iscomplexobj(w) else (w.astype(dtype), None)


def reference(x, q, out0, alpha, dtype):
    """[(component, S)] of beta Out0 + (alpha q)^T x for the (k, n) values x, the (k, m) coefficients q and the (m, n)
    start values out0 (or None): the real components and the sums of the absolute values of their products in `dtype`."""
    a0, a1 = dtype(np.real(alpha)), dtype(np.imag(alpha))
    xr, xi = _parts(x, dtype)
    qr, qi = _parts(q, dtype)
    if xi is None:
        c = a0 * qr
        out = [[c.T @ xr, np.abs(c).T @ np.abs(xr)]]
    else:
        cr, ci = a0 * qr - a1 * qi, a0 * qi + a1 * qr
        Cr, Ci = np.abs(a0 * qr) + np.abs(a1 * qi), np.abs(a0 * qi) + np.abs(a1 * qr)
        axr, axi = np.abs(xr), np.abs(xi)
        out = [[cr.T @ xr - ci.T @ xi, Cr.T @ axr + Ci.T @ axi], [cr.T @ xi + ci.T @ xr, Cr.T @ axi + Ci.T @ axr]]
    if out0 is not None:
        for comp, o in zip(out, _parts(out0, dtype)):
            comp[0] = comp[0] + o
            comp[1] = comp[1] + np.abs(o)
    return out


def verify(key, got, x, q, out0, alpha, kind, tag, family):
    """`got` (m, n) against the reference: bit for bit on exact data, the rounding bound otherwise."""
    comps = [got.real, got.imag] if NC[key] == 2 else [got]
    if kind == 'exact':
        for c, (g, s) in zip(comps, reference(x, q, out0, alpha, np.float64)):
            assert s.size == 0 or 2 * s.max() < (2.0 ** 24 if key in 'sc' else 2.0 ** 52), 'the data is not exact ' + tag
            want = np.ascontiguousarray((g + 0.0).astype(REAL[key]))
            have = np.ascontiguousarray(c)
            if not same_bytes(have, want):
                bad = np.argwhere(~(have == want))
                at = tuple(bad[0]) if len(bad) else (0, 0)
                raise AssertionError('%d elements differ from the exact result, first (column, row) = %s: %r for %r %s'
                                     % (len(bad), at, have[at], want[at], tag))
        _reached(key, family)
        return
    assert np.finfo(LD).nmant >= 63, 'numpy.longdouble is no wider than float64 here'
    u = unit_roundoff(key)
    L = x.shape[0] * NC[key] + (1 if out0 is not None else 0)
    worst = 0.0
    for c, (g, s) in zip(comps, reference(x, q, out0, alpha, LD)):
        err = np.abs(c.astype(LD) - g)
        bound = (L + 4) * LD(u) * s
        bad = ~(err <= bound)                                          # (a NaN fails too)
        if bad.any():
            j, i = np.argwhere(bad)[0]
            raise AssertionError('(column %d, row %d): error %.3e above the bound %.3e %s' % (j, i, err[j, i], bound[j, i], tag))
        pos = bound > 0
        if pos.any():
            worst = max(worst, float((err[pos] / bound[pos]).max()))
    _reached(key, family, worst)


# ---------------------------------------------------------------------------------------------------- one request
def _tag(key, n, ks, ms, beta, align, kind, form, layout, col):
    env = ' '.join('%s=%s' % (k[11:], v) for k, v in sorted(os.environ.items()) if k.startswith('RLH_UPDATE_'))
    return '[update %s %s n=%d k=%s m=%s beta=%d %s %s q:%s column %d %s]' % (form, key, n, ks, ms, beta, align, kind, layout, col, env)


def update(key, n, ks, ms, beta=0, align='aligned', kind='exact', form='one', layout='C', col=1, turn=None, check=True):
    """One request, made twice: form 'one' (rlh_block_update, ks = (k,), ms = (m,)), 'two' (rlh_block_update2,
    ks = (k1, k2)) or '2x2' (rlh_block_update2x2, ms = (ma, mb)).  Returns the result windows stacked, (sum ms, n)."""
    L = _lib()
    lib, code = L.lib(), L.dtype_code(DT[key])
    ks, ms = tuple(ks), tuple(ms)
    assert len(ks) == (1 if form == 'one' else 2) and len(ms) == (2 if form == '2x2' else 1)
    m = sum(ms)
    tag = _tag(key, n, ks, ms, beta, align, kind, form, layout, col)
    aligned = ALIGNMENTS[align]
    alpha = 1.0 if form == '2x2' else alpha_of(key, kind, n + sum(ks) + m if turn is None else turn)
    xs = [Operand(key, n, k, aligned[i], i, values(key, kind, k, n, i), col) for i, k in enumerate(ks)]
    outs = [Operand(key, n, mi, aligned[2], 2 + i, values(key, kind, mi, n, 2 + i) if beta else None, col)
            for i, mi in enumerate(ms)]
    qs = [coefficients(key, kind, k, m, layout, 4 + i) for i, k in enumerate(ks)]
    a = np.array([np.real(alpha), np.imag(alpha)], dtype=np.float64)
    X = [(x.ptr(), x.ld) for x in xs]
    Q = [(L.host_ptr(q),) + _strides(q) for q in qs]
    O = [(o.ptr(), o.ld) for o in outs]

    def call():
        if form == 'one':
            L.check(lib.rlh_block_update(code, n, ks[0], *X[0], m, *O[0], *Q[0], L.host_ptr(a), beta))
        elif form == 'two':
            L.check(lib.rlh_block_update2(code, n, ks[0], *X[0], *Q[0], ks[1], *X[1], *Q[1], m, *O[0], L.host_ptr(a), beta))
        else:
            L.check(lib.rlh_block_update2x2(code, n, ks[0], *X[0], *Q[0], ks[1], *X[1], *Q[1], ms[0], *O[0], ms[1], *O[1]))
        return np.concatenate([o.result(tag) for o in outs], axis=0)

    got = call()
    for o in outs:
        o.upload()
    again = call()
    assert same_bytes(again, got), 'a repeated call gives other bits ' + tag
    for x in xs:
        x.unchanged(tag)
    if check:
        family = route(key, n, ks[0], ks[1] if len(ks) > 1 else 0, ms if form == '2x2' else m, align, form, beta)
        xw = np.concatenate([x.window() for x in xs], axis=0)
        qw = np.concatenate(qs, axis=0)
        out0 = np.concatenate([o.window() for o in outs], axis=0) if beta else None
        verify(key, got, xw, qw, out0, alpha, kind, tag, family)
    return got


class Turn:
    """Bound data sets in turn, where the reference is affordable."""
    KINDS = ['gauss', 'scaled']

    def __init__(self):
        self.turn = 0

    def run(self, key, n, ks, ms, beta, align, form, small=None, **kw):
        """Exact data always; bound data under the cap, and at the row count `small` whatever the shape costs."""
        update(key, n, ks, ms, beta, align, 'exact', form, **kw)
        if n * sum(ks) * sum(ms) <= BOUND_CAP[key] or n == small:
            update(key, n, ks, ms, beta, align, self.KINDS[self.turn % 2], form, **kw)
            self.turn += 1


def single_cases(key, align='aligned', valu=False, rows=None):
    """(n, (k, m)) of rlh_block_update under the present environment; `rows` restricts the row counts."""
    out = pairings(key, shapes(key), shape_rows(key, valu), align)
    return [c for c in out if rows is None or c[0] in rows]


def single(key, align='aligned', valu=False, rows=None):
    """rlh_block_update: every row count of a kernel with a shape of each of its families, every shape with three row
    counts, both beta.  `valu`: the leg sends every request to the VALU kernel."""
    t = Turn()
    for n, (k, m) in single_cases(key, align, valu, rows):
        for beta in (0, 1):
            t.run(key, n, (k,), (m,), beta, align, 'one', small=shape_rows(key, valu)[0])


def two_sources(key, align='aligned', valu=False):
    """rlh_block_update2: every (k1, k2) with two widths and three row counts, every row count of a kernel with a
    request of each of its families, both beta."""
    t = Turn()
    w = TWO_SOURCE_WIDTHS
    requests = [(ks, m) for i, ks in enumerate(TWO_SOURCES) for m in (w[i % len(w)], w[(i + 4) % len(w)])]
    for n, (ks, m) in pairings(key, requests, shape_rows(key, valu), align, 'two'):
        for beta in (0, 1):
            t.run(key, n, ks, (m,), beta, align, 'two', small=shape_rows(key, valu)[0])


def two_results(key, align='aligned', valu=False):
    """rlh_block_update2x2: two result blocks of different ld; on exact data also the bits of rlh_block_update2 into one
    block of ma + mb columns."""
    t = Turn()
    requests = [(ks, ms) for i, ms in enumerate(TWO_RESULTS) for ks in (TWO_RESULT_SOURCES[i % 6], TWO_RESULT_SOURCES[(i + 2) % 6])]
    for n, (ks, ms) in pairings(key, requests, shape_rows(key, valu), align, '2x2'):
        t.run(key, n, ks, ms, 0, align, '2x2', small=shape_rows(key, valu)[0])
    n = shape_rows(key, valu)[2]
    for ks, ms in requests:
        one = update(key, n, ks, (sum(ms),), 0, align, 'exact', 'two', turn=0)
        assert same_bytes(one, update(key, n, ks, ms, 0, align, 'exact', '2x2')), \
            'two result blocks differ from one block of %d columns %s' % (sum(ms), key)


def two_results_beyond_the_lds():
    """complex128, k1 = k2 = 64: (64, 64) takes two matrix-core passes; (96, 32) exceeds the LDS even alone and takes one
    pass of the VALU kernel."""
    for ms in ((64, 64), (96, 32)):
        got = update('z', 4099, (64, 64), ms, 0, 'aligned', 'exact', '2x2')
        assert same_bytes(got, update('z', 4099, (64, 64), (128,), 0, 'aligned', 'exact', 'two', turn=0))


def layouts_and_windows(key, align='aligned'):
    """F-ordered and windowed host coefficients; operands that are windows further inside wider blocks."""
    t = Turn()
    km = [(9, 9), (33, 31), (129, 17), (3, 7)] if key in 'sd' else [(17, 17), (33, 31), (129, 17), (3, 7)]
    for layout, col in (('F', 1), ('window', 1), ('C', WINDOW_COLUMNS[0]), ('F', WINDOW_COLUMNS[1])):
        for k, m in km:
            for n in (shape_rows(key)[0], 4099):
                t.run(key, n, (k,), (m,), 1, align, 'one', layout=layout, col=col)
        t.run(key, 4099, (17, 15), (33,), 0, align, 'two', layout=layout, col=col)
        t.run(key, 4099, (5, 3), (9,), 1, align, 'two', layout=layout, col=col)
        t.run(key, 4099, (16, 16), (17, 33), 0, align, '2x2', layout=layout, col=col)


def chunked(key, rows=(4099, 65)):
    """k beyond one staging slot (exact only): 1024 rows of Q per launch, or fewer for a wide result (float64, m = 1100:
    panels of 64 columns, 112 rows per launch)."""
    for n in rows:
        for beta in (0, 1):
            for k in (1025, 2049):
                update(key, n, (k,), (9,), beta)
            if key == 'd':
                assert chunk_rows('d', 1100) < 117
                for k in (117, 233):
                    update(key, n, (k,), (1100,), beta)


def deep_complex(key, cu, cap):
    """The grid-stride loop of the complex kernel (exact only): every wave of the G workgroups launched takes a third,
    ragged sweep at k = m = 16.  G = CU count x min(cap, 160 KB / LDS bytes), cap 2 or RLH_UPDATE_MFMA_WG."""
    lds = 1 * 4 * 64 * ES[key]
    G = cu * min(cap, LDS_MFMA // lds)
    n = MFMA_TILE * (4 * G * 2 + 2 * G + 1) + 5
    for beta in (0, 1):
        update(key, n, (16,), (16,), beta)


def nt_threshold(key):
    """The default route taking the non-temporal instantiation with nothing forced (exact): k = m = 16, beta = 1."""
    assert key in 'sd' and 'RLH_UPDATE_NT' not in os.environ
    n = NT_BYTES // ((16 + 2 * 16) * ES[key]) + 1 + 5 * TR[key] + 1
    assert n * (16 + 2 * 16) * ES[key] > NT_BYTES
    update(key, n, (16,), (16,), 1)


NT_CASES = {'sd': [(65, (9,), (9,), 'one'), (4099, (33,), (31,), 'one'), (1025, (127,), (47,), 'one'), (4099, (129,), (33,), 'one'),
                   (4099, (17, 15), (33,), 'two'), (2049, (16, 16), (17, 33), '2x2'), (513, (3,), (7,), 'one')],
            'cz': [(65, (17,), (17,), 'one'), (4099, (33,), (31,), 'one'), (1025, (9,), (9,), 'one'), (4099, (129,), (16,), 'one'),
                   (4099, (17, 15), (33,), 'two'), (2049, (16, 16), (17, 33), '2x2')]}


def nt_equals_default(key, setenv, delenv):
    """On bound data the RLH_UPDATE_NT=1 result of a call equals the default result bit for bit."""
    for n, ks, ms, form in NT_CASES['sd' if key in 'sd' else 'cz']:
        for beta in ((0,) if form == '2x2' else (0, 1)):
            check = n * sum(ks) * sum(ms) <= BOUND_CAP[key]
            delenv('RLH_UPDATE_NT', raising=False)
            plain = update(key, n, ks, ms, beta, 'aligned', 'gauss', form, check=check)
            setenv('RLH_UPDATE_NT', '1')
            hinted = update(key, n, ks, ms, beta, 'aligned', 'gauss', form, check=check)
            assert same_bytes(hinted, plain), 'RLH_UPDATE_NT=1 changes the bits %s n=%d k=%s m=%s %s' % (key, n, ks, ms, form)
    delenv('RLH_UPDATE_NT', raising=False)


def family_requests(key):
    """(environment, ks, m, alignment, kernel family): one request for every kernel family that launch_update can
    produce for the type."""
    out = []
    rv = RVMAX[key]
    if key in 'sd':
        for nt in ('', ' NT'):
            env = {'RLH_UPDATE_NT': '1'} if nt else {}
            out += [(env, (k,), 16, 'aligned', 'stream KS%d%s' % (ks, nt)) for k, ks in ((16, 8), (64, 16), (128, 32))]
            out += [(dict(env, RLH_UPDATE_STREAM='0'), (9,), m, 'aligned', 'valu JT%d RV%d%s' % (jt, rv, nt))
                    for m, jt in ((8, 8), (16, 16), (17, 32))]
        widths = [(8, 8), (16, 16), (33, 32 if key == 's' else 64)] + ([(17, 32)] if key == 'd' else [])
        if key == 'd':
            out.append(({'RLH_UPDATE_STREAM': '0'}, (9,), 65, 'aligned', 'valu JT64 RV1'))
    else:
        out += [({}, (k,), 16, 'aligned', 'mfma KS%d' % ks) for k, ks in ((16, 8), (64, 16), (128, 32))]
        out += [({}, (k,), 17, 'mixed', 'mfma KS%d unaligned results' % ks) for k, ks in ((16, 8), (64, 16), (128, 32))]
        widths = [(8, 8), (17, 16)]
        for nt in (('', ' NT') if rv > 1 else ('',)):
            env = dict({'RLH_UPDATE_NT': '1'} if nt else {}, RLH_UPDATE_MFMA='0')
            out += [(env, (17,), m, 'aligned', 'valu JT%d RV%d%s' % (jt, rv, nt)) for m, jt in widths]
    out += [({}, (9,), m, 'unaligned', 'valu JT%d RV1' % jt) for m, jt in widths]
    return out


def every_family(key, setenv, delenv, switches):
    """One request for every kernel family of the type: route(), the model of the dispatch, must name the family under
    the request's environment, and the request must pass (what the library itself launched is not observed)."""
    t = Turn()
    for env, ks, m, align, family in family_requests(key):
        for name in switches:
            delenv('RLH_UPDATE_' + name, raising=False)
        for name, value in env.items():
            setenv(name, value)
        assert route(key, 4099, ks[0], 0, m, align, 'one') == family, (key, env, ks, m, align, family)
        for beta in (0, 1):
            t.run(key, 4099, ks, (m,), beta, align, 'one')
    for name in switches:
        delenv('RLH_UPDATE_' + name, raising=False)


# ---------------------------------------------------------------------------------------------------- degenerate
def degenerate(key):
    L = _lib()
    lib, code = L.lib(), L.dtype_code(DT[key])
    a = np.array([0.3, 0.0])
    for aligned in (True, False):
        # n = 0 and m = 0: nothing may be touched
        x, o = operands(key, 5, 3, aligned, 2)
        q = np.ones((3, 3), dtype=DT[key])
        for n, m in ((0, 3), (5, 0), (0, 0)):
            for beta in (0, 1):
                L.check(lib.rlh_block_update(code, n, 3, x.ptr(), x.ld, m, o.ptr(), o.ld, L.host_ptr(q), 3, 1, L.host_ptr(a), beta))
                L.check(lib.rlh_block_update2(code, n, 3, x.ptr(), x.ld, L.host_ptr(q), 3, 1, 3, x.ptr(), x.ld, L.host_ptr(q), 3, 1,
                                              m, o.ptr(), o.ld, L.host_ptr(a), beta))
        L.check(lib.rlh_block_update2x2(code, 0, 3, x.ptr(), x.ld, L.host_ptr(q), 3, 1, 3, x.ptr(), x.ld, L.host_ptr(q), 3, 1,
                                        1, o.ptr(), o.ld, 2, o.ptr(2), o.ld))
        x.check_unchanged('by an empty request')
        o.check_unchanged('by an empty request')
        # k = 0: beta = 0 makes the window +0 bits (padding rows and guard columns untouched), beta = 1 leaves it alone
        align = 'aligned' if aligned else 'unaligned'
        for n, m in ((1, 1), (65, 9), (4099, 17)):
            got = update(key, n, (0,), (m,), 0, align, 'exact', check=False)
            assert same_bytes(got, np.zeros((m, n), dtype=DT[key])), 'k = 0, beta = 0 does not give +0 %s' % key
            out = Operand(key, n, m, aligned, 2, values(key, 'gauss', m, n, 2))
            L.check(lib.rlh_block_update(code, n, 0, None, n, m, out.ptr(), out.ld, None, m, 1, L.host_ptr(a), 1))
            out.unchanged('by k = 0, beta = 1')


def refusals():
    """Each refusal returns non-zero with its message and leaves every operand bit-identical; the library works afterwards."""
    import pytest
    L = _lib()
    lib = L.lib()
    a = np.array([1.0, 0.0])
    ap = L.host_ptr(a)
    n = 5
    blk, out, out2 = operands('d', n, 6, True, 3)          # sources: columns of blk
    q = np.ones((4, 6))
    qp = L.host_ptr(q)
    p, ld = blk.ptr(), blk.ld

    def refused(message, fn, *args):
        with pytest.raises(L.RlhError, match=message):
            L.check(fn(*args))
        for b in (blk, out, out2):
            b.check_unchanged('by a refused call')

    one, two, x22 = lib.rlh_block_update, lib.rlh_block_update2, lib.rlh_block_update2x2
    refused('rlh_block_update: beta must be 0 or 1', one, 1, n, 2, p, ld, 3, out.ptr(), out.ld, qp, 6, 1, ap, 2)
    refused('rlh_block_update2: beta must be 0 or 1', two, 1, n, 2, p, ld, qp, 6, 1, 2, blk.ptr(3), ld, qp, 6, 1, 3, out.ptr(), out.ld, ap, 2)
    refused('rlh_block_update: leading dimension smaller than n', one, 1, n, 2, p, n - 1, 3, out.ptr(), out.ld, qp, 6, 1, ap, 0)
    refused('rlh_block_update: leading dimension smaller than n', one, 1, n, 2, p, ld, 3, out.ptr(), n - 1, qp, 6, 1, ap, 0)
    refused('rlh_block_update2: leading dimension smaller than n', two, 1, n, 2, p, ld, qp, 6, 1, 2, blk.ptr(3), n - 1, qp, 6, 1, 3,
            out.ptr(), out.ld, ap, 0)
    refused('rlh_block_update2x2: leading dimension smaller than n', x22, 1, n, 2, p, ld, qp, 6, 1, 2, blk.ptr(3), ld, qp, 6, 1, 3,
            out.ptr(), out.ld, 3, out2.ptr(), n - 1)
    # the result one column after the first source column in the same block
    refused('rlh_block_update: output window overlaps the input window', one, 1, n, 2, p, ld, 3, blk.ptr(2), ld, qp, 6, 1, ap, 0)
    refused('rlh_block_update2: output window overlaps an input window', two, 1, n, 2, out.ptr(), out.ld, qp, 6, 1, 2, p, ld, qp, 6, 1,
            3, blk.ptr(2), ld, ap, 1)
    refused('rlh_block_update2x2: an output window overlaps an input window or the other output', x22, 1, n, 2, p, ld, qp, 6, 1, 2,
            blk.ptr(3), ld, qp, 6, 1, 3, out.ptr(), out.ld, 3, out.ptr(3), out.ld)
    # float64, m = 64: 2048 padded rows of coefficients fill the staging slot, one more row does not fit
    k1 = SLOT // (64 * 8) - 4
    wide, = operands('d', 1, k1, True, 1)
    res, = operands('d', 1, 64, True, 1)
    big = np.zeros((k1, 64))
    args = (1, 1, k1, wide.ptr(), wide.ld, L.host_ptr(big), 64, 1)
    L.check(two(*args, 4, p, ld, L.host_ptr(big), 64, 1, 64, res.ptr(), res.ld, ap, 1))
    res.check_unchanged('by an update with zero coefficients')
    refused('rlh_block_update2: coefficient blocks of %d bytes exceed the staging slot' % (SLOT + 4 * 64 * 8), two, *args,
            5, p, ld, L.host_ptr(big), 64, 1, 64, res.ptr(), res.ld, ap, 1)
    res.check_unchanged('by a refused call')
    wide.check_unchanged('by a refused call')
    # float64, m = 32769: fewer than 4 rows of coefficients fit
    m = 32769
    huge, = operands('d', 1, m, True, 1)
    qrow = np.zeros((1, m))
    refused('rlh_block_update: %d output vectors exceed the staging slot' % m, one, 1, 1, 1, p, ld, m, huge.ptr(), huge.ld,
            L.host_ptr(qrow), m, 1, ap, 0)
    huge.check_unchanged('by a refused call')
    update('d', 65, (9,), (9,), 1)


# ---------------------------------------------------------------------------------------------------- child leg
# RLH_UPDATE_RV is read once per process (a function-local static of launch_update), so the one-row-per-lane kernel on
# aligned blocks runs in a child process: tests/_block_update_child.py <leg>, with the leg's variables in its environment.
def _leg_rv0(cu, rows=None):
    for key in ('s', 'd', 'c'):
        single(key, 'aligned', valu=True, rows=rows)    # (two sources and two results on RV = 1: the unaligned legs, same kernel)
    assert all('RV1' in family for _, family in RATIOS), 'a case left the one-row-per-lane kernel: %s' % sorted(RATIOS)


LEGS = {'rv0': ({'RLH_UPDATE_STREAM': '0', 'RLH_UPDATE_MFMA': '0', 'RLH_UPDATE_RV': '0'}, _leg_rv0)}


def run_child(leg, cu, timeout=600, fake=False, env_override=None, rows=None):
    """Starts tests/_block_update_child.py for one leg as a fresh process (its own time limit, never retried) and returns
    the completed process.  `rows` restricts the leg to those row counts (the CPU tier checks the runner, not the leg)."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if not k.startswith('RLH_UPDATE_')}
    env.update(LEGS[leg][0])
    env.update(env_override or {})
    here = os.path.dirname(os.path.abspath(__file__))
    cmd = [sys.executable, os.path.join(here, '_block_update_child.py'), leg, '--cu', str(cu)] + (['--fake'] if fake else [])
    if rows:
        cmd += ['--rows', ','.join(str(n) for n in rows)]
    return subprocess.run(cmd, env=env, timeout=timeout, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
