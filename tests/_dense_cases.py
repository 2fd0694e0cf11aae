"""The dense operator behind rlh_dense_apply / rlh_dense_apply_r1, element by element, shared by the CPU tier
(tests/fake_lib.py: shows that NumPy in the working precision meets every bound below and that every exact case is exact)
and the GPU tier (librlhip.so, every kernel family that dense_impl of raleigh_amd/csrc/dense.hip reaches), through the
raw C ABI.

Harness.  A is an Operand of R lines of lda elements, `length` of them valid (R x length is A as stored: the lines are
the rows of a row-major A, the columns of a column-major one); the elements past `length`, the guard lines before and
after and, for a window of a wider parent, everything left of the window hold NaN.  X and Y are Operands of m + 2 columns;
the call sees the window from column 1 (X: NaN outside its window; Y: NaN inside its window alone, finite values that
differ from position to position in its guard columns and padding rows, so that a NaN stored there is seen as well).  Whatever a kernel reads past an operand's extent must never reach a stored
element (the matrix-core kernels load whole 16-byte pieces and select zero for what lies past the K range; rows and
vectors past the extent are computed and never stored): a NaN in the result is a failure.  Y holds NaN inside its window
before the call and must come back finite; its guard columns and padding rows must be the uploaded bytes; A, X, u and c
must come back bit-identical.  Every call is made twice, the second time on a re-uploaded Y, and must give the same bits.

Alignment legs (ALIGNMENTS): 'aligned'; 'unaligned' (no operand 16-byte aligned: dense_valu_kernel, for float32 the only
way to it); 'y_unaligned' (only Y shifted, ldy odd: stays on the matrix cores); 'tight' (lda == length, ldx == nx: the
re-read at 0 of a piece past the line happens for the last piece of the last K step, where a padded lda reads padding);
'window' (A is a window at element j0 = 16 of lines of j0 + roundup(length) elements -- the call of
raleigh_amd/algebra/hip/dist.py, which passes data_ptr() + j0 * es with the parent's lda), 'window_rows' (further guard
lines) and 'window_odd' (j0 = 17: breaks the 16-byte alignment of every type but complex128).

Two kinds of input.
  * Rounding bound on full-mantissa data (Gaussian; Gaussian with line j scaled by 2^(-3 (j mod 12))).  The reference is
    formed from the uploaded values in numpy.longdouble (64-bit mantissa, asserted), real and imaginary parts separately.
    Every real component of every result element is held to
        |got - ref| <= (L + 4) u S,
    u the unit roundoff of the real type, L the number of real products summed into the component (nx real, 2 nx
    complex, plus 1 (real) or 2 (complex) with a rank-one term) and S the sum of the absolute values of those products
    in the reference precision, |u_i c_v| included.  L terms summed in ANY order cost at most L u S, with or without
    fused operations and across K splits; the 4 covers the epilogue's product, the final rounding and the second-order
    terms for L u < 0.01 (asserted per case).  Derived, never measured.  ny nx m of these cases is capped: BOUND_CAP.
  * Exact data: integers uniform in [-2, 2] (s, c) or [-2^14, 2^14] (d, z) in A, X, u and c.  Every partial sum in any
    order is an integer below 2^23 / 2^51 (asserted on the reference's S, per case), hence exact, and the result must
    equal a float64 / complex128 BLAS reference BIT FOR BIT (normalised to +0) on every leg, kernel and split count.
    This is what catches a dropped, doubled or misplaced K step, split, row, tile or vector however large the case; all
    large cases (16 splits, the workspace cap, many row tiles) are exact-only.

Shapes.  NY / M / NX lists per kernel (float: 128 x 32 | 64 | 128 tiles of 32 x 32 MFMA tiles; dense_mfma16_kernel:
64 x 64 | 128 tiles of 16 x 16; VALU: 64 x 64 tiles, 4 x 4 per thread); pairings() groups the vector counts by the kernel
family that route() names under the leg's environment and gives every K of the list to every (order, transp) form of
every family, the row counts, vector counts and epilogue forms of the family in turn.  Never the full product.

route() restates dense_impl and the split computation of launch_mfma / launch_mfma2 / launch_mfma16 (kchunk rounding and
recomputed split count included).  It names the kernel family and the split count that a case reaches, for the table that
every test prints, for the pairing of shapes with families and for the CPU tier's coverage assertion; it never changes
what a case checks.
"""

import os

import numpy as np

from _columnwise_cases import DT, KEYS, Block, base_shift, leading_dimension, operands, same_bytes, unit_roundoff
from _gram_cases import LD, NC, REAL, values

ES = {'s': 4, 'd': 8, 'c': 8, 'z': 16}
EPU = {key: 16 // es for key, es in ES.items()}       # elements of a 16-byte unit
WORKSPACE = 96 << 20                    # kWorkspaceBytes (common.h): the split-K partial tiles
MAX_SPLITS, SPLIT_K = 16, 512           # launch_*: at most 16 splits of at least 512 k
SWITCHES = ('KERNEL', 'BK', 'MR', 'D_TILE', 'VALU', 'WG_PER_CU')

# ---------------------------------------------------------------------------------------------------- shapes
# float kernels: a tile of MR = 128 rows x BN = 32 | 64 | 128 vectors, waves of 32 or 64 rows, MFMA tiles 32 x 32, vectors
# in groups of 4
NY_F = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257]
M_F = [1, 3, 4, 5, 8, 9, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 257]
# dense_mfma16_kernel: 64 rows x 64 vectors (128 for double with m > 64), 2 x 2 waves, tiles of 16
NY_16 = [1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129]
M_16 = NY_16
# K: one to five K steps of either BK, both parities of the double buffer, the paired loop of the DEEP pipeline with its
# break; 36 (with lda == 36 on the tight leg: the re-read at 0); one, two and three splits
NX = [0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 95, 96, 97, 36, 511, 512, 513, 545, 1024, 1025]
NX_SPLIT = [511, 512, 513, 545, 1024, 1025, 7680, 7681]      # ... 15 and 16 splits, the last one of one element (float)
# VALU kernel: 64 x 64 tile, BK 16, 4 x 4 per thread
NY_V = [1, 3, 4, 5, 63, 64, 65, 129]
M_V = NY_V
NX_V = [0, 1, 15, 16, 17, 33]
# the tight leg: lda == length and ldx == nx, multiples of four elements (a 16-byte unit of every type)
NY_T = [4, 32, 36, 64, 68, 128, 132, 256, 260]
NX_T = [4, 16, 32, 36, 48, 64, 68, 96, 100, 512, 516, 1028]
FORMS = [(0, 0), (0, 1), (1, 0), (1, 1)]                     # (order, transp): for complex the four A_KC x CONJ
EPILOGUES = ['none', 'c', 'uc']                              # no rank-one term; c alone (u: a vector of ones); u and c
# ny nx m of a bound case: the longdouble reference of one test function (a few hundred cases, most of them far below
# the cap) stays within a few seconds on the CPU
BOUND_CAP = {'s': 500000, 'd': 500000, 'c': 150000, 'z': 150000}
ALIGNMENTS = ('aligned', 'unaligned', 'y_unaligned', 'tight', 'window', 'window_rows', 'window_odd')
WINDOW_J0, WINDOW_ODD_J0, WINDOW_R0 = 16, 17, 3


# ---------------------------------------------------------------------------------------------------- layout
def _up(n, unit):
    return (n + unit - 1) // unit * unit


def layout(key, ny, nx, m, order, transp, alignment):
    """Where the three operands of a request lie: leading dimensions, base shifts, the window of A."""
    assert alignment in ALIGNMENTS
    dt, epu = np.dtype(DT[key]), EPU[key]
    kc = (order == 0) != (transp == 1)
    length, R = (nx, ny) if kc else (ny, nx)
    lda, ldx, ldy = (leading_dimension(max(n, 1), dt, True, w) for w, n in enumerate((length, nx, ny)))
    sa = sx = sy = 0
    r0, j0 = 1, 0
    if alignment == 'unaligned':
        lda, ldx, ldy = (leading_dimension(max(n, 1), dt, False, w) for w, n in enumerate((length, nx, ny)))
        sa = sx = sy = base_shift(dt, False)
    elif alignment == 'y_unaligned':
        ldy = (ny + 3) | 1
        sy = base_shift(dt, False)
    elif alignment == 'tight':
        lda, ldx = max(length, 1), max(nx, 1)
    elif alignment == 'window':
        j0 = WINDOW_J0
        lda = j0 + _up(max(length, 1), epu)
    elif alignment == 'window_rows':
        r0 = WINDOW_R0
    elif alignment == 'window_odd':
        j0 = WINDOW_ODD_J0
        lda = leading_dimension(j0 + max(length, 1), dt, True, 0)
    return dict(kc=kc, length=length, R=R, lda=lda, ldx=ldx, ldy=ldy, sa=sa, sx=sx, sy=sy, r0=r0, j0=j0)


# ---------------------------------------------------------------------------------------------------- dispatch model
def _env(name, default):
    v = os.environ.get('RLH_DENSE_' + name)
    return default if v is None or v == '' else int(v)


def split_plan(ny, nx, m, MR, BN, es, unit, cu, target=None):
    """(splits wanted before the workspace cap, splits taken) of launch_mfma / launch_mfma2 / launch_mfma16."""
    bx, by = (ny + MR - 1) // MR, (m + BN - 1) // BN
    target = _env('WG_PER_CU', 8) if target is None else target
    splits = (cu * target + bx * by - 1) // (bx * by)
    splits = min(splits, (nx + SPLIT_K - 1) // SPLIT_K, MAX_SPLITS)
    wanted = max(splits, 1)
    while splits > 1 and splits * m * ny * es > WORKSPACE:
        splits -= 1
    splits = max(splits, 1)
    kchunk = _up((nx + splits - 1) // splits, unit)
    splits = (nx + kchunk - 1) // kchunk
    return wanted, max(splits, 1)


def plan(key, ny, nx, m, order, transp, alignment, cu, target=None):
    """(kernel family, splits wanted, splits taken) under the present environment."""
    lay = layout(key, ny, nx, m, order, transp, alignment)
    es, epu = ES[key], EPU[key]
    ok = ((lay['sa'] + (lay['r0'] * lay['lda'] + lay['j0']) * es) % 16 == 0 and (lay['sx'] + lay['ldx'] * es) % 16 == 0
          and lay['lda'] % epu == 0 and lay['ldx'] % epu == 0 and lay['lda'] >= epu and lay['ldx'] >= epu and nx > 0)
    tiles = 'KC' if lay['kc'] else 'CM'
    conj = ' conj' if transp == 1 and key in 'cz' else ''
    if key == 's' and ok:
        bn = 128 if m > 64 else (64 if m > 32 else 32)
        if _env('KERNEL', 1 if lay['kc'] else 2) == 2:
            bk = 32 if _env('BK', 16 if lay['kc'] else 32) == 32 else 16
            return ('mfma2 BN%d BK%d %s' % (bn, bk, tiles),) + split_plan(ny, nx, m, 128, bn, 4, 32, cu, target)
        mr = 64 if m > 64 and _env('MR', 128) == 64 else 128
        return ('mfma1 %sBN%d %s' % ('MR64 ' if mr == 64 else '', bn, tiles),) + split_plan(ny, nx, m, mr, bn, 4, 32, cu, target)
    if key != 's' and ok and not _env('VALU', 0):
        tv = 4 if key == 'd' and _env('D_TILE', 24) == 24 and m > 64 else 2
        return ('mfma16 2x%d %s%s' % (tv, tiles, conj),) + split_plan(ny, nx, m, 64, 32 * tv, es, 16, cu, target)
    return 'valu' + conj, 1, 1


def route(key, ny, nx, m, order, transp, alignment, cu):
    """The kernel family and the split count that the request reaches under the present environment."""
    family, _, splits = plan(key, ny, nx, m, order, transp, alignment, cu)
    return family if family.startswith('valu') else '%s x%d' % (family, splits)


def table_family(name):
    """The row of the table for a name of route(): the family, direct tile store or split-K reduction."""
    if ' x' not in name:
        return name
    family, splits = name.rsplit(' x', 1)
    return family + (' split' if int(splits) > 1 else '')


RATIOS = {}          # (type, kernel family) -> [bound cases, largest error / bound seen, exact cases]


def ratios_text():
    lines = ['%-2s %-32s %6s %6s  %s' % ('', 'kernel family', 'bound', 'exact', 'largest error / bound')]
    for (key, family), (count, ratio, exact) in sorted(RATIOS.items()):
        lines.append('%-2s %-32s %6d %6d  %s' % (key, family, count, exact, '%.3f' % ratio if count else '-'))
    return '\n'.join(lines)


def _reached(key, family, ratio=None):
    r = RATIOS.setdefault((key, table_family(family)), [0, 0.0, 0])
    if ratio is None:
        r[2] += 1
    else:
        r[0] += 1
        r[1] = max(r[1], ratio)


# ---------------------------------------------------------------------------------------------------- harness
def _lib():
    from raleigh_amd import _lib as L
    return L


def _nan(key):
    return complex(np.nan, np.nan) if NC[key] == 2 else np.nan


class Operand:
    """`R` lines of `ld` elements behind `r0` guard lines (and as many after): `vals` (R, length) in the window that starts
    at element j0 of each line, NaN everywhere else.  `result`: NaN in the window alone; the guard lines and the padding keep
    the Block's own values, which differ from position to position and are finite, so neither a NaN nor a number stored
    outside the window equals what was uploaded there."""

    def __init__(self, key, length, R, ld, shift, which, vals=None, r0=1, j0=0, result=False):
        dt = np.dtype(DT[key])
        assert ld >= j0 + length
        self.length, self.R, self.ld, self.r0, self.j0, self.es = length, R, ld, r0, j0, dt.itemsize
        self.blk = Block(dt, j0 + length, R + 2 * (r0 - 1), ld, shift, which=which)
        if result:
            self.window()[...] = _nan(key)
        else:
            self.blk.host[...] = _nan(key)
            self.window()[...] = vals
        self.blk.upload()

    def ptr(self):
        return self.blk.ptr(self.r0) + self.j0 * self.es

    def window(self):
        return self.blk.host[self.r0:self.r0 + self.R, self.j0:self.j0 + self.length]

    def upload(self):
        self.blk.upload()

    def unchanged(self, what=''):
        self.blk.check_unchanged(what)

    def result(self, what=''):
        """The downloaded window; every other byte of the block must be what was uploaded (as Block.check)."""
        got = self.blk.fetch()
        sel = (slice(self.r0, self.r0 + self.R), slice(self.j0, self.j0 + self.length))
        win = got[sel].copy()
        got[sel] = self.window()
        assert same_bytes(got, self.blk.host), 'guard columns or padding rows of the result modified ' + what
        return win


# ---------------------------------------------------------------------------------------------------- references
def _parts(w, dtype):
    return (w.real.astype(dtype), w.imag.astype(dtype)) if np.iscomplexobj(w) else (w.astype(dtype), None)


def reference(op, x, u, c, dtype):
    """[(component, S)] of x op^T - c u^T for the (ny, nx) operator op (conjugated already), the (m, nx) vectors x, u (ny)
    and c (m) or None: the real components of the (m, ny) result and the sums of the absolute values of their products."""
    ar, ai = _parts(op, dtype)
    xr, xi = _parts(x, dtype)
    if ai is None:
        out = [[xr @ ar.T, np.abs(xr) @ np.abs(ar).T]]
    else:
        Ar, Ai, Xr, Xi = np.abs(ar), np.abs(ai), np.abs(xr), np.abs(xi)
        out = [[xr @ ar.T - xi @ ai.T, Xr @ Ar.T + Xi @ Ai.T], [xr @ ai.T + xi @ ar.T, Xr @ Ai.T + Xi @ Ar.T]]
    if c is not None:
        ur, ui = _parts(u, dtype)
        cr, ci = _parts(c, dtype)
        if ui is None:
            out[0][0] = out[0][0] - np.outer(cr, ur)
            out[0][1] = out[0][1] + np.abs(np.outer(cr, ur))
        else:
            out[0][0] = out[0][0] - (np.outer(cr, ur) - np.outer(ci, ui))
            out[0][1] = out[0][1] + np.abs(np.outer(cr, ur)) + np.abs(np.outer(ci, ui))
            out[1][0] = out[1][0] - (np.outer(cr, ui) + np.outer(ci, ur))
            out[1][1] = out[1][1] + np.abs(np.outer(cr, ui)) + np.abs(np.outer(ci, ur))
    return out


def verify(key, got, op, x, u, c, kind, tag, family):
    """`got` (m, ny) against the reference: bit for bit on exact data, the rounding bound otherwise."""
    comps = [got.real, got.imag] if NC[key] == 2 else [got]
    if kind == 'exact':
        for comp, (g, s) in zip(comps, reference(op, x, u, c, np.float64)):
            assert s.size == 0 or s.max() < (2.0 ** 23 if key in 'sc' else 2.0 ** 51), 'the data is not exact ' + tag
            want = np.ascontiguousarray((g + 0.0).astype(REAL[key]))
            have = np.ascontiguousarray(comp + REAL[key](0))             # (a zero of either sign is +0 on both sides)
            if not same_bytes(have, want):
                bad = np.argwhere(~(have == want))
                at = tuple(bad[0]) if len(bad) else (0, 0)
                raise AssertionError('%d elements differ from the exact result, first (vector, row) = %s: %r for %r %s'
                                     % (len(bad), at, have[at], want[at], tag))
        _reached(key, family)
        return
    assert np.finfo(LD).nmant >= 63, 'numpy.longdouble is no wider than float64 here'
    unit = unit_roundoff(key)
    L = x.shape[1] * NC[key] + (NC[key] if c is not None else 0)
    assert L * unit < 0.01, 'the bound does not hold for so many terms ' + tag
    worst = 0.0
    for comp, (g, s) in zip(comps, reference(op, x, u, c, LD)):
        err = np.abs(comp.astype(LD) - g)
        bound = (L + 4) * LD(unit) * s
        bad = ~(err <= bound)                                          # (a NaN fails too)
        if bad.any():
            j, i = np.argwhere(bad)[0]
            raise AssertionError('(vector %d, row %d): error %.3e above the bound %.3e %s' % (j, i, err[j, i], bound[j, i], tag))
        pos = bound > 0
        if pos.any():
            worst = max(worst, float((err[pos] / bound[pos]).max()))
    _reached(key, family, worst)


# ---------------------------------------------------------------------------------------------------- one request
def _tag(key, ny, nx, m, order, transp, epi, align, kind, family):
    env = ' '.join('%s=%s' % (k[10:], v) for k, v in sorted(os.environ.items()) if k.startswith('RLH_DENSE_'))
    return '[dense %s ny=%d nx=%d m=%d order=%d transp=%d %s %s %s -> %s %s]' % (key, ny, nx, m, order, transp, epi, align, kind, family, env)


def apply(key, ny, nx, m, order=0, transp=0, epi='none', align='aligned', kind='exact', cu=4, null=False, check=True):
    """One request, made twice.  `null`: A and X are NULL (nx = 0).  Returns the result window, (m, ny)."""
    L = _lib()
    lib, code = L.lib(), L.dtype_code(DT[key])
    lay = layout(key, ny, nx, m, order, transp, align)
    family = route(key, ny, nx, m, order, transp, align, cu)
    tag = _tag(key, ny, nx, m, order, transp, epi, align, kind, family)
    a = Operand(key, lay['length'], lay['R'], lay['lda'], lay['sa'], 0, values(key, kind, lay['R'], lay['length'], 0), lay['r0'], lay['j0'])
    x = Operand(key, nx, m, lay['ldx'], lay['sx'], 1, values(key, kind, m, nx, 1))
    y = Operand(key, ny, m, lay['ldy'], lay['sy'], 2, result=True)
    u = c = None
    if epi != 'none':
        c = Operand(key, m, 1, m + 3, 0, 3, values(key, kind, 1, m, 3))
        if epi == 'uc':
            u = Operand(key, ny, 1, ny + 5, 0, 4, values(key, kind, 1, ny, 4))
    M, N = (nx, ny) if transp else (ny, nx)
    ap, xp = (None, None) if null else (a.ptr(), x.ptr())
    assert not null or nx == 0

    def call():
        if epi == 'none':
            L.check(lib.rlh_dense_apply(code, M, N, ap, lay['lda'], order, transp, m, xp, lay['ldx'], y.ptr(), lay['ldy']))
        else:
            L.check(lib.rlh_dense_apply_r1(code, M, N, ap, lay['lda'], order, transp, m, xp, lay['ldx'], y.ptr(), lay['ldy'],
                                           u.ptr() if u else None, c.ptr()))
        return y.result(tag)

    got = call()
    y.upload()
    again = call()
    assert same_bytes(again, got), 'a repeated call gives other bits ' + tag
    for o, name in ((a, 'A'), (x, 'X'), (u, 'u'), (c, 'c')):
        if o is not None:
            o.unchanged('(%s) %s' % (name, tag))
    if check:
        w = a.window()
        op = w if lay['kc'] else w.T
        if transp == 1 and NC[key] == 2:
            op = np.conj(op)
        cv = c.window()[0] if c else None
        uv = (u.window()[0] if u else np.ones(ny, dtype=DT[key])) if c else None
        verify(key, got, op, x.window(), uv, cv, kind, tag, family)
    return got


class Turn:
    """Exact data always; the bound data sets in turn where the reference is affordable."""
    KINDS = ['gauss', 'scaled']

    def __init__(self, cu):
        self.turn, self.cu = 0, cu

    def run(self, key, ny, nx, m, order, transp, epi, align):
        apply(key, ny, nx, m, order, transp, epi, align, 'exact', self.cu)
        if ny * nx * m <= BOUND_CAP[key]:
            apply(key, ny, nx, m, order, transp, epi, align, self.KINDS[self.turn % 2], self.cu)
            self.turn += 1


# ---------------------------------------------------------------------------------------------------- case lists
def lists(key, align, cu):
    """(row counts, K, vector counts) of the kernel that the leg's requests reach under the present environment."""
    if align == 'tight':
        return NY_T, NX_T, (M_F if key == 's' else M_16)
    kernel = route(key, 128, 64, 8, 0, 0, align, cu)
    if kernel.startswith('valu'):
        return NY_V, NX_V, M_V
    return (NY_F, NX, M_F) if key == 's' else (NY_16, NX, M_16)


def pairings(key, align, cu, ks=None):
    """(ny, nx, m, order, transp, epilogue) of a leg: the vector counts are grouped by the kernel family that route()
    names under the present environment (BN 32 | 64 | 128; 2x2 | 2x4), and every K of the list meets every (order,
    transp) form of every group, with the group's vector counts, the row counts and the epilogue forms in turn.  (route()
    chooses which cases run; it never changes what a case checks.)"""
    nys, nxs, ms = lists(key, align, cu)
    nxs = nxs if ks is None else ks
    out = []
    for f, (order, transp) in enumerate(FORMS):
        groups = {}
        for m in ms:
            groups.setdefault(table_family(route(key, 128, 64, m, order, transp, align, cu)), []).append(m)
        for g, members in enumerate(groups.values()):
            rounds = max(1, -(-max(len(nys), len(members)) // len(nxs)))       # short K lists go round until every row count was met
            for i in range(rounds * len(nxs)):
                out.append((nys[(i + f + g) % len(nys)], nxs[i % len(nxs)], members[(i + 2 * f) % len(members)], order, transp,
                            EPILOGUES[(i + f + i // len(nxs)) % 3]))
    return out


def sweep(key, align, cu):
    """Every pairing of the leg."""
    t = Turn(cu)
    for ny, nx, m, order, transp, epi in pairings(key, align, cu):
        t.run(key, ny, nx, m, order, transp, epi, align)


# (ny, m): one per BN / 2x2 | 2x4, ragged in both directions, and some small ones (SPLIT_SMALL gives every family bound data)
SPLIT_SHAPES = {'s': [(129, 33), (257, 65), (65, 129), (17, 8), (5, 3), (3, 33), (2, 65)],
                'd': [(65, 33), (129, 65), (33, 129), (17, 8), (5, 3), (2, 65)],
                'c': [(65, 33), (129, 65), (33, 17), (17, 8), (5, 3)], 'z': [(65, 33), (129, 65), (33, 17), (17, 8), (5, 3)]}


SPLIT_SMALL = {'s': [(5, 3), (3, 33), (2, 65)], 'd': [(5, 3), (2, 65)], 'c': [(5, 3)], 'z': [(5, 3)]}


def split_cases(key):
    """(ny, nx, m, order, transp, epilogue): every K of NX_SPLIT with every epilogue form, the (order, transp) forms and
    the shapes of the type in turn."""
    shapes = SPLIT_SHAPES[key]
    return [(shapes[(3 * i + e) % len(shapes)] + FORMS[(i + e) % 4] + (epi, nx)) for i, nx in enumerate(NX_SPLIT)
            for e, epi in enumerate(EPILOGUES)]


def splits(key, cu, align='aligned'):
    """K splitting pinned: one, two, three, 15 and 16 splits, the last split of one element, every epilogue form through
    the reduce kernel of the type and, at the same shapes below 512, on the direct tile store."""
    t = Turn(cu)
    for ny, m, order, transp, epi, nx in split_cases(key):
        t.run(key, ny, nx, m, order, transp, epi, align)
        t.run(key, ny, 97, m, order, transp, epi, align)
    # bound data through the reduce kernel for every family that route() names: a shape of every BN / 2x2 | 2x4 under the
    # cap with every (order, transp) form at three splits, the smallest also at 16
    for i, (ny, m) in enumerate(SPLIT_SMALL[key]):
        for f, (order, transp) in enumerate(FORMS):
            assert ny * 1025 * m <= BOUND_CAP[key]
            t.run(key, ny, 1025, m, order, transp, EPILOGUES[(i + f) % 3], align)
    ny, m = SPLIT_SMALL[key][0]
    for f, (order, transp) in enumerate(FORMS):
        assert ny * 7681 * m <= BOUND_CAP[key]
        t.run(key, ny, 7681, m, order, transp, EPILOGUES[(f + 1) % 3], align)


def workspace_cap(key, cu):
    """Exact only: ny = 1024, nx = 600 and the smallest multiple of 64 vectors whose two splits exceed the workspace --
    two splits wanted, one taken.  Returns a message where the CU count makes it otherwise (nothing is run then)."""
    ny, nx = 1024, 600
    m = _up(WORKSPACE // (2 * ny * ES[key]) + 1, 64)
    assert 2 * m * ny * ES[key] > WORKSPACE >= 2 * (m - 64) * ny * ES[key]
    for order, transp in ((0, 0), (0, 1)):
        family, wanted, taken = plan(key, ny, nx, m, order, transp, 'aligned', cu)
        if family.startswith('valu') or (wanted, taken) != (2, 1):
            return '%s on %d CUs: %d splits wanted, %d taken' % (family, cu, wanted, taken)
    apply(key, ny, nx, m, 0, 0, 'uc', 'aligned', 'exact', cu)
    apply(key, ny, nx, m, 0, 1, 'c', 'aligned', 'exact', cu)
    return None


def many_row_tiles(key, cu):
    """Exact only: enough row tiles for every CU to hold more than one workgroup, ragged."""
    tile = 128 if key == 's' else 64
    ny = tile * (2 * cu + 1) + 3
    for (order, transp), m, epi in zip(FORMS, (5, 33, 65, 9), ('uc', 'none', 'c', 'uc')):
        apply(key, ny, 100 + m, m, order, transp, epi, 'aligned', 'exact', cu)


# ---------------------------------------------------------------------------------------------------- degenerate
def degenerate(key):
    L = _lib()
    lib, code = L.lib(), L.dtype_code(DT[key])
    for aligned in (True, False):
        # m = 0 and ny = 0: nothing may be touched
        a, x, y = operands(key, 5, 3, aligned, 3)
        for M, N, m, transp in ((5, 5, 0, 0), (0, 5, 3, 0), (5, 0, 3, 1), (0, 0, 0, 0)):
            L.check(lib.rlh_dense_apply(code, M, N, a.ptr(), a.ld, 0, transp, m, x.ptr(), x.ld, y.ptr(), y.ld))
            L.check(lib.rlh_dense_apply_r1(code, M, N, a.ptr(), a.ld, 0, transp, m, x.ptr(), x.ld, y.ptr(), y.ld, a.ptr(2), x.ptr(2)))
        for b in (a, x, y):
            b.check_unchanged('by an empty request')
        # nx = 0: Y is exactly +0, or exactly -u c^T; A and X may be NULL
        align = 'aligned' if aligned else 'unaligned'
        for ny, m in ((1, 1), (65, 9), (129, 65)):
            for order, transp in FORMS:
                for null in (False, True):
                    got = apply(key, ny, 0, m, order, transp, 'none', align, 'exact', null=null, check=False)
                    assert same_bytes(got, np.zeros((m, ny), dtype=DT[key])), 'nx = 0 does not give +0 %s' % key
                    for epi in ('c', 'uc'):
                        apply(key, ny, 0, m, order, transp, epi, align, 'exact', null=null)


def refusals():
    """Every RLH_REQUIRE of rlh_dense_apply_r1: each returns non-zero with its message before any launch and leaves every
    operand bit-identical; the library works afterwards."""
    import pytest
    L = _lib()
    lib, code = L.lib(), L.dtype_code(np.float64)
    M, N, m = 5, 7, 3
    a, x, y = operands('d', 8, 8, True, 3)
    ap, xp, yp, up, cp = a.ptr(), x.ptr(), y.ptr(), a.ptr(7), x.ptr(7)
    fn = lib.rlh_dense_apply_r1

    def refused(message, *args):
        with pytest.raises(L.RlhError, match=message):
            L.check(fn(*args))
        for b in (a, x, y):
            b.check_unchanged('by a refused call')

    refused('rlh_dense_apply_r1: a vector u without coefficients c', code, M, N, ap, a.ld, 0, 0, m, xp, x.ld, yp, y.ld, up, None)
    refused('rlh_dense_apply: unknown dtype 9', 9, M, N, ap, a.ld, 0, 0, m, xp, x.ld, yp, y.ld, None, None)
    for sizes in ((-1, N, m), (M, -1, m), (M, N, -1)):
        refused('rlh_dense_apply: negative size', code, sizes[0], sizes[1], ap, a.ld, 0, 0, sizes[2], xp, x.ld, yp, y.ld, None, None)
    refused(r'rlh_dense_apply: order must be 0 \(row-major\) or 1 \(column-major\)', code, M, N, ap, a.ld, 2, 0, m, xp, x.ld, yp, y.ld, None, None)
    refused('rlh_dense_apply: transp must be 0 or 1', code, M, N, ap, a.ld, 0, 2, m, xp, x.ld, yp, y.ld, None, None)
    refused('rlh_dense_apply: null pointer', code, M, N, ap, a.ld, 0, 0, m, xp, x.ld, None, y.ld, None, None)
    refused('rlh_dense_apply: null pointer', code, M, N, None, a.ld, 0, 0, m, xp, x.ld, yp, y.ld, None, None)
    refused('rlh_dense_apply: null pointer', code, M, N, ap, a.ld, 0, 0, m, None, x.ld, yp, y.ld, None, cp)
    refused('rlh_dense_apply: lda too small', code, M, N, ap, N - 1, 0, 0, m, xp, x.ld, yp, y.ld, None, None)
    refused('rlh_dense_apply: lda too small', code, M, N, ap, N - 1, 0, 1, m, xp, x.ld, yp, y.ld, None, None)
    refused('rlh_dense_apply: lda too small', code, N, M, ap, N - 1, 1, 0, m, xp, x.ld, yp, y.ld, None, None)
    refused('rlh_dense_apply: Matrix and vectors dimensions incompatible', code, M, N, ap, a.ld, 0, 0, m, xp, N - 1, yp, y.ld, None, None)
    refused('rlh_dense_apply: Matrix and vectors dimensions incompatible', code, M, N, ap, a.ld, 0, 0, m, xp, x.ld, yp, M - 1, None, None)
    refused('rlh_dense_apply: Matrix and vectors dimensions incompatible', code, M, N, ap, a.ld, 0, 1, m, xp, M - 1, yp, y.ld, None, None)
    refused('rlh_dense_apply: Matrix and vectors dimensions incompatible', code, M, N, ap, a.ld, 0, 1, m, xp, x.ld, yp, N - 1, None, cp)
    refused('rlh_dense_apply: too many vectors', code, M, N, ap, a.ld, 0, 0, 65535 * 64 + 1, xp, x.ld, yp, y.ld, None, None)
    apply('d', 65, 33, 9, 0, 1, 'uc')


# ---------------------------------------------------------------------------------------------------- child legs
# RLH_DENSE_MR and RLH_DENSE_WG_PER_CU are read once per process (function-local statics of launch_mfma / launch_mfma16),
# so their legs run in a child process each: tests/_dense_child.py <leg>, with the leg's variables in its environment.
def _leg_mr64(cu):
    """launch_mfma<64, 128>: the first float kernel with 64-row tiles, more than 64 vectors."""
    t = Turn(cu)
    for ny, nx, m, order, transp, epi in pairings('s', 'aligned', cu):
        if m > 64 and nx > 0:
            t.run('s', ny, nx, m, order, transp, epi, 'aligned')
    for ny, m, order, transp, epi, nx in split_cases('s'):
        t.run('s', ny, nx, 65 + m, order, transp, epi, 'aligned')
    assert RATIOS and all('MR64' in family for _, family in RATIOS), 'a case left the 64-row tiles: %s' % sorted(RATIOS)


def wg1_shape(key, cu):
    """(ny, m) with at least one workgroup per CU: four tiles of vectors, ceil(cu / 4) ragged row tiles."""
    m = 512 if key in 'sd' else 256
    return (128 if key == 's' else 64) * ((cu + 3) // 4) - 5, m


def _leg_wg1(cu):
    """One workgroup per CU: no K split where the default target of 8 splits (exact: the same bits either way)."""
    for key in KEYS:
        ny, m = wg1_shape(key, cu)
        for (order, transp), epi in zip(((0, 0), (0, 1)), ('uc', 'c')):
            family, _, taken = plan(key, ny, 1025, m, order, transp, 'aligned', cu)
            assert taken == 1 and plan(key, ny, 1025, m, order, transp, 'aligned', cu, target=8)[2] > 1, (key, family, taken)
            apply(key, ny, 1025, m, order, transp, epi, 'aligned', 'exact', cu)
    assert not any(family.endswith('split') for _, family in RATIOS), 'a case was split: %s' % sorted(RATIOS)


LEGS = {'mr64': ({'RLH_DENSE_MR': '64', 'RLH_DENSE_KERNEL': '1'}, _leg_mr64),
        'wg1': ({'RLH_DENSE_WG_PER_CU': '1'}, _leg_wg1)}


def run_child(leg, cu, timeout=300, fake=False, env_override=None):
    """Starts tests/_dense_child.py for one leg as a fresh process (its own time limit, never retried) and returns the
    completed process."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if not k.startswith('RLH_DENSE_')}
    env.update(LEGS[leg][0])
    env.update(env_override or {})
    here = os.path.dirname(os.path.abspath(__file__))
    cmd = [sys.executable, os.path.join(here, '_dense_child.py'), leg, '--cu', str(cu)] + (['--fake'] if fake else [])
    return subprocess.run(cmd, env=env, timeout=timeout, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
