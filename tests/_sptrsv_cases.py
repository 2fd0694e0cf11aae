"""Sparse triangular solves and the block-diagonal solve, element by element, shared by the CPU tier
(tests/fake_lib.py: shows that SciPy in the working precision meets every bound below) and the GPU tier
(librlhip.so): rlh_sptrsv_create / rlh_sptrsv_info / rlh_sptrsv_solve_chain and rlh_bdiag_solve through the raw
C ABI -- handles through ctypes, blocks through rlh_malloc / rlh_h2d / rlh_d2h -- never through TriangularChain,
which sorts every row first.

Harness.  A block is a host array of m + 2 columns of ld elements (one column per ROW of the array) filled with
values that differ from position to position; B and X are uploaded whole, the call runs on the window of m columns
that starts at column 1, rows [0, n), and both arrays are downloaded again: the window of X is held to the bounds
below, every other byte -- the two guard columns, rows n .. ld - 1, all of B when X != B -- must be what was
uploaded.  Every call is made twice and must give the same bits.

Matrices.  Seeded, in all four types, well conditioned by construction: diagonal moduli in [0.5, 2], the moduli of
a row's off-diagonal entries sum to a quarter of the modulus of its diagonal ("the quarter rule").

Bounds.  u is the unit roundoff of the type's real part, c = 1 for the real types and 2 sqrt 2 for the complex ones
(the bound of a complex product, which also covers a complex sum), L_i the number of STORED off-diagonal entries of
row i, T the factor as given (unit diagonal added, duplicates summed), b the permuted right-hand side.  Residuals
are formed in numpy.longdouble (eps < 2^-60): r = |b - T x^|, d = |T| |x^| + |b|.  They count roundings and are not
measurements.

 (1) Transform off (RLH_SPTRSV_BLOCK=1): r_i <= c (L_i + 4) u d_i.
     The device row is x^_i = w b_i - sum_j m_j x^_j with w = fl(1 / t_ii) and m_j = fl(t_ij / t_ii), formed on the
     host in double and rounded once into the type: at most two roundings of the type per coefficient (one for a
     4-byte type, where the double arithmetic is exact to it; a duplicate entry adds one double rounding, and is
     counted in L_i).  The L_i + 1 terms are dealt to the lanes of the row, every lane runs a chain of fused
     multiply-adds over its terms (one rounding each) and the partial sums are added in a tree: a term passes through
     ceil((L_i + 1) / lanes) + log2(lanes) <= L_i + 1 roundings, however the lanes are chosen.  So
         x^_i = (1 / t_ii) (1 + th_b) b_i - sum_j (t_ij / t_ii) (1 + th_j) x^_j,   |th| <= gamma_{L_i + 3},
     and, multiplied by t_ii,  |b_i - sum_j t_ij x^_j - t_ii x^_i| <= gamma_{L_i + 3} (sum_j |t_ij| |x^_j| + |b_i|)
     <= (L_i + 4) u d_i  (gamma_k = k u / (1 - k u) <= (k + 1) u as long as k (k + 1) u <= 1: k <= 1403 here).  The
     bound is a backward error: it holds whatever the conditioning.  SciPy's solve (columns scaled by the inverse
     diagonal, unit solve, result scaled) has the same count with different names.
 (2) Transform on (RLH_SPTRSV_BLOCK unset or 16).  The host replaces the rows of a chain of up to 16 consecutive
     rows with diagonal block D by the rows of D^-1 T: row i becomes x^_i = sum_k w_ik b_k - sum_j m_ij x^_j, W = D^-1
     and M = W T_off formed in double (at most 16 terms per entry: 16 double roundings relative to |W| |T_off|,
     nothing to a 4-byte type, 16 u to an 8-byte one) and rounded once into the type.  As in (1), with s the
     residual of the transformed rows,  |s| <= gamma (|W| |T_off| |x^| + |W| |b|)  over the block, and since the
     diagonal block of D^-1 T is the identity,  r_blk = D s:
         |r_blk| <= gamma |D| |D^-1| (|T_off| |x^| + |b|)_blk <= gamma |D| |D^-1| d_blk.
     With D = Delta (I - N), Delta the diagonal, the quarter rule says that the rows of |N| sum to at most 1/4, so
     |D| |D^-1| <= |Delta| (I + |N|) (I - |N|)^-1 |Delta|^-1 and the middle factor has rows that sum to at most
     (1 + 1/4) / (1 - 1/4) = 5/3.  Strictly this bounds the residual in units of the diagonal,
         r_i / |t_ii| <= (5/3) gamma max_j d_j / |t_jj|:
     the unscaled form can lose the ratio of two diagonal moduli of one block (at most 4 here) on top.  Both forms are
     asserted with the same constant 2 >= 5/3:
         r_i <= 2 c (L'_i + 4) u max{d_j : |j - i| < 16},   r_i / |t_ii| <= 2 c (L'_i + 4) u max{d_j / |t_jj| : |j - i| < 16},
     L'_i = 16 + the largest L_j with |j - i| < 16.  The 16 pays for the block's own right-hand side entries and for
     the double roundings of W T_off; a transformed row whose lanes hold one batch of four entries passes a term
     through at most 4 + log2(256) = 12 roundings, one that is longer (more than 1024 / pl entries, pl the lanes
     across the pieces of a row) through entries * pl / 256 + 8, and its entries are at most the union of 16 rows'.
     A matrix that does not obey the quarter rule (the ILUT factors) takes its own constant in place of the 2:
     Factor.kappa(), the same (1 + s) / (1 - s) with its own largest row sum s of |N| times its own largest ratio of
     two diagonal moduli.
 (3) Chains.  A chain call must give the BITS of the same operators applied one call at a time (every row does the
     same operations in the same order: only the image its right-hand side entries read differs), so every stage
     is held to (1) or (2) through the single calls.  The end result is held against SciPy in float64 /
     complex128, refined twice with longdouble residuals (its own error is then 2^-11 u or less of an 8-byte type):
         |x^ - x| <= E_k,   E_0 = 0,   E_j = |T_j^-1| (E_j-1 + rho_j),
     rho_j the residual bound of stage j as asserted, |T_j^-1| the dense inverse in float64.
 (4) rlh_bdiag_solve: x'_i = coef_0 x_i + coef_1 x_{i+s} is two products and one sum,
         |x'_i - exact| <= 3 c u (|coef_0| |x_i| + |coef_1| |x_{i+s}|);
     a fused multiply-add removes the rounding of ONE of the two products (the other product is rounded before it
     enters the fused operation), a row with s = 0 is one product: its coef_1 is never read (the cases fill it with
     NaN).
"""

import ctypes
import functools
import math

import numpy as np
import scipy.linalg
import scipy.sparse as sp
import scipy.sparse.linalg as sla

DT = {'s': np.float32, 'd': np.float64, 'c': np.complex64, 'z': np.complex128}
WIDE = {'s': np.float64, 'd': np.float64, 'c': np.complex128, 'z': np.complex128}
LONG = {'s': np.longdouble, 'd': np.longdouble, 'c': np.clongdouble, 'z': np.clongdouble}
KEYS = ['s', 'd', 'c', 'z']
assert np.finfo(np.longdouble).eps < 2.0 ** -60

BLOCKS = [None, '1', '16']                   # RLH_SPTRSV_BLOCK at create time (None: unset)
WINDOW = 16                                  # the most rows the transform puts into one diagonal block
RATIOS = {}                                  # (what, key, mode) -> largest error / bound seen


def epl(key):
    return 16 // np.dtype(DT[key]).itemsize


def unit_roundoff(key):
    return float(np.finfo(np.float32 if key in 'sc' else np.float64).eps) / 2


def cfac(key):
    return 2.0 * math.sqrt(2.0) if key in 'cz' else 1.0


def m_list(key):
    e = epl(key)
    out = []
    for m in (1, e - 1, e, e + 1, 8 * e, 8 * e + 1, 70):
        if m > 0 and m not in out:
            out.append(m)
    return out


def big_m(key):
    """More than 512 pieces of 16 bytes per row: a group holds 65 of them, the lanes across them take two trips."""
    return 512 * epl(key) + 1


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def note_ratio(what, key, mode, ratio):
    k = (what, key, mode)
    RATIOS[k] = max(RATIOS.get(k, 0.0), float(ratio))


def ratios_text():
    return '\n'.join('ratio error/bound  %-28s %s %-8s %.3f' % (k[0], k[1], k[2], v) for k, v in sorted(RATIOS.items()))


def native():
    from raleigh_amd import _lib
    return isinstance(_lib.library(), ctypes.CDLL)


# ---------------------------------------------------------------------------------------------------- matrices
def _unit_modulus(rng, key, size):
    if key in 'cz':
        return np.exp(2j * np.pi * rng.uniform(0.0, 1.0, size))
    return rng.choice([-1.0, 1.0], size)


def _raw(rng, key, size):
    v = rng.uniform(0.25, 1.0, size) * rng.choice([-1.0, 1.0], size)
    if key in 'cz':
        v = v + 1j * rng.uniform(0.25, 1.0, size) * rng.choice([-1.0, 1.0], size)
    return v


class Factor:
    """A triangular factor on the host: T (CSR in the working type, sorted, diagonal stored even when it is a unit
    one), its longdouble images and what the bounds need of it."""

    def __init__(self, name, key, T, lower, unit):
        self.name, self.key, self.lower, self.unit = name, key, bool(lower), bool(unit)
        T = sp.csr_matrix(T, dtype=DT[key])
        T.sum_duplicates()
        T.sort_indices()
        self.T, self.n = T, T.shape[0]
        self.Tl = T.astype(LONG[key])
        self.Al = abs(self.Tl)
        self.diag = T.diagonal()
        assert np.all(self.diag != 0)
        self.offcount = np.diff(T.indptr) - 1

    # -- storage forms of the same matrix, as the raw ABI takes them
    def storage(self, form='sorted', seed=0):
        """(indptr, indices, values): 'sorted'; 'shuffled' -- every row in random order behind its diagonal, which comes
        first; 'split' -- sorted, one off-diagonal entry of every row that has one stored as two duplicates that sum
        to it exactly (a = fl(0.625 t), b = t - a, exact since a lies within a factor two of t)."""
        T, n = self.T, self.n
        rng = np.random.default_rng(1000 + seed)
        ip, ix, va = [0], [], []
        for i in range(n):
            c = T.indices[T.indptr[i]:T.indptr[i + 1]]
            v = T.data[T.indptr[i]:T.indptr[i + 1]]
            on = c == i
            oc, ov = c[~on], v[~on]
            if form == 'shuffled':
                p = rng.permutation(oc.size)
                oc, ov = oc[p], ov[p]
            elif form == 'split' and oc.size:
                k = int(rng.integers(oc.size))
                t = ov[k]
                if self.key in 'cz':
                    real = DT[self.key](0).real.dtype.type
                    a = DT[self.key](complex(real(0.625) * t.real, real(0.625) * t.imag))
                else:
                    a = DT[self.key](0.625) * t
                b = t - a
                assert a + b == t
                oc = np.concatenate([oc[:k + 1], oc[k:]])
                ov = np.concatenate([ov[:k], [a, b], ov[k + 1:]]).astype(DT[self.key])
            if not self.unit:
                if form == 'shuffled' or not self.lower:
                    oc, ov = np.concatenate([c[on], oc]), np.concatenate([v[on], ov])
                else:
                    oc, ov = np.concatenate([oc, c[on]]), np.concatenate([ov, v[on]])
            ix.append(oc)
            va.append(ov)
            ip.append(ip[-1] + oc.size)
        indptr = np.asarray(ip, dtype=np.int64)
        if indptr[-1] == 0:
            return indptr, None, None
        return (indptr, np.ascontiguousarray(np.concatenate(ix), dtype=np.int32),
                np.ascontiguousarray(np.concatenate(va), dtype=DT[self.key]))

    def longest_path(self):
        """Rows on the longest dependency path: the levels of the factor as given."""
        T, n = self.T, self.n
        lev = np.zeros(max(n, 1), dtype=np.int64)
        for i in (range(n) if self.lower else range(n - 1, -1, -1)):
            c = T.indices[T.indptr[i]:T.indptr[i + 1]]
            c = c[c != i]
            lev[i] = lev[c].max() + 1 if c.size else 0
        return int(lev[:n].max()) + 1 if n else 0

    def reached_from(self, rows):
        """Rows whose result depends on the right-hand side of one of `rows` (these included)."""
        T, n = self.T, self.n
        hit = np.zeros(n, dtype=bool)
        hit[list(rows)] = True
        for i in (range(n) if self.lower else range(n - 1, -1, -1)):
            if hit[T.indices[T.indptr[i]:T.indptr[i + 1]]].any():
                hit[i] = True
        return hit

    def kappa(self):
        """(1 + s) / (1 - s) times the largest ratio of two diagonal moduli: what |D| |D^-1| of any diagonal block of
        this matrix is bounded by (bound (2) of the header for a matrix that does not obey the quarter rule)."""
        a = np.abs(self.diag).astype(np.float64)
        off = np.asarray(abs(self.T).sum(axis=1)).ravel().astype(np.float64) - a
        s = float(np.max(off / a)) if self.n else 0.0
        assert s < 1.0
        return (1.0 + s) / (1.0 - s) * float(a.max() / a.min())

    def refsolve(self, b):
        """T^-1 b for a longdouble b: SciPy in float64 / complex128, refined twice with longdouble residuals."""
        T64 = self.T.astype(WIDE[self.key])
        x = sla.spsolve_triangular(T64, np.asarray(b, dtype=WIDE[self.key]), lower=self.lower).astype(LONG[self.key])
        for _ in range(2):
            r = b - self.Tl @ x
            x = x + sla.spsolve_triangular(T64, np.asarray(r, dtype=WIDE[self.key]), lower=self.lower)
        return x


_INVERSES = {}


def absinv(f):
    """|T^-1|, dense, float64 (the last few are kept: 32 MB each at n = 2003)."""
    k = id(f)
    if k not in _INVERSES:
        while len(_INVERSES) >= 4:
            _INVERSES.pop(next(iter(_INVERSES)))
        inv = scipy.linalg.solve_triangular(f.T.astype(WIDE[f.key]).toarray(), np.eye(f.n), lower=f.lower)
        _INVERSES[k] = (f, np.abs(inv))
    return _INVERSES[k][1]


def assemble(name, key, n, patterns, lower, unit, seed):
    """The quarter rule on a pattern: patterns[i] holds the distinct off-diagonal columns of row i."""
    rng = np.random.default_rng(seed)
    diag = np.ones(n) if unit else rng.uniform(0.5, 2.0, n) * _unit_modulus(rng, key, n)
    rows, cols, vals = [np.arange(n)], [np.arange(n)], [diag]
    for i, c in enumerate(patterns):
        c = np.asarray(c, dtype=np.int64)
        if c.size == 0:
            continue
        v = _raw(rng, key, c.size)
        v *= 0.25 * abs(diag[i]) / np.abs(v).sum()
        rows.append(np.full(c.size, i))
        cols.append(c)
        vals.append(v)
    T = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    return Factor(name, key, T, lower, unit)


def transposed(patterns, n):
    out = [[] for _ in range(n)]
    for i, c in enumerate(patterns):
        for j in c:
            out[int(j)].append(i)
    return out


STAIR_L = [0, 1, 4, 5, 16, 17, 64, 65, 256, 257, 1024, 1025, 1399]


def staircase_patterns(n, seed):
    """Row i: min(i, L) entries at random earlier columns, one of them i - 1; L cycles through STAIR_L."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        k = min(i, STAIR_L[i % len(STAIR_L)])
        if k == 0:
            out.append([])
        elif k == i:
            out.append(np.arange(i))
        else:
            out.append(np.concatenate([rng.choice(i - 1, k - 1, replace=False), [i - 1]]) if k > 1 else [i - 1])
    return out


def random_patterns(n, seed, most=12):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, most + 1, n)
    return [rng.choice(i, min(i, int(counts[i])), replace=False) if i else [] for i in range(n)]


def block_patterns(n, seed, node=5):
    """Nodes of five rows that each read every earlier row of the node; the rows of a node share one pattern of 5 to
    10 columns in the two nodes before it."""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(n // node):
        lo = max(0, (b - 2) * node)
        avail = b * node - lo
        shared = lo + rng.choice(avail, min(avail, int(rng.integers(5, 11))), replace=False) if avail else np.zeros(0, dtype=np.int64)
        for r in range(node):
            out.append(np.concatenate([shared, b * node + np.arange(r)]).astype(np.int64))
    return out


def _triple(tag, key, n, pat, seed):
    """Lu (unit lower), Ln (lower) and U (upper, the transposed pattern) on one pattern."""
    up = transposed(pat, n)
    return {'Lu': assemble(tag + ' Lu', key, n, pat, True, True, seed),
            'Ln': assemble(tag + ' Ln', key, n, pat, True, False, seed + 1),
            'U': assemble(tag + ' U', key, n, up, False, False, seed + 2)}


@functools.lru_cache(maxsize=64)
def family(name, key, n=None):
    """The factors of a family: a dict with 'Lu' (unit lower), 'U' (upper) and, but for the ILUT factors, 'Ln' (lower
    with a diagonal of its own)."""
    if name == 'diagonal':
        none = [[] for _ in range(n)]
        return _triple('diagonal %d' % n, key, n, none, 100 + n)
    if name == 'staircase':
        n = n or 1400
        return _triple('staircase %d' % n, key, n, staircase_patterns(n, 7), 200)
    if name == 'random':
        return _triple('random', key, 2003, random_patterns(2003, 8), 300)
    if name == 'blocks':
        return _triple('blocks', key, 1000, block_patterns(1000, 9), 400)
    if name == 'bidiagonal':
        return _triple('bidiagonal', key, 300, [[i - 1] if i else [] for i in range(300)], 500)
    if name == 'ilut':
        return ilut_factors(key)
    raise KeyError(name)


def ilut_factors(key):
    """The ILUT(1e-8, 9) factors of lap3d(9, 8, 7) (complex types: plus a Hermitian imaginary part), read with
    rlh_factors_get and cast to the working type."""
    from raleigh_amd import _lib
    from oracle.sparse import lap3d
    A = lap3d(9, 8, 7, 1.0, 1.01, 1.02)
    n = A.shape[0]
    dt = np.float64
    if key in 'cz':
        S = sp.diags([np.full(n - 1, 40.0)], [1])
        A = sp.csr_matrix(A.astype(np.complex128) + 1j * S - 1j * S.T)
        dt = np.complex128
    A.sort_indices()
    L = _lib.library()
    f = ctypes.c_void_p()
    ip, ix, va = (np.ascontiguousarray(A.indptr, dtype=np.int64), np.ascontiguousarray(A.indices, dtype=np.int32),
                  np.ascontiguousarray(A.data, dtype=dt))
    _lib.check(L.rlh_ilut_factor(ctypes.byref(f), _lib.DTYPE_CODE[dt], n, _lib.host_ptr(ip), _lib.host_ptr(ix),
                                 _lib.host_ptr(va), 1e-8, 9))
    out = {}
    try:
        nl, nu = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(L.rlh_factors_nnz(f, ctypes.byref(nl), ctypes.byref(nu)))
        for which, nnz, name in ((0, nl.value, 'Lu'), (1, nu.value, 'U')):
            p = np.zeros(n + 1, dtype=np.int64)
            i = np.zeros(max(nnz, 1), dtype=np.int32)
            v = np.zeros(max(nnz, 1), dtype=dt)
            _lib.check(L.rlh_factors_get(f, which, _lib.host_ptr(p), _lib.host_ptr(i), _lib.host_ptr(v)))
            raw = (p, i[:nnz].copy(), v[:nnz].astype(DT[key]))
            if which == 1:
                assert np.array_equal(i[p[:-1]], np.arange(n)), 'U rows come with the diagonal first'
            M = sp.csr_matrix((raw[2], raw[1], raw[0]), shape=(n, n))
            if which == 0:
                M = M + sp.identity(n, dtype=DT[key], format='csr')
            fac = Factor('ilut ' + name, key, M, which == 0, which == 0)
            fac.raw = raw
            out[name] = fac
    finally:
        L.rlh_factors_destroy(f)
    return out


# ---------------------------------------------------------------------------------------------------- harness
class Handle:
    """A device operator made of a Factor in one storage form."""

    def __init__(self, factor, form='sorted', seed=0):
        from raleigh_amd import _lib
        self._L = _lib.lib()
        self.factor = factor
        if form == 'raw':
            indptr, indices, values = factor.raw
        else:
            indptr, indices, values = factor.storage(form, seed)
        self.counts = np.diff(indptr) - (0 if factor.unit else 1)        # stored off-diagonal entries
        self.h = ctypes.c_void_p()
        rc = self._L.rlh_sptrsv_create(ctypes.byref(self.h), _lib.dtype_code(DT[factor.key]), factor.n, _lib.host_ptr(indptr),
                                       _lib.host_ptr(indices) if indices is not None else None,
                                       _lib.host_ptr(values) if values is not None else None,
                                       1 if factor.lower else 0, 1 if factor.unit else 0)
        _lib.check(rc)

    def info(self):
        from raleigh_amd import _lib
        nnz, lev, nb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        _lib.check(self._L.rlh_sptrsv_info(self.h, ctypes.byref(nnz), ctypes.byref(lev), ctypes.byref(nb)))
        return int(nnz.value), int(lev.value)

    def close(self):
        h, self.h = getattr(self, 'h', None), None
        if h:
            self._L.rlh_sptrsv_destroy(h)

    __del__ = close


def handle_array(handles):
    return (ctypes.c_void_p * len(handles))(*[h.h.value for h in handles])


_POOL = {}


def _pool(dtype, count, offset=0):
    dtype = np.dtype(dtype)
    have = _POOL.get(dtype)
    if have is None or have.size < count + offset:
        size = max(count + offset, 1 << 20)
        rng = np.random.default_rng(4040 + dtype.num)
        have = rng.standard_normal(size)
        if dtype.kind == 'c':
            have = have + 1j * rng.standard_normal(size)
        have = have.astype(dtype)
        have.setflags(write=False)
        _POOL[dtype] = have
    return have[offset:offset + count]


def rhs(key, n, m, seed=0):
    """An (m, n) right-hand side (one column per row of the array)."""
    return _pool(DT[key], n * m, 17 + 101 * seed).reshape(m, n).copy()


def _device(host):
    from raleigh_amd import _lib
    from raleigh_amd.algebra.hip.memory import DeviceBuffer
    buf = DeviceBuffer(host.nbytes + 16, zero=False)
    _lib.check(_lib.lib().rlh_h2d(buf.ptr, _lib.host_ptr(host), host.nbytes))
    return buf


def _fetch(buf, like):
    from raleigh_amd import _lib
    out = np.empty_like(like)
    _lib.check(_lib.lib().rlh_d2h(_lib.host_ptr(out), buf.ptr, out.nbytes))
    return out


def solve(handles, b, perm_in=None, perm_out=None, ldb=None, ldx=None, inplace=False, expect_error=None, what='',
          null_b=False, m_arg=None):
    """One rlh_sptrsv_solve_chain on the (m, n) block b.  Returns the window of X (rows of X as written: after
    perm_out); the whole of X outside it and the whole of B (X != B) must be what was uploaded.  expect_error: the
    call must return non-zero with this text in its message and leave X as it was."""
    from raleigh_amd import _lib
    L = _lib.lib()
    key = handles[0].factor.key
    n = handles[0].factor.n
    m = b.shape[0]
    ldb = n if ldb is None else ldb
    ldx = ldb if inplace or ldx is None else ldx
    es = np.dtype(DT[key]).itemsize
    hb = _pool(DT[key], (m + 2) * max(ldb, 1), 3).reshape(m + 2, max(ldb, 1)).copy()
    hb[1:m + 1, :n] = b[:, :n]
    db = _device(hb)
    if inplace:
        hx, dx = hb, db
    else:
        hx = _pool(DT[key], (m + 2) * max(ldx, 1), 7777).reshape(m + 2, max(ldx, 1)).copy()
        dx = _device(hx)
    pin = _device(np.ascontiguousarray(perm_in, dtype=np.int64)) if perm_in is not None else None
    pout = _device(np.ascontiguousarray(perm_out, dtype=np.int64)) if perm_out is not None else None
    rc = L.rlh_sptrsv_solve_chain(len(handles), handle_array(handles), pin.ptr if pin else None, pout.ptr if pout else None,
                                  m if m_arg is None else m_arg, None if null_b else db.ptr + max(ldb, 1) * es, ldb,
                                  dx.ptr + max(ldx, 1) * es, ldx)
    if expect_error is not None:
        assert rc != 0, 'accepted: ' + what
        msg = L.rlh_last_error()
        msg = msg.decode() if isinstance(msg, bytes) else str(msg)
        assert expect_error in msg, '%r lacks %r %s' % (msg, expect_error, what)
        _lib.check(L.rlh_sync())
        assert same_bytes(_fetch(dx, hx), hx), 'a refused call wrote to X ' + what
        return None
    _lib.check(rc)
    _lib.check(L.rlh_sync())
    gx = _fetch(dx, hx)
    win = gx[1:m + 1, :n].copy()
    rest = gx
    rest[1:m + 1, :n] = hx[1:m + 1, :n]
    assert same_bytes(rest, hx), 'guard columns or padding rows of X modified ' + what
    if not inplace:
        assert same_bytes(_fetch(db, hb), hb), 'B modified ' + what
    return win


def solve_twice(handles, b, **kw):
    x = solve(handles, b, **kw)
    assert same_bytes(x, solve(handles, b, **kw)), 'two runs of one call differ ' + kw.get('what', '')
    return x


# ---------------------------------------------------------------------------------------------------- bounds
def _window_max(a):
    """max over |j - i| < WINDOW along axis 0."""
    n = a.shape[0]
    out = a.copy()
    for s in range(1, WINDOW):
        if s >= n:
            break
        np.maximum(out[s:], a[:-s], out=out[s:])
        np.maximum(out[:-s], a[s:], out=out[:-s])
    return out


def residual_bound(h, b, x, mode, what, tag):
    """Bounds (1) / (2) of the header for one operator: b (n, m) the right-hand side as the operator saw it, x (n, m) the
    result in the working type.  Returns the bound on |b - T x| as asserted, in float64."""
    f = h.factor
    key = f.key
    u, c = unit_roundoff(key), cfac(key)
    bl = np.asarray(b, dtype=LONG[key])
    xl = np.asarray(x).astype(LONG[key])
    r = np.abs(bl - f.Tl @ xl)
    d = f.Al @ np.abs(xl) + np.abs(bl)
    cnt = h.counts.astype(np.float64)
    if mode == 'off':
        bound = (c * (cnt + 4) * u)[:, None] * d
        ok = r <= bound
        ratio = np.max(r / bound) if r.size else 0.0
    else:
        K = 2.0 if not hasattr(f, 'raw') else max(2.0, f.kappa())
        lw = (K * c * (_window_max(cnt) + WINDOW + 4) * u)[:, None]
        a = np.abs(f.diag).astype(np.longdouble)[:, None]
        bound = lw * _window_max(d)
        scaled = lw * _window_max(d / a)
        ok = (r <= bound) & (r / a <= scaled)
        ratio = max(np.max(r / bound), np.max(r / a / scaled)) if r.size else 0.0
    if not np.all(ok):
        i, j = np.argwhere(~ok)[0]
        raise AssertionError('(row %d, column %d): residual %.3e above the bound %.3e (%d stored entries) %s'
                             % (i, j, r[i, j], bound[i, j], cnt[i], what))
    note_ratio(tag, key, mode, ratio)
    return np.asarray(bound, dtype=np.float64) * (1.0 + 1e-12)


def forward_check(stages, b0, x, what, tag, mode):
    """Bound (3): stages = [(handle, rho)], b0 (n, m) the permuted right-hand side, x (n, m) the end result."""
    key = stages[0][0].factor.key
    ref = np.asarray(b0, dtype=LONG[key])
    E = 0.0
    for h, rho in stages:
        ref = h.factor.refsolve(ref)
        E = absinv(h.factor) @ (E + rho)
    E = E * (1.0 + 1e-8)
    err = np.abs(np.asarray(x).astype(LONG[key]) - ref)
    ok = err <= E
    if not np.all(ok):
        i, j = np.argwhere(~ok)[0]
        raise AssertionError('(row %d, column %d): error %.3e above the bound %.3e %s' % (i, j, err[i, j], E[i, j], what))
    if err.size:
        note_ratio(tag + ' forward', key, mode, np.max(err / np.where(E > 0, E, 1)))


def mode_of(block):
    return 'off' if block == '1' else 'on'


def single(h, b, mode, tag, what, **kw):
    """One operator alone: twice the same bits, bounds (1) / (2) and (3).  Returns the window."""
    x = solve_twice([h], b, what=what, **kw)
    rho = residual_bound(h, b.T, x.T, mode, what, tag)
    forward_check([(h, rho)], b.T, x.T, what, tag, mode)
    return x


def chain(handles, b, mode, tag, what, perm_in=None, perm_out=None, **kw):
    """A chain call against the same operators one call at a time (bits), every stage under (1) / (2), the end
    result under (3).  Returns the window of the chain call."""
    n = handles[0].factor.n
    xc = solve_twice(handles, b, perm_in=perm_in, perm_out=perm_out, what=what, **kw)
    cur = b
    stages = []
    for k, h in enumerate(handles):
        first, last = k == 0, k == len(handles) - 1
        nxt = solve([h], cur, perm_in=perm_in if first else None, perm_out=perm_out if last else None,
                    what=what + ' step %d' % k)
        seen = cur[:, perm_in] if first and perm_in is not None else cur         # what the operator read
        made = nxt[:, perm_out] if last and perm_out is not None else nxt       # what it wrote, by internal row
        stages.append((h, residual_bound(h, seen.T, made.T, mode, what + ' step %d' % k, tag)))
        cur = nxt
    assert same_bytes(xc, cur), 'the chain differs from its operators applied one call at a time ' + what
    b0 = b[:, perm_in] if perm_in is not None else b
    xe = xc[:, perm_out] if perm_out is not None else xc
    forward_check(stages, b0.T, xe.T, what, tag, mode)
    return xc


# ---------------------------------------------------------------------------------------------------- the calls
def make_handles(fam, form='sorted'):
    return {name: Handle(f, 'raw' if hasattr(f, 'raw') else form) for name, f in fam.items()}


def close_all(hs):
    for h in hs.values():
        h.close()


def set_block(monkeypatch, block):
    """RLH_SPTRSV_BLOCK as rlh_sptrsv_create will read it (None: unset)."""
    if block is None:
        monkeypatch.delenv('RLH_SPTRSV_BLOCK', raising=False)
    else:
        monkeypatch.setenv('RLH_SPTRSV_BLOCK', block)


def calls(name, key, block, monkeypatch, n=None):
    """The whole set of calls on one family created under RLH_SPTRSV_BLOCK = block (None: unset)."""
    set_block(monkeypatch, block)
    for v in ('RLH_SPTRSV_WG_PER_CU', 'RLH_SPTRSV_NAP'):
        monkeypatch.delenv(v, raising=False)
    fam = family(name, key, n)
    hs = make_handles(fam)
    try:
        _calls(name, key, block, monkeypatch, fam, hs)
    finally:
        close_all(hs)


def _calls(name, key, block, monkeypatch, fam, hs):
    mode = mode_of(block)
    tag = name
    A = hs.get('Ln', hs['Lu'])
    Lu, U = hs['Lu'], hs['U']
    n = A.factor.n
    e = epl(key)
    rng = np.random.default_rng(n + e)
    pin, pout = rng.permutation(n), rng.permutation(n)
    replay = []                                                  # (handles, b, keywords, bits) for the call-time switches

    def T(m, k):
        return '[%s %s block=%s m=%d %s]' % (name, key, block, m, k)

    # ---- one operator, every m, leading dimensions n and n + 3 in turn
    for q, m in enumerate(m_list(key)):
        b = rhs(key, n, m, q)
        for k, h in (('lower', A), ('upper', U)):
            kw = dict(ldb=n + 3 * (q & 1), ldx=n + 3 * ((q >> 1) & 1))
            x = single(h, b, mode, tag, T(m, k), **kw)
            if m in (1, 8 * e + 1, 70):
                replay.append(([h], b, kw, x))
    x = single(Lu, rhs(key, n, e + 1, 9), mode, tag, T(e + 1, 'unit lower'))
    if fam['Lu'].offcount.max() == 0:                            # nothing stored at all: the result is B
        assert same_bytes(x, rhs(key, n, e + 1, 9))
        b = rhs(key, n, 3, 10)
        x = solve_twice([Lu], b, perm_in=pin, perm_out=pout, what=T(3, 'empty unit factor, permutations'))
        want = np.empty_like(b)
        want[:, pout] = b[:, pin]
        assert same_bytes(x, want)
    # ---- chains
    kinds = [('L U', [Lu, U], None, None), ('L U permuted', [Lu, U], pin, pout), ('L U L', [A, U, A], None, None),
             ('eight', [Lu, U] * 4, None, None), ('twice', [A, A], None, None)]
    for m in (e + 1, 8 * e + 1):
        b = rhs(key, n, m, 11)
        for k, ops, p_in, p_out in kinds:
            if m != e + 1 and k != 'L U permuted':
                continue
            x = chain(ops, b, mode, tag, T(m, 'chain ' + k), perm_in=p_in, perm_out=p_out)
            if k in ('L U permuted', 'eight'):
                replay.append((ops, b, dict(perm_in=p_in, perm_out=p_out), x))
    # ---- leading dimensions, out of place and in place: the same bits every way
    m = e + 1
    b = rhs(key, n, m, 12)
    first = None
    for ldb, ldx, inplace in ((n, n, False), (n, n + 3, False), (n + 3, n, False), (n + 3, n + 3, False), (n, n, True),
                              (n + 3, n + 3, True)):
        x = solve_twice([Lu, U], b, perm_in=pin, perm_out=pout, ldb=ldb, ldx=ldx, inplace=inplace,
                        what=T(m, 'ldb=%d ldx=%d inplace=%s' % (ldb, ldx, inplace)))
        if first is None:
            first = x
        assert same_bytes(x, first), T(m, 'ldb=%d ldx=%d inplace=%s differs from ldb=ldx=n' % (ldb, ldx, inplace))
    assert same_bytes(first, chain([Lu, U], b, mode, tag, T(m, 'chain for the leading dimensions'), perm_in=pin, perm_out=pout))
    # ---- call-time switches: the order of the operations inside a row does not depend on the schedule
    for var, val in (('RLH_SPTRSV_WG_PER_CU', '1'), ('RLH_SPTRSV_NAP', '4')):
        monkeypatch.setenv(var, val)
        for ops, b, kw, bits in replay:
            x = solve_twice(ops, b, what=T(b.shape[0], '%s=%s' % (var, val)), **kw)
            assert same_bytes(x, bits), T(b.shape[0], 'differs under %s=%s' % (var, val))
        monkeypatch.delenv(var)
    refusals(key, hs, n)


def refusals(key, hs, n):
    """Calls that must return non-zero with a message and leave X alone; empty calls that return 0 and write nothing."""
    Lu, U = hs['Lu'], hs['U']
    b = rhs(key, n, 3, 13)
    solve([Lu, U] * 4 + [Lu], b, expect_error='1 to 8 operators', what='nine operators')
    if n > 1:
        solve([Lu], b, ldb=n, ldx=n - 1, expect_error='bad block arguments', what='ldx < n')
        solve([Lu], b[:, :n - 1], ldb=n - 1, ldx=n, expect_error='bad block arguments', what='ldb < n')
    solve([Lu], b, null_b=True, expect_error='bad block arguments', what='B = NULL')
    solve([Lu], b, m_arg=65537, expect_error='bad block size', what='m = 65537')
    small = Handle(family('diagonal', key, n + 1)['Ln'])
    solve([Lu, small], b, expect_error='one type and one size', what='two sizes')
    small.close()
    other = Handle(family('diagonal', 'd' if key != 'd' else 's', n)['Ln'])
    solve([Lu, other], b, expect_error='one type and one size', what='two types')
    other.close()
    # m = 0: accepted, nothing written (the window is empty: all of X is guard)
    assert solve([Lu, U], b[:0]).shape == (0, n)


def empty_operator(key):
    """n = 0: the handle is made, a solve returns 0 and writes nothing."""
    f = Factor('empty', key, sp.csr_matrix((0, 0), dtype=DT[key]), True, False)
    h = Handle(f)
    assert h.info() == (0, 0)
    x = solve([h], np.zeros((3, 0), dtype=DT[key]), ldb=0, ldx=0)
    assert x.shape == (3, 0)
    h.close()


def m_zero_writes_nothing(key):
    fam = family('diagonal', key, 9)
    h = Handle(fam['Ln'])
    b = rhs(key, 9, 3, 1)
    from raleigh_amd import _lib
    L = _lib.lib()
    hx = _pool(DT[key], 5 * 9, 5).reshape(5, 9).copy()
    dx, db = _device(hx), _device(b)
    _lib.check(L.rlh_sptrsv_solve_chain(1, handle_array([h]), None, None, 0, db.ptr, 9, dx.ptr, 9))
    _lib.check(L.rlh_sync())
    assert same_bytes(_fetch(dx, hx), hx)
    h.close()


def large_m(name, key, block, monkeypatch, n=None):
    """m = 512 pieces + 1 on a small matrix: the second trip of the lanes across the pieces of a row."""
    set_block(monkeypatch, block)
    fam = family(name, key, n)
    hs = make_handles(fam)
    try:
        mode, m = mode_of(block), big_m(key)
        nn = hs['Lu'].factor.n
        b = rhs(key, nn, m, 14)
        tag = '%s large m' % name
        what = '[%s %s block=%s m=%d]' % (name, key, block, m)
        single(hs['Ln'], b, mode, tag, what + ' lower', ldb=nn + 3, ldx=nn)
        single(hs['U'], b, mode, tag, what + ' upper')
        rng = np.random.default_rng(5)
        chain([hs['Lu'], hs['U']], b, mode, tag, what + ' chain', perm_in=rng.permutation(nn), perm_out=rng.permutation(nn))
    finally:
        close_all(hs)


def plan_cache(key, block, monkeypatch):
    """Three different numbers of lanes across a row's pieces on one handle (two plans are kept): pl = 1, 2, 16, then 1
    again, which must rebuild the evicted plan and give the first result's bits."""
    set_block(monkeypatch, block)
    fam = family('staircase', key)
    mode = mode_of(block)
    e = epl(key)
    for name in ('Ln', 'U'):
        h = Handle(fam[name])
        n = h.factor.n
        b = rhs(key, n, 72 * e, 15)
        got = []
        for m in (1, 8 * e + 1, 72 * e, 1):                      # 1, 9 and 72 pieces: 1, 2 and 9 per group
            got.append(single(h, b[:m], mode, 'staircase plans', '[plan cache %s %s block=%s m=%d]' % (name, key, block, m)))
        assert same_bytes(got[0], got[3]), 'the rebuilt plan gives other bits'
        h.close()


def storage_forms(key, block, monkeypatch):
    """Sorted rows, shuffled rows with the diagonal first, and one entry of every row split into two duplicates."""
    set_block(monkeypatch, block)
    fam = family('random', key)
    mode = mode_of(block)
    e = epl(key)
    for name in ('Ln', 'U', 'Lu'):
        f = fam[name]
        hs = {form: Handle(f, form, seed=3) for form in ('sorted', 'shuffled', 'split')}
        assert hs['split'].info()[0] == hs['sorted'].info()[0] + int((f.offcount > 0).sum())
        assert hs['sorted'].info()[0] == int(f.offcount.sum()) == hs['shuffled'].info()[0]
        for m in (1, e + 1, 70):
            b = rhs(key, f.n, m, 16)
            what = '[random %s %s block=%s m=%d]' % (name, key, block, m)
            xs = single(hs['sorted'], b, mode, 'random forms', what + ' sorted')
            assert same_bytes(xs, solve_twice([hs['shuffled']], b, what=what + ' shuffled')), 'shuffled rows give other bits ' + what
            single(hs['split'], b, mode, 'random forms', what + ' split')
        close_all(hs)


def levels(key, monkeypatch):
    """rlh_sptrsv_info: exactly the longest dependency path with the transform off, never more with it on, fewer on
    the chained blocks and the bidiagonal matrix (the stand-in of the CPU tier has no transform)."""
    for name in ('blocks', 'bidiagonal', 'staircase', 'random'):
        fam = family(name, key)
        for fname, f in fam.items():
            path = f.longest_path()
            for block in BLOCKS:
                set_block(monkeypatch, block)
                h = Handle(f)
                nnz, lev = h.info()
                h.close()
                assert nnz == int(f.offcount.sum())
                if block == '1':
                    assert lev == path, (name, fname, block, lev, path)
                else:
                    assert lev <= path, (name, fname, block, lev, path)
                    if block is None:                        # kept only where it removes a tenth of the levels, else undone
                        assert lev == path or lev <= 0.9 * path, (name, fname, lev, path)
                    if native() and name in ('blocks', 'bidiagonal'):
                        assert lev < path, (name, fname, block, lev, path)


def nonfinite(key, monkeypatch):
    """+Inf, a quiet NaN and the NaN whose words are the hand-off pattern in column 2 of B: a normal return, the
    other columns and the rows out of reach as without them, the three rows themselves not finite."""
    from raleigh_amd import _lib
    assert key in 'sd'
    set_block(monkeypatch, None)
    f = family('random', key)['Ln']
    h = Handle(f)
    n, m = f.n, 5
    b = rhs(key, n, m, 17)
    clean = solve_twice([h], b, what='[non-finite: clean run]')
    rows = (1500, 1700, 1900)
    bad = b.copy()
    bad[2, rows[0]] = np.inf
    bad[2, rows[1]] = np.nan
    if key == 's':
        pattern = np.array([0xFFFFDEAD], dtype=np.uint32).view(np.float32)[0]
    else:
        pattern = np.array([0xFFFFDEAD12345678], dtype=np.uint64).view(np.float64)[0]
    bad[2, rows[2]] = pattern
    assert np.isnan(pattern) and not same_bytes(bad[2, rows[2]:rows[2] + 1], bad[2, rows[1]:rows[1] + 1])
    x = solve_twice([h], bad, what='[non-finite]')             # (the call and rlh_sync returned 0)
    _lib.check(_lib.lib().rlh_sync())
    for col in (0, 1, 3, 4):
        assert same_bytes(x[col], clean[col]), 'column %d differs' % col
    hit = f.reached_from(rows)
    assert hit[list(rows)].all() and not hit[:rows[0]].any() and hit.sum() > 3 and (~hit[rows[0]:]).sum() > 3
    assert same_bytes(x[2, ~hit], clean[2, ~hit]), 'rows out of reach of the non-finite entries differ'
    assert not np.isfinite(x[2, list(rows)]).any()
    assert np.isfinite(clean).all()
    h.close()


# ---------------------------------------------------------------------------------------------------- rlh_bdiag_solve
BDIAG_N = [1, 2, 3, 255, 256, 257, 1003]
BDIAG_M = [1, 7, 300]


def bdiag_shift(n):
    """2 x 2 pivots at both ends, back to back (rows 0-1 and 2-3), across the end of a workgroup (rows 255-256) and
    here and there in between."""
    s = np.zeros(n, dtype=np.int32)
    rng = np.random.default_rng(n)
    starts = [0, 2, n - 2, 255] + [int(v) for v in rng.choice(max(n - 1, 1), n // 9, replace=False)]
    if n == 3:
        starts = [1]
    for i in starts:
        if 0 <= i and i + 1 < n and s[i] == 0 and s[i + 1] == 0:
            s[i], s[i + 1] = 1, -1
    return s


def bdiag(key, n, m, padded):
    from raleigh_amd import _lib
    L = _lib.lib()
    u, c = unit_roundoff(key), cfac(key)
    shift = bdiag_shift(n)
    if n >= 2:
        assert shift[0] == 1 or n == 3
        assert shift[n - 1] == -1
    if n >= 256:
        assert shift[2] == 1 and (n == 256 or shift[255] == 1 or shift[254] == 1)
    coef = _pool(DT[key], 2 * n, 29).reshape(n, 2).copy()
    coef[shift == 0, 1] = np.nan
    ld = n + 5 if padded else n
    hx = _pool(DT[key], (m + 2) * ld, 31).reshape(m + 2, ld).copy()
    dx, dc, ds = _device(hx), _device(coef), _device(shift)
    es = hx.itemsize
    _lib.check(L.rlh_bdiag_solve(_lib.dtype_code(DT[key]), n, dc.ptr, ds.ptr, m, dx.ptr + ld * es, ld))
    _lib.check(L.rlh_sync())
    got = _fetch(dx, hx)
    win = got[1:m + 1, :n].copy()
    got[1:m + 1, :n] = hx[1:m + 1, :n]
    what = '[bdiag %s n=%d m=%d ld=%d]' % (key, n, m, ld)
    assert same_bytes(got, hx), 'guard columns or padding rows modified ' + what
    old = hx[1:m + 1, :n].astype(LONG[key])
    c0 = coef[:, 0].astype(LONG[key])
    c1 = np.where(shift != 0, coef[:, 1], 0).astype(LONG[key])
    other = old[:, np.arange(n) + shift]
    want = c0 * old + c1 * other
    bound = 3 * c * u * (np.abs(c0) * np.abs(old) + np.abs(c1) * np.abs(other))
    err = np.abs(win.astype(LONG[key]) - want)
    ok = err <= bound
    if not np.all(ok):
        j, i = np.argwhere(~ok)[0]
        raise AssertionError('(column %d, row %d, shift %d): error %.3e above the bound %.3e %s'
                             % (j, i, shift[i], err[j, i], bound[j, i], what))
    note_ratio('bdiag', key, '-', np.max(err / bound))


def bdiag_refusals():
    from raleigh_amd import _lib
    L = _lib.lib()
    n, m = 9, 3
    coef = _pool(np.float64, 2 * n, 1).copy()
    shift = np.zeros(n, dtype=np.int32)
    hx = _pool(np.float64, m * n, 2).copy()
    dx, dc, ds = _device(hx), _device(coef), _device(shift)
    for args, text in (((1, n, None, ds.ptr, m, dx.ptr, n), 'bad arguments'), ((1, n, dc.ptr, ds.ptr, m, dx.ptr, n - 1), 'bad arguments'),
                       ((1, n, dc.ptr, ds.ptr, 65536, dx.ptr, n), 'bad sizes')):
        assert L.rlh_bdiag_solve(*args) != 0
        msg = L.rlh_last_error()
        assert text in (msg.decode() if isinstance(msg, bytes) else str(msg))
        _lib.check(L.rlh_sync())
        assert same_bytes(_fetch(dx, hx), hx)
    for nn, mm in ((0, m), (n, 0)):
        _lib.check(L.rlh_bdiag_solve(1, nn, dc.ptr, ds.ptr, mm, dx.ptr, n))
    _lib.check(L.rlh_sync())
    assert same_bytes(_fetch(dx, hx), hx)
