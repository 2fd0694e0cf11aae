"""tests/fake_device_operator.py's stand-in library plus the approximate inverse (the factorised sparse approximate
inverse T = G^H G) in NumPy / SciPy, with the checks, their order and the messages of the real library: TEST
INFRASTRUCTURE ONLY.  "Device" pointers are host addresses.  Laid out like the library: this module is what
csrc/fsai.hip exports (every rlh_fsai_*, rlh_fsfilter_* and rlh_fsthreshold_* entry point, rlh_fsvalues_update* and
rlh_fsvalues_info), tests/fake_fsai_apply.py what csrc/fsai_apply.hip exports; `install()` installs the one class.

One build (`_build`) serves the ten create calls; an entry point passes the arguments it has, and those are the ones
that are checked (`_check_create`).  The pattern is formed from its definition: the level pattern (`level_pattern`:
L(i) the stored columns j <= i of row i; P_1 = L, P_{l+1}(i) the union of L(j) over j in P_l(i); the max_row largest
are kept after every level, a row counts as truncated when any level overflows) -- of A's own structure, or with
prefilter of the strong lower structure (`strong_lower`: entry (i, j), j < i, is strong iff |a_ji|^2 >= (tau^2 a_ii)
a_jj in double, a_ji the partner above the diagonal, a comparison with a NaN false, the diagonal always a member) --
then for an adaptive build `steps` times per row (`enrich_row`): solve on the pattern, score the stored neighbours below
the diagonal that are not members, take the best.  The numeric phase (`_solve_rows`) then solves every row once on its
pattern by `solve_row` (numpy.linalg in double) on the block of the Hermitian matrix that the upper triangle defines
(`_hermitian`), and rounds to the storage type: a stored zero and a missing entry are the same block, so a level-1
build of a padded matrix and a wider build of the original give the same bits.  With drop the rule of include/rlhip.h
is applied to the stored values (`kept_mask`: entry (i, j), j < i, stays iff |g_ij|^2 a_jj >= drop^2 g_ii^2 a_ii in
double, the diagonal always) and the numeric phase runs once more on the columns that are left.  An update of the
values is the checks on the new arrays without the partner check and the numeric phase on the pattern the handle keeps;
nothing is committed before every row has succeeded."""

import ctypes

import numpy as np
import scipy.sparse as sp

from fake_lib import _DT, _addr, _block, _flat
import fake_csr_input
import fake_device_operator
from fake_device_operator import as_device  # noqa: F401
from fake_fsai_apply import FakeFsaiApplyMixin, put, wide_type


def rsqrt_rounded(d):
    """d^(-1/2) correctly rounded to double: the longdouble value rounded, then moved to a neighbour where the exact
    comparison d m^2 <> 1 at the midpoint m says so (rounding twice, 64 then 53 bits, misses about one value in 2^11)."""
    from fractions import Fraction
    g = float(1 / np.sqrt(np.longdouble(d)))
    for _ in range(2):
        up, down = float(np.nextafter(g, np.inf)), float(np.nextafter(g, 0.0))
        if Fraction(d) * ((Fraction(g) + Fraction(up)) / 2) ** 2 < 1:
            g = up
        elif Fraction(d) * ((Fraction(g) + Fraction(down)) / 2) ** 2 > 1:
            g = down
        else:
            break
    return g


def level_pattern(n, ip, ix, max_row, levels):
    """Per row the (at most max_row, the largest) columns of P_levels ascending, and the number of rows whose full
    pattern has more.  ip, ix: the structure the pattern is the power of."""
    low = []
    for i in range(n):
        c = ix[ip[i]:ip[i + 1]]
        low.append(np.asarray(c[c <= i], dtype=np.int64))
    over = np.array([len(c) > max_row for c in low], dtype=bool)
    pat = [c[-max_row:] for c in low]
    for _ in range(levels - 1):
        nxt = []
        for i in range(n):
            u = np.unique(np.concatenate([low[j] for j in pat[i]]))
            if len(u) > max_row:
                over[i] = True
                u = u[-max_row:]
            nxt.append(u)
        pat = nxt
    return pat, int(over.sum())


def strong_lower(n, ip, ix, va, tau):
    """The strong lower structure of a canonical CSR matrix as (indptr, indices) -- per row the strong columns j < i
    ascending, then the stored diagonal -- and the number of weak entries below the diagonal."""
    wide = wide_type(va.dtype)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ip))
    key = rows * n + ix                                         # ascending: rows in order, columns ascending within each

    def find(r, c):
        want = r * n + c
        at = np.minimum(np.searchsorted(key, want), max(key.size - 1, 0))
        return at, (key[at] == want if key.size else np.zeros(want.shape, dtype=bool))
    at, has = find(np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64))
    diag = np.where(has, va[at].astype(wide).real, 0.0).astype(np.float64)
    lower = ix < rows
    at, has = find(ix, rows)                                    # the partner (j, i) of the entry (i, j)
    v = va[at].astype(wide)
    with np.errstate(all='ignore'):
        size2 = v.real * v.real + v.imag * v.imag
        strong = lower & has & (size2 >= ((tau * tau) * diag[rows]) * diag[ix])
    member = strong | (ix == rows)
    sip = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows[member], minlength=n), out=sip[1:])
    return sip, ix[member], int(np.sum(lower & ~strong))


class _NotPd(Exception):
    pass


def solve_row(i, s):
    """Row i of G from its block s = A[P, P]: g with s g^H = e_k / g_kk and g_kk > 0, in the precision of s."""
    try:
        np.linalg.cholesky(s)
    except np.linalg.LinAlgError:
        raise _NotPd(i)
    k = s.shape[0]
    if k == 1:
        return np.array([rsqrt_rounded(float(s[0, 0].real))], dtype=s.dtype)
    e = np.zeros(k, dtype=s.dtype)
    e[-1] = 1
    y = np.linalg.solve(s, e)
    g = np.conj(y) / np.sqrt(y[-1].real)
    g[-1] = g[-1].real
    return g


def enrich_row(i, pat, full, diag, ip, ix, max_row, steps, step_size):
    """The enriched pattern of row i (ascending) and whether max_row held the row back."""
    pat = np.asarray(pat, dtype=np.int64)
    limited = False
    for _ in range(steps):
        if len(pat) >= max_row:
            limited = True
            break
        s = full[np.ix_(pat, pat)]
        try:
            np.linalg.cholesky(s)
        except np.linalg.LinAlgError:
            raise _NotPd(i)
        e = np.zeros(len(pat), dtype=full.dtype)
        e[-1] = 1
        g = np.conj(np.linalg.solve(s, e))
        cand = np.unique(np.concatenate([ix[ip[p]:ip[p + 1]] for p in pat]))
        cand = np.setdiff1d(cand[cand < i], pat)
        if not cand.size:
            break
        r = np.zeros(cand.size, dtype=full.dtype)
        for t, p in enumerate(pat):                         # ascending p
            r = r + g[t] * full[p, cand]
        with np.errstate(divide='ignore', invalid='ignore'):
            score = np.abs(r) ** 2 / diag[cand]
        good = np.flatnonzero(np.isfinite(score) & (score > 0))
        room = max_row - len(pat)
        if room < min(step_size, good.size):
            limited = True
        order = good[np.lexsort((-cand[good], -score[good]))]        # by score, equal scores the larger column first
        took = cand[order[:min(step_size, room)]]
        if not took.size:
            break
        pat = np.sort(np.concatenate([pat, took]))
    return pat, limited


def kept_mask(g, cols, diag, drop):
    """The entries of one stored row (values g, columns cols ascending, the diagonal last) that stay."""
    g = g.astype(wide_type(g.dtype))
    gii = float(g[-1].real)
    bar = ((drop * drop) * (gii * gii)) * diag[cols[-1]]
    keep = (g.real * g.real + g.imag * g.imag) * diag[cols] >= bar
    keep[-1] = True
    return keep


def _hermitian(n, rows, ix, va):
    """The Hermitian matrix that the upper triangle defines, as CSR in float64 / complex128: nothing below the
    diagonal is read, a position the upper triangle does not store is zero.  rows: the rows of the entries."""
    upper = rows <= ix
    u = sp.csr_matrix((va[upper].astype(wide_type(va.dtype)), (rows[upper], ix[upper])), shape=(n, n))
    return sp.csr_matrix(u + sp.triu(u, k=1).conj().T)


def _rows_of(g):
    """The column patterns of a CSR matrix, row by row."""
    return [g.indices[g.indptr[i]:g.indptr[i + 1]].astype(np.int64) for i in range(g.shape[0])]


def _solve_rows(patterns, full, dense, code):
    """The numeric phase: every row solved on its pattern, rounded to the storage type, assembled as G."""
    n = len(patterns)
    gp, gi, gv = [0], [], []
    for i, p in enumerate(patterns):
        g = solve_row(i, dense[np.ix_(p, p)] if dense is not None else full[p][:, p].toarray())
        gi.extend(p.tolist())
        gv.extend(g.tolist())
        gp.append(len(gi))
    return sp.csr_matrix((np.array(gv, dtype=full.dtype).astype(_DT[code]), np.array(gi, dtype=np.int32),
                          np.array(gp, dtype=np.int64)), shape=(n, n))


class _Fsai:
    """The handle: G, G^H and what the info calls report."""

    def __init__(self, g, code, truncated, levels, steps, step_size):
        self.code, self.truncated = code, truncated
        self.levels, self.steps, self.step_size = levels, steps, step_size
        self.drop, self.removed, self.prefilter, self.weak, self.updates = 0.0, 0, 0.0, 0, 0
        self.set_g(g)

    def set_g(self, g):
        self.g, self.gh = g, sp.csr_matrix(g.conj().T)


class FakeFsaiLib(FakeFsaiApplyMixin, fake_device_operator.FakeDeviceOperatorLib):

    def __init__(self):
        super().__init__()
        self._fsai = {}

    # ---------------------------------------------------------------- the three arrays of an entry point
    def _host_arrays(self, name, code, n, indptr, indices, values):
        """(ip, ix, va, cap) of host arrays; None with the message set: what decides how much is read is checked here."""
        ip = _flat(indptr, np.int64, n + 1).copy()
        if msg := fake_csr_input.indptr_message(name + ': ', ip):
            self._fail(msg)
            return None
        nnz = int(ip[-1])
        if nnz and not (_addr(indices) and _addr(values)):
            self._fail(name + ': null indices or values')
            return None
        return ip, _flat(indices, np.int32, nnz).astype(np.int64), _flat(values, _DT[code], nnz).copy(), None

    def _device_arrays(self, name, code, n, index_bits, indptr, indices, values):
        """(ip, ix, va, cap) of device arrays; cap: the entries the index and value arrays can hold (None: not known;
        0: one of them is null).  None with the message set for an index_bits that is neither 32 nor 64."""
        if index_bits not in (32, 64):
            self._fail(name + ': index_bits must be 32 or 64, got %d' % index_bits)
            return None
        if n == 0:                               # (as in the library: nothing is read)
            return np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=_DT[code]), None
        it = np.int32 if index_bits == 32 else np.int64
        ip = _flat(indptr, it, n + 1).astype(np.int64)
        if not _addr(indices) or not _addr(values):
            return ip, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=_DT[code]), 0
        nnz = max(int(ip[-1]), 0)
        return ip, _flat(indices, it, nnz).astype(np.int64), _flat(values, _DT[code], nnz).copy(), None

    # ---------------------------------------------------------------- the build
    def _check_create(self, name, ph, code, n, indptr, max_row, levels=None, steps=None, step_size=None, drop=None,
                      prefilter=None):
        """The real library's checks in its order; None: the entry point has no such argument, or leaves it unchecked."""
        if ph is None:
            return self._fail(name + ': null handle pointer')
        ph._obj.value = None
        if code not in _DT:
            return self._fail(name + ': unknown dtype %d' % code)
        if not 0 <= n < 2 ** 31 - 1:
            return self._fail(name + ': the size must lie in [0, 2^31 - 1)')
        if not 1 <= max_row <= 64:
            return self._fail(name + ': max_row must lie in [1, 64], got %d' % max_row)
        if levels is not None and not 1 <= levels <= 8:
            return self._fail(name + ': levels must lie in [1, 8], got %d' % levels)
        if steps is not None and not 1 <= steps <= 63:
            return self._fail(name + ': steps must lie in [1, 63], got %d' % steps)
        if step_size is not None and not 1 <= step_size <= 16:
            return self._fail(name + ': step_size must lie in [1, 16], got %d' % step_size)
        if drop is not None and not 0.0 < drop < 1.0:
            return self._fail(name + ': drop must lie in (0, 1), got %g' % drop)
        if prefilter is not None and not 0.0 < prefilter < 1.0:
            return self._fail(name + ': prefilter must lie in (0, 1), got %g' % prefilter)
        if not _addr(indptr):
            return self._fail(name + ': null indptr')
        return 0

    def _checked_matrix(self, name, code, n, ip, ix, va, cap, partners):
        """The checks on the arrays as they came -- canonical CSR, a stored diagonal in every row and (partners) the
        partner of every entry below the diagonal -- then the Hermitian matrix.  None with the message set."""
        if msg := fake_csr_input.message(name + ': ', ip, ix, n, cap):
            self._fail(msg)
            return None
        rows = np.repeat(np.arange(n), np.diff(ip))
        stored = set(zip(rows.tolist(), ix.tolist()))
        for i in range(n):
            if (i, i) not in stored:
                self._fail(name + ': row %d does not store its diagonal entry' % i)
                return None
        for i, j in zip(rows.tolist(), ix.tolist()) if partners else ():
            if j < i and (j, i) not in stored:
                self._fail(name + ': the stored structure is not symmetric: entry (%d, %d) has no partner (%d, %d); '
                           'the device build creates no entries' % (i, j, j, i))
                return None
        return _hermitian(n, rows, ix, va)

    def _build(self, name, ph, code, n, ip, ix, va, cap, max_row, levels=1, steps=None, step_size=None, drop=None,
               prefilter=None):
        steps, step_size = steps or 0, (step_size or 0) if steps else 0
        full = self._checked_matrix(name, code, n, ip, ix, va, cap, partners=True)
        if full is None:
            return 1
        dense = full.toarray() if n <= 4096 or steps else None
        diag = full.diagonal().real.astype(np.float64)
        # ---- the pattern: its definition (include/rlhip.h), level by level -- of A's structure or of the strong lower
        # structure -- and then step by step
        weak = 0
        if prefilter is not None and n:
            sip, six, weak = strong_lower(n, ip, ix, va, prefilter)
            pat, truncated = level_pattern(n, sip, six, max_row, levels)
        else:
            pat, truncated = level_pattern(n, ip, ix, max_row, levels)
        try:
            if steps:
                held = [False] * n
                for i in range(n):
                    pat[i], held[i] = enrich_row(i, pat[i], dense, diag, ip, ix, max_row, steps, step_size)
                truncated = sum(held)
            # ---- one solve per row on that pattern, whatever kind of build asked for it
            g = _solve_rows(pat, full, dense, code)
            f = _Fsai(g, code, truncated, levels, steps, step_size)
            if drop is not None:
                # ---- post-filtration on the stored values, and one more solve per row on what is left
                kept = [p[kept_mask(g.data[g.indptr[i]:g.indptr[i + 1]], p, diag, drop)] for i, p in enumerate(_rows_of(g))]
                f.set_g(_solve_rows(kept, full, dense, code))
                f.drop, f.removed = float(drop), int(g.nnz - f.g.nnz)
        except _NotPd as e:
            return self._fail(name + ': local block of row %d is not positive definite' % e.args[0])
        if prefilter is not None:
            f.prefilter, f.weak = float(prefilter), weak
        h = self._next_handle
        self._next_handle += 1
        self._fsai[h] = f
        ph._obj.value = h
        return 0

    def _create(self, name, ph, code, n, index_bits, indptr, indices, values, max_row, **more):
        """index_bits None: host arrays."""
        self._count(name[len('rlh_'):])
        if self._check_create(name, ph, code, n, indptr, max_row, **more):
            return 1
        arrays = (self._host_arrays(name, code, n, indptr, indices, values) if index_bits is None else
                  self._device_arrays(name, code, n, index_bits, indptr, indices, values))
        if arrays is None:
            return 1
        return self._build(name, ph, code, n, *arrays, max_row, **more)

    def rlh_fsai_create_device(self, ph, code, n, index_bits, indptr, indices, values, max_row):
        return self._create('rlh_fsai_create_device', ph, code, n, index_bits, indptr, indices, values, max_row)

    def rlh_fsai_create(self, ph, code, n, indptr, indices, values, max_row):
        return self._create('rlh_fsai_create', ph, code, n, None, indptr, indices, values, max_row)

    def rlh_fsai_create_levels_device(self, ph, code, n, index_bits, indptr, indices, values, max_row, levels):
        return self._create('rlh_fsai_create_levels_device', ph, code, n, index_bits, indptr, indices, values, max_row, levels=levels)

    def rlh_fsai_create_levels(self, ph, code, n, indptr, indices, values, max_row, levels):
        return self._create('rlh_fsai_create_levels', ph, code, n, None, indptr, indices, values, max_row, levels=levels)

    def rlh_fsai_create_adaptive_device(self, ph, code, n, index_bits, indptr, indices, values, max_row, levels, steps,
                                        step_size):
        return self._create('rlh_fsai_create_adaptive_device', ph, code, n, index_bits, indptr, indices, values, max_row,
                            levels=levels, steps=steps, step_size=step_size)

    def rlh_fsai_create_adaptive(self, ph, code, n, indptr, indices, values, max_row, levels, steps, step_size):
        return self._create('rlh_fsai_create_adaptive', ph, code, n, None, indptr, indices, values, max_row, levels=levels,
                            steps=steps, step_size=step_size)

    @staticmethod
    def _optional(levels, steps, step_size, **more):
        """steps == 0: no enrichment, step_size is not looked at."""
        return dict(levels=levels, **more) if steps == 0 else dict(levels=levels, steps=steps, step_size=step_size, **more)

    def rlh_fsfilter_create_device(self, ph, code, n, index_bits, indptr, indices, values, max_row, levels, steps, step_size,
                                   drop):
        return self._create('rlh_fsfilter_create_device', ph, code, n, index_bits, indptr, indices, values, max_row,
                            **self._optional(levels, steps, step_size, drop=drop))

    def rlh_fsfilter_create(self, ph, code, n, indptr, indices, values, max_row, levels, steps, step_size, drop):
        return self._create('rlh_fsfilter_create', ph, code, n, None, indptr, indices, values, max_row,
                            **self._optional(levels, steps, step_size, drop=drop))

    def rlh_fsthreshold_create_device(self, ph, code, n, index_bits, indptr, indices, values, max_row, levels, steps, step_size,
                                      drop, prefilter):
        """drop == 0: no post-filtration (anything else is checked as a drop)."""
        return self._create('rlh_fsthreshold_create_device', ph, code, n, index_bits, indptr, indices, values, max_row,
                            **self._optional(levels, steps, step_size, drop=None if drop == 0.0 else drop, prefilter=prefilter))

    def rlh_fsthreshold_create(self, ph, code, n, indptr, indices, values, max_row, levels, steps, step_size, drop, prefilter):
        return self._create('rlh_fsthreshold_create', ph, code, n, None, indptr, indices, values, max_row,
                            **self._optional(levels, steps, step_size, drop=None if drop == 0.0 else drop, prefilter=prefilter))

    # ---------------------------------------------------------------- new values on the kept pattern
    def _update(self, name, h, index_bits, indptr, indices, values):
        """index_bits None: host arrays."""
        self._count(name[len('rlh_'):])
        if not _addr(h):
            return self._fail(name + ': null handle')
        if not _addr(indptr):
            return self._fail(name + ': null indptr')
        f = self._fsai[_addr(h)]
        n = f.g.shape[0]
        arrays = (self._host_arrays(name, f.code, n, indptr, indices, values) if index_bits is None else
                  self._device_arrays(name, f.code, n, index_bits, indptr, indices, values))
        if arrays is None:
            return 1
        if n:                                    # (n == 0: a valid update that solves nothing)
            full = self._checked_matrix(name, f.code, n, *arrays, partners=False)
            if full is None:
                return 1
            try:
                g = _solve_rows(_rows_of(f.g), full, full.toarray() if n <= 4096 else None, f.code)
            except _NotPd as e:
                return self._fail(name + ': local block of row %d is not positive definite' % e.args[0])
            f.set_g(g)
        f.updates += 1
        return 0

    def rlh_fsvalues_update_device(self, h, index_bits, indptr, indices, values):
        return self._update('rlh_fsvalues_update_device', h, index_bits, indptr, indices, values)

    def rlh_fsvalues_update(self, h, indptr, indices, values):
        return self._update('rlh_fsvalues_update', h, None, indptr, indices, values)

    def rlh_fsvalues_info(self, h, updates, seconds):
        if not _addr(h):
            return self._fail('rlh_fsvalues_info: null handle')
        put(updates, ctypes.c_int64, self._fsai[_addr(h)].updates)
        put(seconds, ctypes.c_double, 0.0)
        return 0

    # ---------------------------------------------------------------- what a handle reports, its application, its end
    def rlh_fsai_levels(self, h, levels):
        if not _addr(h) or levels is None:
            return self._fail('rlh_fsai_levels: null handle or output')
        put(levels, ctypes.c_int, self._fsai[_addr(h)].levels)
        return 0

    def rlh_fsai_adaptive(self, h, steps, step_size):
        if not _addr(h) or steps is None or step_size is None:
            return self._fail('rlh_fsai_adaptive: null handle or output')
        f = self._fsai[_addr(h)]
        put(steps, ctypes.c_int, f.steps)
        put(step_size, ctypes.c_int, f.step_size)
        return 0

    def rlh_fsfilter_info(self, h, drop, removed):
        if not _addr(h) or drop is None or removed is None:
            return self._fail('rlh_fsfilter_info: null handle or output')
        f = self._fsai[_addr(h)]
        put(drop, ctypes.c_double, f.drop)
        put(removed, ctypes.c_int64, f.removed)
        return 0

    def rlh_fsthreshold_info(self, h, prefilter, weak_entries):
        if not _addr(h) or prefilter is None or weak_entries is None:
            return self._fail('rlh_fsthreshold_info: null handle or output')
        f = self._fsai[_addr(h)]
        put(prefilter, ctypes.c_double, f.prefilter)
        put(weak_entries, ctypes.c_int64, f.weak)
        return 0

    def rlh_fsai_destroy(self, h):
        self._fsai.pop(_addr(h), None)
        return 0

    def rlh_fsai_info(self, h, n, nnz, longest, truncated, nbytes, seconds):
        if not _addr(h):
            return self._fail('rlh_fsai_info: null handle')
        f = self._fsai[_addr(h)]
        es = np.dtype(_DT[f.code]).itemsize
        lens = np.diff(f.g.indptr)
        for p, v in ((n, f.g.shape[0]), (nnz, f.g.nnz), (longest, int(lens.max()) if lens.size else 0),
                     (truncated, f.truncated), (nbytes, 2 * f.g.nnz * (es + 4) + 16 * (f.g.shape[0] + 1))):
            put(p, ctypes.c_int64, v)
        put(seconds, ctypes.c_double, 0.0)
        return 0

    def rlh_fsai_get(self, h, indptr, indices, values):
        if not _addr(h):
            return self._fail('rlh_fsai_get: null handle')
        f = self._fsai[_addr(h)]
        n, nnz = f.g.shape[0], f.g.nnz
        _flat(indptr, np.int64, n + 1)[:] = f.g.indptr
        _flat(indices, np.int32, nnz)[:] = f.g.indices
        _flat(values, _DT[f.code], nnz)[:] = f.g.data
        return 0

    def rlh_fsai_apply(self, h, m, X, ldx, Y, ldy):
        self._count('fsai_apply')
        if not _addr(h):
            return self._fail('rlh_fsai_apply: null handle')
        f = self._fsai[_addr(h)]
        n = f.g.shape[0]
        if m < 0:
            return self._fail('rlh_fsai_apply: negative number of vectors')
        if m == 0 or n == 0:
            return 0
        if ldx < n or ldy < n:
            return self._fail('rlh_fsai_apply: Matrix and vectors dimensions incompatible')
        x = _block(X, f.code, n, m, ldx)
        w = np.asarray(f.g @ x.T).astype(_DT[f.code])
        _block(Y, f.code, n, m, ldy)[:, :] = np.asarray(f.gh @ w).T.astype(_DT[f.code])
        return 0


def install():
    from raleigh_amd import _lib
    fake = FakeFsaiLib()
    _lib.set_library(fake)
    return fake
