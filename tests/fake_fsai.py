"""tests/fake_device_operator.py's stand-in library plus every rlh_fsai_* entry point (the factorised sparse
approximate inverse) in NumPy / SciPy, with the checks, their order and the messages of the real library: TEST
INFRASTRUCTURE ONLY.  "Device" pointers are host addresses.

One build path (`_fsai_build`) serves the six create calls.  The pattern is formed from its definition: the level
pattern (`level_pattern`: L(i) the stored columns j <= i of row i; P_1 = L, P_{l+1}(i) the union of L(j) over j in
P_l(i); the max_row largest are kept after every level, a row counts as truncated when any level overflows), then for
an adaptive build `steps` times per row (`enrich_row`): solve on the pattern, score the stored neighbours below the
diagonal that are not members, take the best.  Every row is then solved once on its pattern by `solve_row`
(numpy.linalg in double), on the block of the Hermitian matrix that the upper triangle defines: a stored zero and a
missing entry are the same block, so a level-1 build of a padded matrix and a wider build of the original give the
same bits."""

import ctypes

import numpy as np
import scipy.sparse as sp

from fake_lib import _DT, _addr, _block, _flat
import fake_csr_input
import fake_device_operator
from fake_device_operator import as_device  # noqa: F401


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
    pattern has more."""
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


class _Fsai:
    def __init__(self, g, code, truncated, levels, steps, step_size):
        self.g, self.gh, self.code, self.truncated = g, sp.csr_matrix(g.conj().T), code, truncated
        self.levels, self.steps, self.step_size = levels, steps, step_size


class FakeFsaiLib(fake_device_operator.FakeDeviceOperatorLib):

    def __init__(self):
        super().__init__()
        self._fsai = {}

    def _fsai_build(self, name, ph, code, n, ip, ix, va, max_row, levels=1, steps=0, step_size=0):
        # ---- the checks, on the arrays as they came
        if msg := fake_csr_input.message(name + ': ', ip, ix, n):
            return self._fail(msg)
        rows = np.repeat(np.arange(n), np.diff(ip))
        stored = set(zip(rows.tolist(), ix.tolist()))
        for i in range(n):
            if (i, i) not in stored:
                return self._fail(name + ': row %d does not store its diagonal entry' % i)
        for i, j in zip(rows.tolist(), ix.tolist()):
            if j < i and (j, i) not in stored:
                return self._fail(name + ': the stored structure is not symmetric: entry (%d, %d) has no partner (%d, %d); '
                                  'the device build creates no entries' % (i, j, j, i))
        wide = np.complex128 if np.dtype(_DT[code]).kind == 'c' else np.float64
        upper = rows <= ix                       # the upper triangle defines the matrix: nothing below it is read
        u = sp.csr_matrix((va[upper].astype(wide), (rows[upper], ix[upper])), shape=(n, n))
        full = sp.csr_matrix(u + sp.triu(u, k=1).conj().T)
        dense = full.toarray() if n <= 4096 or steps else None
        # ---- the pattern: its definition (include/rlhip.h), level by level and then step by step
        pat, truncated = level_pattern(n, ip, ix, max_row, levels)
        gp, gi, gv = [0], [], []
        try:
            if steps:
                diag, held = dense.diagonal().real, [False] * n
                for i in range(n):
                    pat[i], held[i] = enrich_row(i, pat[i], dense, diag, ip, ix, max_row, steps, step_size)
                truncated = sum(held)
            # ---- one solve per row on that pattern, whatever kind of build asked for it
            for i, p in enumerate(pat):
                g = solve_row(i, dense[np.ix_(p, p)] if dense is not None else full[p][:, p].toarray())
                gi.extend(p.tolist())
                gv.extend(g.tolist())
                gp.append(len(gi))
        except _NotPd as e:
            return self._fail(name + ': local block of row %d is not positive definite' % e.args[0])
        g = sp.csr_matrix((np.array(gv, dtype=wide).astype(_DT[code]), np.array(gi, dtype=np.int32),
                           np.array(gp, dtype=np.int64)), shape=(n, n))
        h = self._next_handle
        self._next_handle += 1
        self._fsai[h] = _Fsai(g, code, truncated, levels, steps, step_size)
        ph._obj.value = h
        return 0

    def _fsai_args(self, name, ph, code, n, indptr, max_row, levels=None, steps=None, step_size=None):
        """The real library's checks in its order; None: the entry point has no such argument."""
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
        if not _addr(indptr):
            return self._fail(name + ': null indptr')
        return 0

    def _create_device(self, entry, ph, code, n, index_bits, indptr, indices, values, max_row, **more):
        self._count('fsai_create%s_device' % entry)
        name = 'rlh_fsai_create%s_device' % entry
        if self._fsai_args(name, ph, code, n, indptr, max_row, **more):
            return 1
        if index_bits not in (32, 64):
            return self._fail(name + ': index_bits must be 32 or 64, got %d' % index_bits)
        it = np.int32 if index_bits == 32 else np.int64
        ip = _flat(indptr, it, n + 1).astype(np.int64)
        nnz = max(int(ip[-1]), 0)
        return self._fsai_build(name, ph, code, n, ip, _flat(indices, it, nnz).astype(np.int64),
                                _flat(values, _DT[code], nnz).copy(), max_row, **more)

    def _create_host(self, entry, ph, code, n, indptr, indices, values, max_row, **more):
        self._count('fsai_create' + entry)
        name = 'rlh_fsai_create' + entry
        if self._fsai_args(name, ph, code, n, indptr, max_row, **more):
            return 1
        ip = _flat(indptr, np.int64, n + 1).copy()
        nnz = max(int(ip[-1]), 0)
        return self._fsai_build(name, ph, code, n, ip, _flat(indices, np.int32, nnz).astype(np.int64),
                                _flat(values, _DT[code], nnz).copy(), max_row, **more)

    def rlh_fsai_create_device(self, ph, code, n, index_bits, indptr, indices, values, max_row):
        return self._create_device('', ph, code, n, index_bits, indptr, indices, values, max_row)

    def rlh_fsai_create(self, ph, code, n, indptr, indices, values, max_row):
        return self._create_host('', ph, code, n, indptr, indices, values, max_row)

    def rlh_fsai_create_levels_device(self, ph, code, n, index_bits, indptr, indices, values, max_row, levels):
        return self._create_device('_levels', ph, code, n, index_bits, indptr, indices, values, max_row, levels=levels)

    def rlh_fsai_create_levels(self, ph, code, n, indptr, indices, values, max_row, levels):
        return self._create_host('_levels', ph, code, n, indptr, indices, values, max_row, levels=levels)

    def rlh_fsai_create_adaptive_device(self, ph, code, n, index_bits, indptr, indices, values, max_row, levels, steps,
                                        step_size):
        return self._create_device('_adaptive', ph, code, n, index_bits, indptr, indices, values, max_row, levels=levels,
                                   steps=steps, step_size=step_size)

    def rlh_fsai_create_adaptive(self, ph, code, n, indptr, indices, values, max_row, levels, steps, step_size):
        return self._create_host('_adaptive', ph, code, n, indptr, indices, values, max_row, levels=levels, steps=steps,
                                 step_size=step_size)

    def rlh_fsai_levels(self, h, levels):
        if not _addr(h) or levels is None:
            return self._fail('rlh_fsai_levels: null handle or output')
        ctypes.cast(levels, ctypes.POINTER(ctypes.c_int))[0] = self._fsai[_addr(h)].levels
        return 0

    def rlh_fsai_adaptive(self, h, steps, step_size):
        if not _addr(h) or steps is None or step_size is None:
            return self._fail('rlh_fsai_adaptive: null handle or output')
        f = self._fsai[_addr(h)]
        ctypes.cast(steps, ctypes.POINTER(ctypes.c_int))[0] = f.steps
        ctypes.cast(step_size, ctypes.POINTER(ctypes.c_int))[0] = f.step_size
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
            if p is not None:
                ctypes.cast(p, ctypes.POINTER(ctypes.c_int64))[0] = v
        if seconds is not None:
            ctypes.cast(seconds, ctypes.POINTER(ctypes.c_double))[0] = 0.0
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
