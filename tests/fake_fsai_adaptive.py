"""tests/fake_fsai_levels.py's stand-in library plus rlh_fsai_create_adaptive_device, rlh_fsai_create_adaptive and
rlh_fsai_adaptive: TEST INFRASTRUCTURE ONLY.  The pattern is formed from its definition (include/rlhip.h): the level
pattern, then per row `steps` times: solve on the pattern, score the stored neighbours below the diagonal that are not
members, take the best.  The rows are then solved by the parent's code, which is given the matrix with explicit zeros
on the final pattern and its mirror image, as tests/fake_fsai_levels.py does: every pattern holds the level-1 row (or,
where max_row cuts that, its max_row largest columns, which are then also the largest of the padded row)."""

import ctypes

import numpy as np
import scipy.sparse as sp

from fake_lib import _DT, _addr, _flat
import fake_fsai
import fake_fsai_levels
from fake_fsai_levels import as_device, level_pattern  # noqa: F401


class _NotPd(Exception):
    pass


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


class FakeFsaiAdaptiveLib(fake_fsai_levels.FakeFsaiLevelsLib):

    def __init__(self):
        super().__init__()
        self._adaptive = {}
        self._grow = None           # (steps, step_size) of the build in progress

    def _fsai_build(self, name, ph, code, n, ip, ix, va, max_row):
        if self._grow is None:
            return super()._fsai_build(name, ph, code, n, ip, ix, va, max_row)
        levels, (steps, step_size) = self._want, self._grow
        plain = fake_fsai.FakeFsaiLib._fsai_build
        rc = plain(self, name, ph, code, n, ip, ix, va, max_row)            # the checks, on the arrays as they came
        if rc:
            return rc
        self._fsai.pop(ph._obj.value, None)
        ph._obj.value = None
        pat, _ = level_pattern(n, ip, ix, max_row, levels)
        wide = np.complex128 if np.dtype(_DT[code]).kind == 'c' else np.float64
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ip))
        upper = rows <= ix                                   # nothing below the diagonal is read
        u = sp.csr_matrix((va[upper].astype(wide), (rows[upper], ix[upper])), shape=(n, n))
        full = (u + sp.triu(u, k=1).conj().T).toarray()
        diag = full.diagonal().real
        truncated = 0
        try:
            for i in range(n):
                pat[i], limited = enrich_row(i, pat[i], full, diag, ip, ix, max_row, steps, step_size)
                truncated += 1 if limited else 0
        except _NotPd as e:
            return self._fail(name + ': local block of row %d is not positive definite' % e.args[0])
        pr = np.repeat(np.arange(n, dtype=np.int64), [len(p) for p in pat])
        pc = np.concatenate(pat)
        key = np.unique(np.concatenate([rows * n + ix, pr * n + pc, pc * n + pr]))
        data = np.zeros(key.size, dtype=va.dtype)
        data[np.searchsorted(key, rows * n + ix)] = va
        ip2 = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(key // n, minlength=n), out=ip2[1:])
        rc = plain(self, name, ph, code, n, ip2, key % n, data, max_row)
        if rc:
            return rc
        h = ph._obj.value
        self._fsai[h].truncated = truncated
        self._levels[h] = levels
        self._adaptive[h] = (steps, step_size)
        return 0

    def _adaptive_args(self, name, ph, code, n, indptr, max_row, levels, steps, step_size):
        ph._obj.value = None
        if code not in _DT:
            return self._fail(name + ': unknown dtype %d' % code)
        if not 0 <= n < 2 ** 31 - 1:
            return self._fail(name + ': the size must lie in [0, 2^31 - 1)')
        if not 1 <= max_row <= 64:
            return self._fail(name + ': max_row must lie in [1, 64], got %d' % max_row)
        if not 1 <= levels <= 8:
            return self._fail(name + ': levels must lie in [1, 8], got %d' % levels)
        if not 1 <= steps <= 63:
            return self._fail(name + ': steps must lie in [1, 63], got %d' % steps)
        if not 1 <= step_size <= 16:
            return self._fail(name + ': step_size must lie in [1, 16], got %d' % step_size)
        if not _addr(indptr):
            return self._fail(name + ': null indptr')
        return 0

    def _with_growth(self, levels, steps, step_size, *args):
        self._grow = (steps, step_size)
        try:
            return self._with_levels(levels, *args)
        finally:
            self._grow = None

    def rlh_fsai_create_adaptive_device(self, ph, code, n, index_bits, indptr, indices, values, max_row, levels, steps,
                                        step_size):
        self._count('fsai_create_adaptive_device')
        name = 'rlh_fsai_create_adaptive_device'
        if self._adaptive_args(name, ph, code, n, indptr, max_row, levels, steps, step_size):
            return 1
        if index_bits not in (32, 64):
            return self._fail(name + ': index_bits must be 32 or 64, got %d' % index_bits)
        it = np.int32 if index_bits == 32 else np.int64
        ip = _flat(indptr, it, n + 1).astype(np.int64)
        nnz = max(int(ip[-1]), 0)
        return self._with_growth(levels, steps, step_size, name, ph, code, n, ip, _flat(indices, it, nnz).astype(np.int64),
                                 _flat(values, _DT[code], nnz).copy(), max_row)

    def rlh_fsai_create_adaptive(self, ph, code, n, indptr, indices, values, max_row, levels, steps, step_size):
        self._count('fsai_create_adaptive')
        name = 'rlh_fsai_create_adaptive'
        if self._adaptive_args(name, ph, code, n, indptr, max_row, levels, steps, step_size):
            return 1
        ip = _flat(indptr, np.int64, n + 1).copy()
        nnz = max(int(ip[-1]), 0)
        return self._with_growth(levels, steps, step_size, name, ph, code, n, ip, _flat(indices, np.int32, nnz).astype(np.int64),
                                 _flat(values, _DT[code], nnz).copy(), max_row)

    def rlh_fsai_adaptive(self, h, steps, step_size):
        if not _addr(h) or steps is None or step_size is None:
            return self._fail('rlh_fsai_adaptive: null handle or output')
        got = self._adaptive.get(_addr(h), (0, 0))
        ctypes.cast(steps, ctypes.POINTER(ctypes.c_int))[0] = got[0]
        ctypes.cast(step_size, ctypes.POINTER(ctypes.c_int))[0] = got[1]
        return 0

    def rlh_fsai_destroy(self, h):
        self._adaptive.pop(_addr(h), None)
        return super().rlh_fsai_destroy(h)


def install():
    from raleigh_amd import _lib
    fake = FakeFsaiAdaptiveLib()
    _lib.set_library(fake)
    return fake
