"""tests/fake_fsai.py's stand-in library plus rlh_fsai_create_levels_device, rlh_fsai_create_levels and rlh_fsai_levels:
TEST INFRASTRUCTURE ONLY.  The level pattern is formed from its definition (L(i): the stored columns j <= i of row i;
P_1 = L, P_{l+1}(i) the union of L(j) over j in P_l(i); the max_row largest are kept after every level, a row counts as
truncated when any level overflows); the rows are then solved by the parent's code, which is given the matrix with
explicit zeros on that pattern (a stored zero and a missing entry are the same to the gather)."""

import ctypes

import numpy as np

from fake_lib import _DT, _addr, _flat
import fake_fsai
from fake_fsai import as_device  # noqa: F401


def level_pattern(n, ip, ix, max_row, levels):
    """Per row the (at most max_row, the largest) columns of P_levels ascending, and the number of rows whose full
    pattern has more."""
    low = []
    for i in range(n):
        c = ix[ip[i]:ip[i + 1]]
        low.append(np.asarray(c[c <= i], dtype=np.int64))
    over = np.array([len(c) > max_row for c in low])
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


class FakeFsaiLevelsLib(fake_fsai.FakeFsaiLib):

    def __init__(self):
        super().__init__()
        self._levels = {}
        self._want = 1              # the levels of the build in progress

    def _fsai_build(self, name, ph, code, n, ip, ix, va, max_row):
        levels = self._want
        rc = super()._fsai_build(name, ph, code, n, ip, ix, va, max_row)        # the checks, on the arrays as they came
        if rc or levels == 1:
            if not rc:
                self._levels[ph._obj.value] = 1
            return rc
        self._fsai.pop(ph._obj.value, None)
        ph._obj.value = None
        pat, truncated = level_pattern(n, ip, ix, max_row, levels)
        # the matrix plus explicit zeros on the pattern and its mirror image
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ip))
        pr = np.repeat(np.arange(n, dtype=np.int64), [len(p) for p in pat])
        pc = np.concatenate(pat)
        key = np.unique(np.concatenate([rows * n + ix, pr * n + pc, pc * n + pr]))
        data = np.zeros(key.size, dtype=va.dtype)
        data[np.searchsorted(key, rows * n + ix)] = va
        ip2 = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(key // n, minlength=n), out=ip2[1:])
        rc = super()._fsai_build(name, ph, code, n, ip2, key % n, data, max_row)
        if rc:
            return rc
        h = ph._obj.value
        self._fsai[h].truncated = truncated
        self._levels[h] = levels
        return 0

    def _levels_args(self, name, ph, code, n, indptr, max_row, levels):
        ph._obj.value = None
        if code not in _DT:
            return self._fail(name + ': unknown dtype %d' % code)
        if not 0 <= n < 2 ** 31 - 1:
            return self._fail(name + ': the size must lie in [0, 2^31 - 1)')
        if not 1 <= max_row <= 64:
            return self._fail(name + ': max_row must lie in [1, 64], got %d' % max_row)
        if not 1 <= levels <= 8:
            return self._fail(name + ': levels must lie in [1, 8], got %d' % levels)
        if not _addr(indptr):
            return self._fail(name + ': null indptr')
        return 0

    def _with_levels(self, levels, *args):
        self._want = levels
        try:
            return self._fsai_build(*args)
        finally:
            self._want = 1

    def rlh_fsai_create_levels_device(self, ph, code, n, index_bits, indptr, indices, values, max_row, levels):
        self._count('fsai_create_levels_device')
        name = 'rlh_fsai_create_levels_device'
        if self._levels_args(name, ph, code, n, indptr, max_row, levels):
            return 1
        if index_bits not in (32, 64):
            return self._fail(name + ': index_bits must be 32 or 64, got %d' % index_bits)
        it = np.int32 if index_bits == 32 else np.int64
        ip = _flat(indptr, it, n + 1).astype(np.int64)
        nnz = max(int(ip[-1]), 0)
        return self._with_levels(levels, name, ph, code, n, ip, _flat(indices, it, nnz).astype(np.int64),
                                 _flat(values, _DT[code], nnz).copy(), max_row)

    def rlh_fsai_create_levels(self, ph, code, n, indptr, indices, values, max_row, levels):
        self._count('fsai_create_levels')
        name = 'rlh_fsai_create_levels'
        if self._levels_args(name, ph, code, n, indptr, max_row, levels):
            return 1
        ip = _flat(indptr, np.int64, n + 1).copy()
        nnz = max(int(ip[-1]), 0)
        return self._with_levels(levels, name, ph, code, n, ip, _flat(indices, np.int32, nnz).astype(np.int64),
                                 _flat(values, _DT[code], nnz).copy(), max_row)

    def rlh_fsai_levels(self, h, levels):
        if not _addr(h) or levels is None:
            return self._fail('rlh_fsai_levels: null handle or output')
        ctypes.cast(levels, ctypes.POINTER(ctypes.c_int))[0] = self._levels[_addr(h)]
        return 0

    def rlh_fsai_destroy(self, h):
        self._levels.pop(_addr(h), None)
        return super().rlh_fsai_destroy(h)


def install():
    from raleigh_amd import _lib
    fake = FakeFsaiLevelsLib()
    _lib.set_library(fake)
    return fake
