"""tests/fake_fsai_values.py's stand-in library plus the three entry points of prefiltration (rlh_fsthreshold_create,
rlh_fsthreshold_create_device, rlh_fsthreshold_info) in NumPy, with the checks, their order and the messages of the real
library: TEST INFRASTRUCTURE ONLY.  "Device" pointers are host addresses.

A thresholded build is the stand-in's own build (`_fsai_build`: the checks, the level pattern, enrichment when steps > 0,
one solve per row on the FULL matrix, post-filtration when drop > 0) with one thing replaced: the level pattern is formed
(by the same `fake_fsai.level_pattern`) on the strong lower structure, the rule of include/rlhip.h evaluated on the stored
values -- entry (i, j), j < i, is strong iff |a_ji|^2 >= (tau^2 a_ii) a_jj in double, a_ji the partner above the
diagonal, a comparison with a NaN false, the diagonal always a member."""

import ctypes

import numpy as np

from fake_lib import _DT, _addr, _flat
import fake_csr_input
import fake_fsai
import fake_fsai_values
from fake_fsai import as_device  # noqa: F401


def strong_lower(n, ip, ix, va, tau):
    """The strong lower structure of a canonical CSR matrix as (indptr, indices) -- per row the strong columns j < i
    ascending, then the stored diagonal -- and the number of weak entries below the diagonal."""
    wide = np.complex128 if va.dtype.kind == 'c' else np.float64
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


class FakeFsaiThresholdLib(fake_fsai_values.FakeFsaiValuesLib):

    def _threshold_args(self, name, ph, code, n, indptr, max_row, levels, steps, step_size, drop, prefilter):
        """The checks of the other entry points in their order, drop (checked unless it is 0) and prefilter between step_size
        and indptr.  steps == 0: no enrichment, step_size is not looked at."""
        if ph is None:
            self._fail(name + ': null handle pointer')
            return None
        more = dict(levels=levels) if steps == 0 else dict(levels=levels, steps=steps, step_size=step_size)
        if drop != 0.0:
            more['drop'] = drop
        if self._fsai_args(name, ph, code, n, 1, max_row, **more):
            return None
        if not 0.0 < prefilter < 1.0:
            self._fail(name + ': prefilter must lie in (0, 1), got %g' % prefilter)
            return None
        if not _addr(indptr):
            self._fail(name + ': null indptr')
            return None
        return more

    def _threshold_build(self, name, ph, code, n, ip, ix, va, max_row, more, prefilter):
        weak = 0
        if n == 0 or fake_csr_input.message(name + ': ', ip, ix, n):         # (the build itself reports it)
            rc = self._fsai_build(name, ph, code, n, ip, ix, va, max_row, **more)
        else:
            sip, six, weak = strong_lower(n, ip, ix, va, prefilter)
            plain = fake_fsai.level_pattern
            fake_fsai.level_pattern = lambda n_, ip_, ix_, max_row_, levels_: plain(n_, sip, six, max_row_, levels_)
            try:
                rc = self._fsai_build(name, ph, code, n, ip, ix, va, max_row, **more)
            finally:
                fake_fsai.level_pattern = plain
        if rc:
            return rc
        f = self._fsai[ph._obj.value]
        f.prefilter, f.weak = float(prefilter), weak
        return 0

    def rlh_fsthreshold_create_device(self, ph, code, n, index_bits, indptr, indices, values, max_row, levels, steps, step_size,
                                      drop, prefilter):
        self._count('fsthreshold_create_device')
        name = 'rlh_fsthreshold_create_device'
        more = self._threshold_args(name, ph, code, n, indptr, max_row, levels, steps, step_size, drop, prefilter)
        if more is None:
            return 1
        if index_bits not in (32, 64):
            return self._fail(name + ': index_bits must be 32 or 64, got %d' % index_bits)
        it = np.int32 if index_bits == 32 else np.int64
        ip = _flat(indptr, it, n + 1).astype(np.int64)
        nnz = max(int(ip[-1]), 0)
        return self._threshold_build(name, ph, code, n, ip, _flat(indices, it, nnz).astype(np.int64),
                                     _flat(values, _DT[code], nnz).copy(), max_row, more, prefilter)

    def rlh_fsthreshold_create(self, ph, code, n, indptr, indices, values, max_row, levels, steps, step_size, drop, prefilter):
        self._count('fsthreshold_create')
        name = 'rlh_fsthreshold_create'
        more = self._threshold_args(name, ph, code, n, indptr, max_row, levels, steps, step_size, drop, prefilter)
        if more is None:
            return 1
        ip = _flat(indptr, np.int64, n + 1).copy()
        if msg := fake_csr_input.indptr_message(name + ': ', ip):          # (what decides how much is uploaded)
            return self._fail(msg)
        nnz = int(ip[-1])
        if nnz and not (_addr(indices) and _addr(values)):
            return self._fail(name + ': null indices or values')
        return self._threshold_build(name, ph, code, n, ip, _flat(indices, np.int32, nnz).astype(np.int64),
                                     _flat(values, _DT[code], nnz).copy(), max_row, more, prefilter)

    def rlh_fsthreshold_info(self, h, prefilter, weak_entries):
        if not _addr(h) or prefilter is None or weak_entries is None:
            return self._fail('rlh_fsthreshold_info: null handle or output')
        f = self._fsai[_addr(h)]
        ctypes.cast(prefilter, ctypes.POINTER(ctypes.c_double))[0] = getattr(f, 'prefilter', 0.0)
        ctypes.cast(weak_entries, ctypes.POINTER(ctypes.c_int64))[0] = getattr(f, 'weak', 0)
        return 0


def install():
    from raleigh_amd import _lib
    fake = FakeFsaiThresholdLib()
    _lib.set_library(fake)
    return fake
