"""tests/fake_fsai_work.py's stand-in library plus the three entry points of post-filtration (rlh_fsfilter_create,
rlh_fsfilter_create_device, rlh_fsfilter_info) in NumPy, with the checks, their order and the messages of the real
library: TEST INFRASTRUCTURE ONLY.  "Device" pointers are host addresses.

A filtered build is the stand-in's own build (`_fsai_build`: level pattern, enrichment when steps > 0, one solve per row,
rounded to the storage type), then per row the rule of include/rlhip.h on the stored values -- entry (i, j), j < i,
stays iff |g_ij|^2 a_jj >= drop^2 g_ii^2 a_ii in double, the diagonal always -- and `solve_row` once more on the columns
that are left."""

import ctypes

import numpy as np
import scipy.sparse as sp

from fake_lib import _DT, _addr, _flat
import fake_fsai
import fake_fsai_work
from fake_fsai import as_device  # noqa: F401


def kept_mask(g, cols, diag, drop):
    """The entries of one stored row (values g, columns cols ascending, the diagonal last) that stay."""
    g = g.astype(np.complex128 if g.dtype.kind == 'c' else np.float64)
    gii = float(g[-1].real)
    bar = ((drop * drop) * (gii * gii)) * diag[cols[-1]]
    keep = (g.real * g.real + g.imag * g.imag) * diag[cols] >= bar
    keep[-1] = True
    return keep


class FakeFsaiFilterLib(fake_fsai_work.FakeFsaiWorkLib):

    def _fsai_args(self, name, ph, code, n, indptr, max_row, levels=None, steps=None, step_size=None, drop=None):
        """The checks of the other entry points in their order, drop (None: no such argument) between step_size and indptr."""
        if super()._fsai_args(name, ph, code, n, 1, max_row, levels=levels, steps=steps, step_size=step_size):
            return 1
        if drop is not None and not 0.0 < drop < 1.0:
            return self._fail(name + ': drop must lie in (0, 1), got %g' % drop)
        if not _addr(indptr):
            return self._fail(name + ': null indptr')
        return 0

    def _fsai_build(self, name, ph, code, n, ip, ix, va, max_row, levels=1, steps=0, step_size=0, drop=None):
        if steps is None:                                   # a filtered build without enrichment
            steps, step_size = 0, 0
        if super()._fsai_build(name, ph, code, n, ip, ix, va, max_row, levels=levels, steps=steps, step_size=step_size):
            return 1
        f = self._fsai[ph._obj.value]
        f.drop, f.removed = 0.0, 0
        if drop is None:
            return 0
        wide = np.complex128 if np.dtype(_DT[code]).kind == 'c' else np.float64
        rows = np.repeat(np.arange(n), np.diff(ip))
        upper = rows <= ix
        u = sp.csr_matrix((va[upper].astype(wide), (rows[upper], ix[upper])), shape=(n, n))
        full = sp.csr_matrix(u + sp.triu(u, k=1).conj().T)
        dense = full.toarray() if n <= 4096 else None
        diag = full.diagonal().real.astype(np.float64)
        g0 = f.g
        gp, gi, gv = [0], [], []
        for i in range(n):
            cols = g0.indices[g0.indptr[i]:g0.indptr[i + 1]].astype(np.int64)
            p = cols[kept_mask(g0.data[g0.indptr[i]:g0.indptr[i + 1]], cols, diag, drop)]
            g = fake_fsai.solve_row(i, dense[np.ix_(p, p)] if dense is not None else full[p][:, p].toarray())
            gi.extend(p.tolist())
            gv.extend(g.tolist())
            gp.append(len(gi))
        g = sp.csr_matrix((np.array(gv, dtype=wide).astype(_DT[code]), np.array(gi, dtype=np.int32),
                           np.array(gp, dtype=np.int64)), shape=(n, n))
        f.drop, f.removed = float(drop), int(g0.nnz - g.nnz)
        f.g, f.gh = g, sp.csr_matrix(g.conj().T)
        return 0

    @staticmethod
    def _filtered_args(levels, steps, step_size, drop):
        """steps == 0: no enrichment, step_size is not looked at."""
        if steps == 0:
            return dict(levels=levels, drop=drop)
        return dict(levels=levels, steps=steps, step_size=step_size, drop=drop)

    def rlh_fsfilter_create_device(self, ph, code, n, index_bits, indptr, indices, values, max_row, levels, steps, step_size,
                                   drop):
        self._count('fsfilter_create_device')
        name, more = 'rlh_fsfilter_create_device', self._filtered_args(levels, steps, step_size, drop)
        if self._fsai_args(name, ph, code, n, indptr, max_row, **more):
            return 1
        if index_bits not in (32, 64):
            return self._fail(name + ': index_bits must be 32 or 64, got %d' % index_bits)
        it = np.int32 if index_bits == 32 else np.int64
        ip = _flat(indptr, it, n + 1).astype(np.int64)
        nnz = max(int(ip[-1]), 0)
        return self._fsai_build(name, ph, code, n, ip, _flat(indices, it, nnz).astype(np.int64),
                                _flat(values, _DT[code], nnz).copy(), max_row, **more)

    def rlh_fsfilter_create(self, ph, code, n, indptr, indices, values, max_row, levels, steps, step_size, drop):
        self._count('fsfilter_create')
        name, more = 'rlh_fsfilter_create', self._filtered_args(levels, steps, step_size, drop)
        if self._fsai_args(name, ph, code, n, indptr, max_row, **more):
            return 1
        ip = _flat(indptr, np.int64, n + 1).copy()
        nnz = max(int(ip[-1]), 0)
        return self._fsai_build(name, ph, code, n, ip, _flat(indices, np.int32, nnz).astype(np.int64),
                                _flat(values, _DT[code], nnz).copy(), max_row, **more)

    def rlh_fsfilter_info(self, h, drop, removed):
        if not _addr(h) or drop is None or removed is None:
            return self._fail('rlh_fsfilter_info: null handle or output')
        f = self._fsai[_addr(h)]
        ctypes.cast(drop, ctypes.POINTER(ctypes.c_double))[0] = getattr(f, 'drop', 0.0)
        ctypes.cast(removed, ctypes.POINTER(ctypes.c_int64))[0] = getattr(f, 'removed', 0)
        return 0


def install():
    from raleigh_amd import _lib
    fake = FakeFsaiFilterLib()
    _lib.set_library(fake)
    return fake
