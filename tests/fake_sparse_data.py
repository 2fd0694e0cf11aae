"""tests/fake_lib.py's stand-in library plus the rlh_spd_* entry points (general sparse data matrix) on top of
SciPy: TEST INFRASTRUCTURE ONLY, so that the CPU tier runs truncated_svd / pca on sparse input through the
same host logic as the GPU.  "Device" pointers are host addresses, as in FakeLib."""

import ctypes

import numpy as np
import scipy.sparse as sp

import fake_lib
from fake_lib import _DT, _addr, _block, _flat


class FakeSparseDataLib(fake_lib.FakeLib):

    def __init__(self):
        super().__init__()
        self._spd = {}

    def rlh_spd_create(self, ph, code, n_rows, n_cols, indptr, indices, values):
        ip = _flat(indptr, np.int64, n_rows + 1).copy()
        nnz = int(ip[-1])
        ix = _flat(indices, np.int32, nnz).copy()
        va = _flat(values, _DT[code], nnz).copy()
        if nnz and (ix.min() < 0 or ix.max() >= n_cols):
            return self._fail('rlh_spd_create: column index out of range')
        h = self._next_handle
        self._next_handle += 1
        a = sp.csr_matrix((va, ix, ip), shape=(n_rows, n_cols))
        self._spd[h] = (a, sp.csr_matrix(a.conj().T), code)
        ph._obj.value = h
        return 0

    def rlh_spd_destroy(self, h):
        self._spd.pop(_addr(h), None)
        return 0

    def rlh_spd_info(self, h, n_rows, n_cols, nnz, nbytes):
        a, at, code = self._spd[_addr(h)]
        es = np.dtype(_DT[code]).itemsize
        for p, v in ((n_rows, a.shape[0]), (n_cols, a.shape[1]), (nnz, a.nnz),
                     (nbytes, 2 * a.nnz * (es + 4) + 8 * (a.shape[0] + a.shape[1] + 2))):
            if p is not None:
                ctypes.cast(p, ctypes.POINTER(ctypes.c_int64))[0] = v
        return 0

    def rlh_spd_stats(self, h, work, seconds):
        ctypes.cast(work, ctypes.POINTER(ctypes.c_int64))[0] = 0
        ctypes.cast(seconds, ctypes.POINTER(ctypes.c_double))[0] = 0.0
        return 0

    def rlh_spd_apply(self, h, transp, m, X, ldx, Y, ldy, d_u, d_c):
        self._count('spd_apply')
        a, at, code = self._spd[_addr(h)]
        op = at if transp else a
        ny, nx = op.shape
        if ldx < nx or ldy < ny:
            return self._fail('rlh_spd_apply: Matrix and vectors dimensions incompatible')
        if m == 0 or ny == 0:
            return 0
        x = _block(X, code, nx, m, ldx)
        y = np.asarray(op @ x.T).T.astype(_DT[code])
        if _addr(d_c):
            c = _flat(d_c, _DT[code], m)
            u = _flat(d_u, _DT[code], ny) if _addr(d_u) else np.ones(ny, dtype=_DT[code])
            y = y - c[:, None] * u[None, :]
        _block(Y, code, ny, m, ldy)[:, :] = y
        return 0


def install():
    from raleigh_amd import _lib
    fake = FakeSparseDataLib()
    _lib.set_library(fake)
    return fake
