"""tests/fake_lib.py's stand-in library plus the rlh_bytes_* entry points (dense 8-bit data matrix) in NumPy
float32: TEST INFRASTRUCTURE ONLY, so that the CPU tier runs truncated_svd / pca on uint8 / int8 input through
the same host logic as the GPU.  "Device" pointers are host addresses, as in FakeLib."""

import ctypes

import numpy as np

import fake_lib
from fake_lib import _addr, _block, _flat


class FakeByteDataLib(fake_lib.FakeLib):

    def __init__(self):
        super().__init__()
        self._bytes = {}

    def rlh_bytes_create(self, ph, kind, n_rows, n_cols, h_data, row_stride):
        if kind not in (0, 1):
            return self._fail('rlh_bytes_create: kind must be 0 (uint8) or 1 (int8)')
        if row_stride < n_cols:
            return self._fail('rlh_bytes_create: row stride smaller than the number of columns')
        dt = np.int8 if kind else np.uint8
        if n_rows and n_cols:
            flat = _flat(h_data, dt, (n_rows - 1) * row_stride + n_cols)
            a = np.lib.stride_tricks.as_strided(flat, shape=(n_rows, n_cols), strides=(row_stride, 1)).copy()
        else:
            a = np.zeros((n_rows, n_cols), dtype=dt)
        h = self._next_handle
        self._next_handle += 1
        self._bytes[h] = a                      # kept as bytes: widened product by product, never as a whole copy
        ph._obj.value = h
        return 0

    def rlh_bytes_destroy(self, h):
        self._bytes.pop(_addr(h), None)
        return 0

    def rlh_bytes_info(self, h, n_rows, n_cols, device_bytes, workspace_bytes):
        a = self._bytes[_addr(h)]
        lda = max(16, (a.shape[1] + 15) // 16 * 16)
        for p, v in ((n_rows, a.shape[0]), (n_cols, a.shape[1]), (device_bytes, max(a.shape[0], 1) * lda),
                     (workspace_bytes, 0)):
            if p is not None:
                ctypes.cast(p, ctypes.POINTER(ctypes.c_int64))[0] = v
        return 0

    def rlh_bytes_apply(self, h, transp, m, X, ldx, Y, ldy, d_u, d_c):
        self._count('bytes_apply')
        a = self._bytes[_addr(h)]
        if _addr(d_u) and not _addr(d_c):
            return self._fail('rlh_bytes_apply: a vector u without coefficients c')
        op = (a.T if transp else a).astype(np.float32)
        ny, nx = op.shape
        if ldx < nx or ldy < ny:
            return self._fail('rlh_bytes_apply: Matrix and vectors dimensions incompatible')
        if m == 0 or ny == 0:
            return 0
        x = _block(X, 0, nx, m, ldx)
        y = (op @ x.T).T.astype(np.float32)
        if _addr(d_c):
            c = _flat(d_c, np.float32, m)
            u = _flat(d_u, np.float32, ny) if _addr(d_u) else np.ones(ny, dtype=np.float32)
            y = y - c[:, None] * u[None, :]
        _block(Y, 0, ny, m, ldy)[:, :] = y
        return 0

    def rlh_bytes_row_sumsq(self, h, h_out):
        a = self._bytes[_addr(h)].astype(np.int64)
        if a.shape[0]:
            _flat(h_out, np.float64, a.shape[0])[:] = (a * a).sum(axis=1).astype(np.float64)
        return 0

    def rlh_bytes_absmax(self, h, h_out):
        a = self._bytes[_addr(h)]
        val = 0.0 if a.size == 0 else float(np.abs(a.astype(np.int64)).max())
        ctypes.cast(h_out, ctypes.POINTER(ctypes.c_double))[0] = val
        return 0


def install():
    from raleigh_amd import _lib
    fake = FakeByteDataLib()
    _lib.set_library(fake)
    return fake
