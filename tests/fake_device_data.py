"""tests/fake_byte_data.py's and tests/fake_sparse_data.py's stand-in libraries plus the entry points that take data
already in device memory (rlh_spd_create_device, rlh_spd_row_sumsq, rlh_spd_absmax, rlh_bytes_create_device) in
NumPy / SciPy: TEST INFRASTRUCTURE ONLY.  "Device" pointers are host addresses, as in FakeLib, so a CPU torch tensor
plays the part of a device tensor once ``device_data._on_device`` is patched (``as_device``)."""

import ctypes

import numpy as np
import scipy.sparse as sp

from fake_lib import _DT, _addr, _flat
import fake_byte_data
import fake_csr_input
import fake_sparse_data


class FakeDeviceDataLib(fake_byte_data.FakeByteDataLib, fake_sparse_data.FakeSparseDataLib):

    def rlh_bytes_create_device(self, ph, kind, n_rows, n_cols, d_data, row_stride):
        self._count('bytes_create_device')
        return self.rlh_bytes_create(ph, kind, n_rows, n_cols, d_data, row_stride)

    def rlh_spd_create_device(self, ph, code, n_rows, n_cols, index_bits, indptr, indices, values):
        self._count('spd_create_device')
        ph._obj.value = None
        if index_bits not in (32, 64):
            return self._fail('rlh_spd_create_device: index_bits must be 32 or 64')
        it = np.int32 if index_bits == 32 else np.int64
        ip = _flat(indptr, it, n_rows + 1).astype(np.int64)
        if msg := fake_csr_input.indptr_message('rlh_spd_create_device: ', ip, terse=True):
            return self._fail(msg)
        nnz = int(ip[-1])
        ix = _flat(indices, it, nnz).astype(np.int64)
        va = _flat(values, _DT[code], nnz).copy()
        if msg := fake_csr_input.columns_message('rlh_spd_create_device: ', ip, ix, n_cols, terse=True):
            return self._fail(msg)
        h = self._next_handle
        self._next_handle += 1
        a = sp.csr_matrix((va, ix.astype(np.int32), ip), shape=(n_rows, n_cols))
        self._spd[h] = (a, sp.csr_matrix(a.conj().T), code)
        ph._obj.value = h
        return 0

    def rlh_spd_row_sumsq(self, h, h_out):
        a = self._spd[_addr(h)][0]
        if a.shape[0]:
            rows = np.repeat(np.arange(a.shape[0]), np.diff(a.indptr))
            _flat(h_out, np.float64, a.shape[0])[:] = np.bincount(rows, weights=np.abs(a.data).astype(np.float64) ** 2,
                                                                  minlength=a.shape[0])
        return 0

    def rlh_spd_absmax(self, h, h_out):
        d = self._spd[_addr(h)][0].data
        val = 0.0 if d.size == 0 else float(max(np.abs(d.real).max(), np.abs(d.imag).max()))
        ctypes.cast(h_out, ctypes.POINTER(ctypes.c_double))[0] = val
        return 0


def install():
    from raleigh_amd import _lib
    fake = FakeDeviceDataLib()
    _lib.set_library(fake)
    return fake


def as_device(monkeypatch):
    """From here on every torch tensor counts as lying in device memory (the stand-in's device is the host)."""
    from raleigh_amd.algebra.hip import device_data
    monkeypatch.setattr(device_data, '_on_device', lambda t: True)
