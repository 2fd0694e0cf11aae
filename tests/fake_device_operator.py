"""tests/fake_device_data.py's stand-in library plus rlh_csr_create_device (the sparse operator from CSR arrays
already in device memory) in SciPy, with the checks and messages of the real entry point: TEST INFRASTRUCTURE ONLY.
The host creation calls are counted too, so that a test can tell which path built an operator."""

import numpy as np
import scipy.sparse as sp

from fake_lib import _DT, _Csr, _flat
import fake_csr_input
import fake_device_data
from fake_device_data import as_device  # noqa: F401


class FakeDeviceOperatorLib(fake_device_data.FakeDeviceDataLib):

    def rlh_csr_create(self, *a):
        self._count('csr_create')
        return super().rlh_csr_create(*a)

    def rlh_csr_create_upper(self, *a):
        self._count('csr_create_upper')
        return super().rlh_csr_create_upper(*a)

    def rlh_csr_create_device(self, ph, code, n_rows, n_cols, index_bits, indptr, indices, values, mirror_upper):
        self._count('csr_create_device')
        ph._obj.value = None
        name = 'rlh_csr_create_device: '
        if index_bits not in (32, 64):
            return self._fail(name + 'index_bits must be 32 or 64, got %d' % index_bits)
        if mirror_upper and n_rows != n_cols:
            return self._fail(name + 'mirror_upper needs a square matrix, got %d x %d' % (n_rows, n_cols))
        it = np.int32 if index_bits == 32 else np.int64
        ip = _flat(indptr, it, n_rows + 1).astype(np.int64)
        if msg := fake_csr_input.indptr_message(name, ip):
            return self._fail(msg)
        nnz = int(ip[-1])
        ix = _flat(indices, it, nnz).astype(np.int64)
        va = _flat(values, _DT[code], nnz).copy()
        if msg := fake_csr_input.columns_message(name, ip, ix, n_cols):
            return self._fail(msg)
        rows = np.repeat(np.arange(n_rows), np.diff(ip))
        a = sp.csr_matrix((va, ix.astype(np.int32), ip), shape=(n_rows, n_cols))
        if mirror_upper:
            stored = set(zip(rows.tolist(), ix.tolist()))
            for i, j in zip(rows.tolist(), ix.tolist()):
                if i != j and (j, i) not in stored:
                    return self._fail(name + 'the stored structure is not symmetric: entry (%d, %d) has no partner '
                                      '(%d, %d); the device build creates no entries' % (i, j, j, i))
            u, s1 = sp.triu(a, format='csr'), sp.triu(a, k=1, format='csr')
            a = sp.csr_matrix(u + s1.conj().T)
        h = self._next_handle
        self._next_handle += 1
        self._csr[h] = _Csr(a, code)
        ph._obj.value = h
        return 0


def install():
    from raleigh_amd import _lib
    fake = FakeDeviceOperatorLib()
    _lib.set_library(fake)
    return fake
