"""MI355X operator of a general (rectangular) sparse data matrix: truncated SVD and PCA of sparse data.

The sparse counterpart of ``Matrix`` (matrix.py): the same ``shape / data_type / new_vectors / apply /
apply_r1 / dots / absmax`` surface the interfaces use, with the products running in librlhip.so
(rlh_spd_apply: A and a CSR copy of A^H on the device, work split by nonzeros, the rank-one term of the
mean shift in the epilogue).  The data are never densified.
"""

import ctypes

import numpy as np
import scipy.sparse as scs

from ... import _lib
from . import device_data
from .vectors import Vectors


def canonical_csr(a):
    """A scipy.sparse matrix or array as a canonical CSR matrix (duplicates summed, indices sorted); the
    caller's object is never modified.  Unsupported value types, integer ones included, raise ValueError."""
    if not scs.issparse(a):
        raise ValueError('a scipy.sparse matrix is needed')
    if a.ndim != 2:
        raise ValueError('a 2D sparse matrix is needed')
    if a.dtype.type not in _lib.DTYPE_CODE:
        raise ValueError('data type %s not supported' % repr(a.dtype.type))
    csr = scs.csr_matrix(a)
    if not csr.has_canonical_format:
        csr = csr.copy()
        csr.sum_duplicates()
    return csr


class SparseMatrix:

    def __init__(self, a):
        self._dots = self._absmax = None
        if device_data.is_device_tensor(a):
            self._from_device_tensor(a)
            return
        csr = canonical_csr(a)
        self._dtype = csr.dtype.type
        self._shape = csr.shape
        self._nnz = int(csr.nnz)
        self._code = _lib.DTYPE_CODE[self._dtype]
        # squared row norms (float64) and the largest entry, once, from the host values
        rows = np.repeat(np.arange(self._shape[0]), np.diff(csr.indptr))
        self._dots = np.bincount(rows, weights=np.abs(csr.data).astype(np.float64) ** 2, minlength=self._shape[0])
        if self._nnz == 0:
            self._absmax = 0.0
        elif self.is_complex():
            self._absmax = float(max(np.abs(csr.data.real).max(), np.abs(csr.data.imag).max()))
        else:
            self._absmax = float(np.abs(csr.data).max())
        indptr = np.ascontiguousarray(csr.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(csr.indices, dtype=np.int32)
        values = np.ascontiguousarray(csr.data)
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().rlh_spd_create(ctypes.byref(h), self._code, self._shape[0], self._shape[1],
                                             _lib.host_ptr(indptr), _lib.host_ptr(indices), _lib.host_ptr(values)))
        self._h = h

    def _from_device_tensor(self, t):
        """A torch.sparse_csr tensor in device memory: both CSR copies and the partition are built by kernels
        (rlh_spd_create_device), which also check that the tensor is canonical -- rows with ascending columns and no
        duplicates, as torch's own constructors and conversions produce; the squared row norms and the largest entry
        come from the device copy when first asked for.  The tensor's arrays are copied, never written."""
        import torch
        if t.layout != torch.sparse_csr or t.dim() != 2:
            raise ValueError('a 2D torch.sparse_csr tensor is needed')
        self._dtype = device_data.numpy_type(t)
        if self._dtype not in _lib.DTYPE_CODE:
            raise ValueError('data type %s not supported' % repr(self._dtype))
        crow, col, val = t.crow_indices(), t.col_indices(), t.values()
        bits = {'int32': 32, 'int64': 64}.get(str(crow.dtype).split('.')[-1])
        if bits is None or col.dtype != crow.dtype:
            raise ValueError('sparse index type %s not supported (int32, int64)' % crow.dtype)
        crow, col, val = crow.contiguous(), col.contiguous(), val.detach().resolve_conj().resolve_neg().contiguous()
        if val.is_cuda:
            torch.cuda.current_stream(val.device).synchronize()
        self._shape = tuple(t.shape)
        self._code = _lib.DTYPE_CODE[self._dtype]
        h = ctypes.c_void_p()
        try:
            _lib.check(_lib.lib().rlh_spd_create_device(
                ctypes.byref(h), self._code, self._shape[0], self._shape[1], bits, ctypes.c_void_p(crow.data_ptr()),
                ctypes.c_void_p(col.data_ptr()), ctypes.c_void_p(val.data_ptr())))
        except _lib.RlhError as e:
            if ': rlh_spd_create_device:' in str(e):         # the library's own check, not a HIP failure
                raise ValueError('the sparse tensor is not canonical CSR: %s' % e)
            raise
        self._h = h
        nnz = ctypes.c_int64()
        _lib.check(_lib.lib().rlh_spd_info(self._h, None, None, ctypes.byref(nnz), None))
        self._nnz = int(nnz.value)

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h:
            try:
                _lib.library().rlh_spd_destroy(h)
            except Exception:       # interpreter shutdown
                pass

    def shape(self):
        return self._shape

    def data_type(self):
        return self._dtype

    def is_complex(self):
        return self._dtype in (np.complex64, np.complex128)

    def nnz(self):
        return self._nnz

    def device_bytes(self):
        """Device memory held by the operator: both CSR copies, the work partition and the workspace."""
        nb = ctypes.c_int64()
        _lib.check(_lib.lib().rlh_spd_info(self._h, None, None, None, ctypes.byref(nb)))
        return int(nb.value)

    def workspace_bytes(self):
        nb, t = ctypes.c_int64(), ctypes.c_double()
        _lib.check(_lib.lib().rlh_spd_stats(self._h, ctypes.byref(nb), ctypes.byref(t)))
        return int(nb.value)

    def transpose_seconds(self):
        """Seconds taken by building the CSR copy of A^H when the operator was created: on the host threads, or on the
        device (measured with events) for an operator built from device arrays."""
        nb, t = ctypes.c_int64(), ctypes.c_double()
        _lib.check(_lib.lib().rlh_spd_stats(self._h, ctypes.byref(nb), ctypes.byref(t)))
        return float(t.value)

    def dots(self):
        """Squared norms of the rows (float64): from the host values at construction, or from the device copy
        (rlh_spd_row_sumsq) when the operator was built from device arrays; computed once."""
        if self._dots is None:
            out = np.zeros(self._shape[0], dtype=np.float64)
            _lib.check(_lib.lib().rlh_spd_row_sumsq(self._h, _lib.host_ptr(out)))
            self._dots = out
        return self._dots.copy()

    def absmax(self):
        """Largest modulus of the (real / imaginary parts of the) entries."""
        if self._absmax is None:
            out = ctypes.c_double()
            _lib.check(_lib.lib().rlh_spd_absmax(self._h, ctypes.byref(out)))
            self._absmax = float(out.value)
        return self._absmax

    def new_vectors(self, dim=None, nv=0):
        if dim is None:
            dim = self.shape()[1]
        return Vectors(dim, nv, self.data_type())

    def apply(self, x, y, transp=False):
        self.apply_r1(x, y, transp)

    def apply_r1(self, x, y, transp=False, u=None, c=None):
        """y = Op(A) x - u c^T with the rank-one term in the product's epilogue (as Matrix.apply_r1): `c` a device
        pointer to x.nvec() coefficients, `u` a Vectors window of ONE vector of y's dimension or None for a vector
        of ones.  c None: the plain product."""
        if x.data_type() != self._dtype or y.data_type() != self._dtype:
            raise ValueError('Matrix and vectors data types differ')
        m, n = self._shape
        if transp:
            if n != y.dimension() or m != x.dimension():
                raise ValueError('Matrix and vectors dimensions incompatible')
        else:
            if m != y.dimension() or n != x.dimension():
                raise ValueError('Matrix and vectors dimensions incompatible')
        k = x.nvec()
        if k != y.nvec():
            raise ValueError('Numbers of input and output vectors differ')
        if u is not None and (u.nvec() != 1 or u.dimension() != y.dimension() or c is None):
            raise ValueError('the rank-one term needs one vector of the output dimension and coefficients')
        _lib.check(_lib.lib().rlh_spd_apply(self._h, 1 if transp else 0, k, x.data_ptr(), x.ld(), y.data_ptr(), y.ld(),
                                            None if u is None else u.data_ptr(), c))
