"""MI355X operator of a dense 8-bit data matrix: PCA and truncated SVD of uint8 / int8 data (images).

The 8-bit counterpart of ``Matrix`` (matrix.py): the same ``shape / data_type / new_vectors / apply /
apply_r1 / dots / absmax`` surface the interfaces use.  The data stay bytes, on the host and in HBM (one copy,
a quarter of what ``Matrix`` holds for the same data as float32); the vectors are float32 and the products
run in librlhip.so on the bfloat16 matrix cores (rlh_bytes_apply: A converted exactly, the block split
exactly into three bfloat16 planes, float32 accumulation -- the error of a float32 product).
"""

import ctypes

import numpy as np

from ... import _lib
from . import device_data
from .vectors import Vectors

_KINDS = {np.uint8: 0, np.int8: 1}


class ByteMatrix:

    def __init__(self, a):
        self._tensor = None
        if device_data.is_device_tensor(a):
            self._from_device_tensor(a)
            return
        if not isinstance(a, np.ndarray):
            raise ValueError('wrong argument %s in ByteMatrix constructor' % repr(type(a)))
        if a.ndim != 2:
            raise ValueError('Matrix data must be a 2D array')
        if a.dtype.type not in _KINDS:
            raise ValueError('data type %s not supported' % repr(a.dtype.type))
        if not a.flags['C_CONTIGUOUS']:
            raise ValueError('8-bit matrix data must be C-contiguous')
        self._storage = a.dtype.type
        self._shape = a.shape
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().rlh_bytes_create(ctypes.byref(h), _KINDS[self._storage], a.shape[0], a.shape[1],
                                               _lib.host_ptr(a), a.shape[1]))
        self._h = h
        self._dots = None
        self._absmax = None

    def _from_device_tensor(self, t):
        """Row-major bytes in device memory (rlh_bytes_create_device): borrowed when the number of columns, the row
        stride and the address are multiples of 16, else copied into the padded layout by a kernel.  The tensor is
        kept alive with the operator and never written."""
        if t.dim() != 2:
            raise ValueError('Matrix data must be a 2D tensor')
        dt = device_data.numpy_type(t)
        if dt not in _KINDS:
            raise ValueError('data type %s not supported' % repr(dt))
        if t.shape[0] > 1 and t.shape[1] > 0 and (t.stride(1) != 1 or t.stride(0) < t.shape[1]) \
                or t.shape[1] > 1 and t.stride(1) != 1:
            raise ValueError('8-bit matrix data must be row-major with unit stride along the rows: make the tensor '
                             'contiguous first')
        self._storage = dt
        self._shape = tuple(t.shape)
        stride = t.stride(0) if t.shape[0] > 1 else t.shape[1]
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().rlh_bytes_create_device(ctypes.byref(h), _KINDS[dt], t.shape[0], t.shape[1],
                                                      ctypes.c_void_p(t.data_ptr()), max(stride, t.shape[1])))
        self._h = h
        self._tensor = t
        self._dots = None
        self._absmax = None

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h:
            try:
                _lib.library().rlh_bytes_destroy(h)
            except Exception:       # interpreter shutdown
                pass

    def shape(self):
        return self._shape

    def data_type(self):
        """The type of the vectors the operator acts on (and of every result): float32."""
        return np.float32

    def storage_type(self):
        """The type of the stored entries: numpy.uint8 or numpy.int8."""
        return self._storage

    def is_complex(self):
        return False

    def _info(self):
        nb, nw = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(_lib.lib().rlh_bytes_info(self._h, None, None, ctypes.byref(nb), ctypes.byref(nw)))
        return int(nb.value), int(nw.value)

    def device_bytes(self):
        """Device memory held by the operator: the bytes of the data and the workspace."""
        return self._info()[0]

    def workspace_bytes(self):
        """The split-K workspace alone."""
        return self._info()[1]

    def dots(self):
        """Squared norms of the rows: exact integer sums formed on the device, as float64."""
        if self._dots is None:
            out = np.zeros(self._shape[0], dtype=np.float64)
            _lib.check(_lib.lib().rlh_bytes_row_sumsq(self._h, _lib.host_ptr(out)))
            self._dots = out
        return self._dots.copy()

    def absmax(self):
        """Largest modulus of the entries (exact), found on the device."""
        if self._absmax is None:
            out = ctypes.c_double()
            _lib.check(_lib.lib().rlh_bytes_absmax(self._h, ctypes.byref(out)))
            self._absmax = float(out.value)
        return self._absmax

    def new_vectors(self, dim=None, nv=0):
        if dim is None:
            dim = self.shape()[1]
        return Vectors(dim, nv, np.float32)

    def apply(self, x, y, transp=False):
        self.apply_r1(x, y, transp)

    def apply_r1(self, x, y, transp=False, u=None, c=None):
        """y = Op(A) x - u c^T with the rank-one term in the product's epilogue (as Matrix.apply_r1): `c` a device
        pointer to x.nvec() float32 coefficients, `u` a Vectors window of ONE vector of y's dimension or None for a
        vector of ones.  c None: the plain product."""
        if x.data_type() != np.float32 or y.data_type() != np.float32:
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
        _lib.check(_lib.lib().rlh_bytes_apply(self._h, 1 if transp else 0, k, x.data_ptr(), x.ld(), y.data_ptr(), y.ld(),
                                              None if u is None else u.data_ptr(), c))
