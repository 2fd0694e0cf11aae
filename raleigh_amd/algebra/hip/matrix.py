"""MI355X implementation of RALEIGH's dense Matrix operator.

Mirrors raleigh/algebra/dense_cublas.py:635-776 (constructor from ndarray or
Vectors, shape/order/data_type/dots/new_vectors/apply) with the GEMM of
``apply`` running in librlhip.so (rlh_dense_apply, MFMA for fp32).
"""

import numpy as np

from ... import _lib
from . import device_data
from .memory import DeviceBuffer, upload
from .vectors import Vectors, _padded


class _Borrowed:
    """Device memory that belongs to the caller (a torch tensor): an address, nothing to release."""

    def __init__(self, owner):
        self.owner = owner              # kept alive for as long as anything addresses its memory
        self.ptr = int(owner.data_ptr())
        self.nbytes = 0


class Matrix:

    def __init__(self, arg):
        if isinstance(arg, Vectors):
            f, m = arg.selected()
            self._shape = (m, arg.dimension())
            self._dtype = arg.data_type()
            self._order = 'C_CONTIGUOUS'
            self._lda = arg.ld()
            self._buf = arg.vectors_data()
            self._off = arg.data_ptr() - (self._buf.ptr if self._buf is not None else 0)
        elif isinstance(arg, np.ndarray):
            if arg.ndim != 2:
                raise ValueError('Matrix data must be a 2D array')
            self._shape = arg.shape
            self._dtype = arg.dtype.type
            if arg.flags['C_CONTIGUOUS']:
                self._order = 'C_CONTIGUOUS'
                rows, cols, host = arg.shape[0], arg.shape[1], arg
            elif arg.flags['F_CONTIGUOUS']:
                self._order = 'F_CONTIGUOUS'
                rows, cols, host = arg.shape[1], arg.shape[0], arg.T
            else:
                raise ValueError('Matrix data must be either C- or F-contiguous')
            if self._dtype not in _lib.DTYPE_CODE:
                raise ValueError('data type %s not supported' % repr(self._dtype))
            self._lda = _padded(cols)
            es = arg.itemsize
            self._buf = DeviceBuffer(max(rows, 1) * self._lda * es)
            self._off = 0
            upload(self._buf.ptr, self._lda * es, host)
        elif device_data.is_device_tensor(arg):
            self._from_device_tensor(arg)
        else:
            raise ValueError('wrong argument %s in Matrix constructor' % repr(type(arg)))
        self._code = _lib.DTYPE_CODE[self._dtype]
        self._es = _lib.DTYPE_SIZE[self._dtype]

    def _from_device_tensor(self, t):
        """A 2D strided tensor in device memory: BORROWED as it stands (no copy; the Matrix keeps the tensor alive and
        never writes it) when the fast kernels take its layout -- unit stride along one axis, address and leading
        dimension in bytes both multiples of 16, the storage reaching to the end of the last leading dimension --
        otherwise copied once, device to device, into the padded layout the ndarray constructor makes."""
        if t.dim() != 2:
            raise ValueError('Matrix data must be a 2D tensor')
        self._dtype = device_data.numpy_type(t)
        if self._dtype not in _lib.DTYPE_CODE:
            raise ValueError('data type %s not supported' % repr(self._dtype))
        self._shape = tuple(t.shape)
        es = t.element_size()
        s0, s1 = t.stride()
        if t.is_contiguous() or (s1 == 1 and s0 >= t.shape[1]):
            self._order = 'C_CONTIGUOUS'
            rows, cols, ld = t.shape[0], t.shape[1], (t.shape[1] if t.is_contiguous() else s0)
        elif s0 == 1 and s1 >= t.shape[0]:
            self._order = 'F_CONTIGUOUS'
            rows, cols, ld = t.shape[1], t.shape[0], s1
        else:
            raise ValueError('Matrix data must have unit stride along one axis: make the tensor contiguous first')
        self._tensor = None
        if rows > 0 and cols > 0 and t.data_ptr() % 16 == 0 and (ld * es) % 16 == 0 \
                and device_data.storage_room(t) >= rows * ld * es:
            self._tensor = t                    # borrowed
            self._buf = _Borrowed(t)
            self._lda = ld
        else:
            self._lda = _padded(cols)
            self._buf = DeviceBuffer(max(rows, 1) * self._lda * es)
            if rows > 0 and cols > 0:
                _lib.check(_lib.lib().rlh_copy2d(self._buf.ptr, self._lda * es, t.data_ptr(), ld * es, cols * es, rows, 2))
                _lib.check(_lib.lib().rlh_sync())       # the caller's tensor is not needed after the constructor
        self._off = 0

    def borrowed(self):
        """True when the data are the caller's device tensor itself, not a library allocation."""
        return getattr(self, '_tensor', None) is not None

    def data_ptr(self):
        return (self._buf.ptr if self._buf is not None else 0) + self._off

    def matrix_data(self):
        return self._buf

    def lda(self):
        return self._lda

    def order(self):
        return self._order

    def shape(self):
        return self._shape

    def data_type(self):
        return self._dtype

    def data_size(self):
        return self._es

    def is_complex(self):
        return self._dtype in (np.complex64, np.complex128)

    def fill(self, data):
        if self.borrowed():
            raise ValueError('a Matrix over a borrowed tensor is never written')
        host = data if self._order == 'C_CONTIGUOUS' else data.T
        upload(self.data_ptr(), self._lda * self._es, np.ascontiguousarray(host, dtype=self._dtype))

    def dots(self):
        """Squared norms of the rows."""
        if self._order != 'C_CONTIGUOUS':
            # the device holds the columns: row i collects element i of every stored column
            rows, cols = self._shape
            w = np.zeros((rows,), dtype=self._dtype)
            if rows > 0:
                L = _lib.lib()
                tmp = DeviceBuffer(rows * self._es, zero=False)
                _lib.check(L.rlh_dots_transp(self._code, rows, cols, self.data_ptr(), self._lda,
                                             self.data_ptr(), self._lda, tmp.ptr))
                _lib.check(L.rlh_d2h(_lib.host_ptr(w), tmp.ptr, rows * self._es))
            return w
        v = Vectors(self, shallow=True)
        return v.dots(v)

    def absmax(self):
        """Largest modulus of the (real / imaginary parts of the) entries, computed on the device."""
        import ctypes
        rows = self._shape[0] if self._order == 'C_CONTIGUOUS' else self._shape[1]
        cols = self._shape[1] if self._order == 'C_CONTIGUOUS' else self._shape[0]
        out = ctypes.c_double()
        _lib.check(_lib.lib().rlh_absmax(self._code, cols, rows, self.data_ptr(), self._lda, ctypes.byref(out)))
        return float(out.value)

    def new_vectors(self, dim=None, nv=0):
        if dim is None:
            dim = self.shape()[1]
        return Vectors(dim, nv, self.data_type())

    def apply(self, x, y, transp=False):
        self.apply_r1(x, y, transp)

    def apply_r1(self, x, y, transp=False, u=None, c=None):
        """y = Op(A) x - u c^T with the rank-one term folded into the product's epilogue (rlh_dense_apply_r1):
        `c` a device pointer to x.nvec() coefficients (e.g. written by `coefficients_into`), `u` a Vectors
        window of ONE vector of y's dimension or None for a vector of ones.  c None: the plain product."""
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
        _lib.check(_lib.lib().rlh_dense_apply_r1(
            self._code, m, n, self.data_ptr(), self._lda,
            0 if self._order == 'C_CONTIGUOUS' else 1, 1 if transp else 0,
            k, x.data_ptr(), x.ld(), y.data_ptr(), y.ld(),
            None if u is None else u.data_ptr(), c))


def coefficients_into(buf_ptr, x, w):
    """buf[j] = <x_j, w> = w^H x_j for the selected vectors of x and the ONE vector w, written to DEVICE
    memory at buf_ptr without a host synchronisation (rlh_gram with a device output): the coefficients
    of a rank-one epilogue."""
    if w.nvec() != 1 or w.dimension() != x.dimension():
        raise ValueError('one vector of the same dimension is needed')
    n = getattr(x, 'local_dimension', x.dimension)()
    _lib.check(_lib.lib().rlh_gram(x._code, n, x.nvec(), x.data_ptr(), x.ld(), 1, w.data_ptr(), w.ld(), buf_ptr, None))
