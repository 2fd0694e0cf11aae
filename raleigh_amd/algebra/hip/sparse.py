"""MI355X sparse symmetric/Hermitian operator for SciPy sparse matrices and for
square ``torch.sparse_csr`` tensors that already lie on the bound GPU.

Counterpart of raleigh/algebra/sparse_mkl.py:16-48 (SparseSymmetricMatrix) and
:143-154 (Operator): same constructor argument (a SciPy sparse matrix whose
UPPER triangle defines the symmetric/Hermitian operator, as MKL's 'SUNF'/'HUNF'
descriptor does), same ``apply(x, y)``, but x and y are device Vectors and the
product runs in librlhip.so (rlh_spmm) on a sliced-ELL copy of the full matrix.

A tensor on the GPU becomes the operator without a host trip: the library builds
the device layout from the tensor's three arrays by kernels (rlh_csr_create_device).
It must store BOTH triangles (a symmetric structure): the device build creates no
entries; the values below the diagonal are ignored, as on the host path.
"""

import ctypes

import numpy as np
import scipy.sparse as scs

from ... import _lib
from . import device_data


def full_from_upper(matrix):
    """A = U + U^H - diag(U) from U = triu(matrix): what the reference's MKL call
    computes with (raleigh/algebra/mkl_wrap.py:211-276)."""
    u = scs.triu(matrix, format='csr')
    s = scs.triu(matrix, k=1, format='csr')
    full = scs.csr_matrix(u + s.conj().T)
    full.sort_indices()
    return full


class CsrOperator:
    """Device CSR operator: y = A x for rows owned by this process.  upper=True: the Hermitian operator defined by
    the upper triangle of `csr` (entries below the diagonal ignored), mirrored inside the library
    (rlh_csr_create_upper) instead of by three SciPy passes on the host."""

    def __init__(self, csr, n_own=None, upper=False):
        csr = scs.csr_matrix(csr)
        if not csr.has_canonical_format:
            # an assembled matrix may carry duplicate or unsorted entries: a COPY is put into canonical form (equal
            # columns summed, indices sorted) -- the caller's own object is never modified
            csr = csr.copy()
            csr.sum_duplicates()
        dt = csr.data.dtype.type
        if dt not in _lib.DTYPE_CODE:
            raise ValueError('unsupported data type')
        self._dtype = dt
        self._shape = csr.shape
        self._nnz = int(csr.nnz)
        self._n_own = csr.shape[1] if n_own is None else int(n_own)
        indptr = np.ascontiguousarray(csr.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(csr.indices, dtype=np.int32)
        values = np.ascontiguousarray(csr.data)
        h = ctypes.c_void_p()
        if upper:
            if csr.shape[0] != csr.shape[1] or n_own is not None:
                raise ValueError('an operator given by its upper triangle is square and unsharded')
            _lib.check(_lib.lib().rlh_csr_create_upper(ctypes.byref(h), _lib.DTYPE_CODE[dt], csr.shape[0], _lib.host_ptr(indptr),
                                                       _lib.host_ptr(indices), _lib.host_ptr(values)))
            nnz, dummy = ctypes.c_int64(), ctypes.c_int64()
            _lib.check(_lib.lib().rlh_csr_info(h, ctypes.byref(dummy), ctypes.byref(dummy), ctypes.byref(nnz), ctypes.byref(dummy)))
            self._nnz = int(nnz.value)
        else:
            _lib.check(_lib.lib().rlh_csr_create(ctypes.byref(h), _lib.DTYPE_CODE[dt], csr.shape[0],
                                                 csr.shape[1], _lib.host_ptr(indptr),
                                                 _lib.host_ptr(indices), _lib.host_ptr(values)))
        self._h = h

    @classmethod
    def from_tensor(cls, t, upper=False):
        """The operator of a ``torch.sparse_csr`` tensor on the bound GPU (checked by ``operator_tensor`` or
        ``device_data.prepare``), built on the device from its three arrays, which are read in place and not kept.
        upper=True: the Hermitian operator defined by the upper triangle (rlh_csr_create_device, mirror_upper)."""
        self = cls.__new__(cls)
        dt = device_data.numpy_type(t)
        if dt not in _lib.DTYPE_CODE:
            raise ValueError('unsupported data type')
        if upper and t.shape[0] != t.shape[1]:
            raise ValueError('an operator given by its upper triangle is square and unsharded')
        import torch
        crow, col, val = t.crow_indices(), t.col_indices(), t.values()
        if col.dtype != crow.dtype:                 # (torch takes mixed index types: both as the wider one)
            crow, col = crow.to(torch.int64), col.to(torch.int64)
        crow, col, val = crow.contiguous(), col.contiguous(), val.detach().resolve_conj().resolve_neg().contiguous()
        # the conversions above may have launched work on torch's stream after device_data.prepare synchronised
        # it; the library reads the arrays on its own stream, so that work has to be finished first
        if val.is_cuda:
            torch.cuda.current_stream(val.device).synchronize()
        self._dtype = dt
        self._shape = tuple(t.shape)
        self._n_own = self._shape[1]
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().rlh_csr_create_device(ctypes.byref(h), _lib.DTYPE_CODE[dt], self._shape[0], self._shape[1],
                                                    32 if crow.element_size() == 4 else 64, crow.data_ptr(),
                                                    col.data_ptr(), val.data_ptr(), 1 if upper else 0))
        self._h = h
        self._nnz = int(val.numel())
        return self

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h:
            try:
                _lib.library().rlh_csr_destroy(h)
            except Exception:
                pass

    def shape(self):
        return self._shape

    def nnz(self):
        return self._nnz

    def data_type(self):
        return self._dtype

    def layout(self):
        """('sell' | 'well' | 'wide', stored entry slots, staged elements per slot): the device layout
        the library chose (rlh_csr_layout)."""
        lay, stored, ratio = ctypes.c_int(), ctypes.c_int64(), ctypes.c_double()
        _lib.check(_lib.lib().rlh_csr_layout(self._h, ctypes.byref(lay), ctypes.byref(stored), ctypes.byref(ratio)))
        return ('sell', 'well', 'wide')[lay.value], int(stored.value), float(ratio.value)

    def stacks(self):
        """(stacks, staged elements per row and vector without / with them): the stacked row blocks of the windowed
        layout (rlh_csr_stacks); 0 stacks when the layout was not built."""
        n, a, b = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
        _lib.check(_lib.lib().rlh_csr_stacks(self._h, ctypes.byref(n), ctypes.byref(a), ctypes.byref(b)))
        return int(n.value), float(a.value), float(b.value)

    def bf16_ready(self, ldh=0):
        """Whether the bfloat16 Chebyshev step takes this operator (rlh_csr_bf16_ready); ldh: the leading dimension of
        the halo block of a row shard (ignored without halo columns)."""
        ok = ctypes.c_int()
        _lib.check(_lib.lib().rlh_csr_bf16_ready(self._h, self._n_own, int(ldh), ctypes.byref(ok)))
        return bool(ok.value)

    def apply_ptr(self, m, x_ptr, ldx, y_ptr, ldy, halo_ptr=None, ldh=0, part=0):
        """part 0: all rows; 1: the rows that need no halo column; 2: the others (rlh_spmm_part)."""
        _lib.check(_lib.lib().rlh_spmm_part(self._h, part, m, x_ptr, ldx, self._n_own, halo_ptr, ldh, y_ptr, ldy))

    def cheb_step_bf16(self, m, y, p, b, cy, cp, cb, halo_ptr=None, ldh=0, part=0):
        _lib.check(_lib.lib().rlh_spmm_cheb_bf16_part(self._h, part, m, y.ptr(), y.ld, self._n_own, halo_ptr, ldh,
                                                      p.ptr(), p.ld, b.ptr(), b.ld, float(cy), float(cp), float(cb)))

    def cheb_step_ptr(self, m, y, p, b, cy, cp, cb, halo_ptr=None, ldh=0, part=0):
        """p = cy y + cp p + cb (b - A y) in one pass (y, p, b: Vectors windows; p updated in place)."""
        _lib.check(_lib.lib().rlh_spmm_cheb_part(self._h, part, m, y.data_ptr(), y.ld(), self._n_own, halo_ptr, ldh,
                                                 p.data_ptr(), p.ld(), b.data_ptr(), b.ld(),
                                                 float(cy), float(cp), float(cb)))


class Bf16Block:
    """A block of vectors stored as bfloat16 (device memory, column-major, leading dimension a
    multiple of 8): work storage of the polynomial preconditioner, not a Vectors type."""

    def __init__(self, n, m):
        from .memory import DeviceBuffer
        self.n, self.m = int(n), int(m)
        self.ld = -(-self.n // 64) * 64
        self._buf = DeviceBuffer(max(self.m, 1) * self.ld * 2, zero=False)

    def ptr(self):
        return self._buf.ptr

    def zero(self, m):
        _lib.check(_lib.lib().rlh_memset(self._buf.ptr, 0, ((m - 1) * self.ld + self.n) * 2))

    def pack(self, x, scale=1.0):
        """self[:, :m] = bf16(scale * x) for a float32 / float64 Vectors window x."""
        _lib.check(_lib.lib().rlh_bf16_pack(x._code, self.n, x.nvec(), x.data_ptr(), x.ld(), float(scale),
                                            self._buf.ptr, self.ld))

    def unpack(self, y):
        _lib.check(_lib.lib().rlh_bf16_unpack(y._code, self.n, y.nvec(), self._buf.ptr, self.ld, y.data_ptr(), y.ld()))


def operator_tensor(t):
    """Checks a torch tensor given as the matrix of an eigenproblem and returns it prepared (device_data.prepare):
    a square ``torch.sparse_csr`` tensor of a float or complex type, on the CPU or on the bound GPU."""
    import torch
    if t.layout != torch.sparse_csr:
        raise ValueError('tensor layout %s not supported for a sparse operator: torch.sparse_csr (use to_sparse_csr())'
                         % t.layout)
    t = device_data.prepare(t)
    if t.shape[0] != t.shape[1]:
        raise ValueError('a square matrix is needed, got %d x %d' % tuple(t.shape))
    return t


def tensor_to_scipy(t):
    """A sparse_csr tensor as a scipy.sparse.csr_matrix: ONE copy to the host if it lies on a GPU."""
    return device_data.to_host(t.cpu())


class SparseSymmetricMatrix:

    def __init__(self, matrix):
        # the UPPER triangle of `matrix` defines the operator (sparse_mkl.py:16-40); the library mirrors it, so the
        # matrix goes in as it comes (both triangles or one) and triu() is only taken if somebody asks for csr()
        self.__tensor = None
        if device_data.is_tensor(matrix):
            t = operator_tensor(matrix)
            if device_data._on_device(t):
                # built on the device from the tensor's arrays; the tensor is kept (not copied) for csr()
                self.__tensor = t
                self.__given = None
                self.__upper = None
                self.__op = CsrOperator.from_tensor(t, upper=True)
                return
            matrix = device_data.to_host(t)
        try:
            self.__given = matrix.csr()
        except Exception:
            self.__given = scs.csr_matrix(matrix)
        self.__upper = None
        self.__op = CsrOperator(self.__given, upper=True)

    def size(self):
        return self.__op.shape()[0]

    def data_type(self):
        return np.dtype(self.__op.data_type())

    def csr(self):
        """The upper triangle as SciPy CSR.  Of an operator built from a GPU tensor: one copy of the matrix to the
        host, made here on first use (only the direct factorisation asks for it)."""
        if self.__upper is None and self.__tensor is not None:
            self.__given = tensor_to_scipy(self.__tensor)
        if self.__upper is None:
            self.__upper = scs.triu(self.__given, format='csr')
            self.__upper.sort_indices()
        return self.__upper

    def nnz_full(self):
        return self.__op.nnz()

    def apply(self, x, y):
        if x.data_type() != self.__op.data_type() or y.data_type() != self.__op.data_type():
            raise ValueError('Matrix and vectors data types differ')
        if x.dimension() != self.size() or y.dimension() != self.size():
            raise ValueError('Matrix and vectors dimensions incompatible')
        if x.nvec() != y.nvec():
            raise ValueError('Numbers of input and output vectors differ')
        self.__op.apply_ptr(x.nvec(), x.data_ptr(), x.ld(), y.data_ptr(), y.ld())

    def cheb_step(self, y, p, b, cy, cp, cb):
        """Fused step of the three-term Chebyshev semi-iteration: p = cy y + cp p + cb (b - A y)."""
        self.__op.cheb_step_ptr(y.nvec(), y, p, b, cy, cp, cb)

    def cheb_step_bf16(self, m, y, p, b, cy, cp, cb):
        """The same step on bfloat16 blocks (Bf16Block), float32 arithmetic; float32 operators in
        the 1024-row windowed or the 256-row interleaved layout -- built on the host or from a GPU
        tensor -- and not in the sliced one (supports_bf16() tells; the library reports an error
        otherwise)."""
        self.__op.cheb_step_bf16(m, y, p, b, cy, cp, cb)

    def supports_bf16(self):
        return self.__op.bf16_ready()

    def layout(self):
        """Device layout of the operator and its stacked row blocks (diagnostics: CsrOperator.layout, .stacks)."""
        return self.__op.layout() + self.__op.stacks()


class Operator:
    """Wraps a user operator with ``apply(x, y)`` acting on device Vectors
    (raleigh/algebra/sparse_mkl.py:143-154 passes host arrays instead)."""

    def __init__(self, op):
        self.__op = op

    def apply(self, x, y):
        self.__op.apply(x, y)
