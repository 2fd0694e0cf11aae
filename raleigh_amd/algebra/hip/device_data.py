"""Data that already lie in HBM as torch tensors: what the operators and the interfaces need to take them as they
stand and to hand their results back the same way.

``torch`` is imported only once an argument's type is seen to come from the torch module (``is_tensor``): the
package imports and runs without it.  A tensor on the bound GPU becomes an operator without a host trip (matrix.py,
byte_data.py, sparse_data.py borrow or copy it on the device) and the results come back as tensors on the same
device, copied device to device out of the Vectors; a CPU tensor is handed to the host path as an ndarray view or
a scipy.sparse.csr_matrix of its arrays.
"""

import numpy as np

from ... import _lib

_FLOATS = ('float32', 'float64', 'complex64', 'complex128')
_BYTES = ('uint8', 'int8')


def is_tensor(x):
    """True for a torch.Tensor; torch is imported only if x's type says it comes from there."""
    if (type(x).__module__ or '').split('.')[0] != 'torch':
        return False
    import torch
    return isinstance(x, torch.Tensor)


def _on_device(t):
    """Does the tensor lie in GPU memory?  (The one place that decides: the CPU test tier patches it so that CPU
    tensors stand for device tensors over the stand-in library, whose device pointers are host addresses.)"""
    return bool(t.is_cuda)


def is_device_tensor(x):
    return is_tensor(x) and _on_device(x)


def numpy_type(t):
    name = str(t.dtype).split('.')[-1]
    try:
        return np.dtype(name).type
    except TypeError:
        raise ValueError('data type %s not supported' % t.dtype)


def prepare(t):
    """Checks a tensor given as a data matrix and returns it ready for an operator: detached, conjugate / negative
    views resolved (one copy on its device), its stream synchronised once.  ValueError says what is not taken."""
    import torch
    if t.dim() != 2:
        raise ValueError('a 2D tensor is needed, got %d dimensions' % t.dim())
    name = str(t.dtype).split('.')[-1]
    if t.layout == torch.strided:
        if name not in _FLOATS + _BYTES:
            raise ValueError('data type %s not supported (float32, float64, complex64, complex128, uint8, int8)' % t.dtype)
    elif t.layout == torch.sparse_csr:
        if name not in _FLOATS:
            raise ValueError('data type %s not supported for sparse data (float32, float64, complex64, complex128)'
                             % t.dtype)
        if str(t.crow_indices().dtype).split('.')[-1] not in ('int32', 'int64'):
            raise ValueError('sparse index type %s not supported (int32, int64)' % t.crow_indices().dtype)
    else:
        raise ValueError('tensor layout %s not supported: torch.strided or torch.sparse_csr (use to_sparse_csr())'
                         % t.layout)
    if t.is_cuda:
        bound = _lib.local_device()
        index = t.device.index if t.device.index is not None else torch.cuda.current_device()
        if index != bound:
            raise ValueError('the tensor lies on GPU %d, the library is bound to GPU %d (one process per GPU)'
                             % (index, bound))
    if t.requires_grad:
        t = t.detach()
    if t.layout == torch.strided and (t.is_conj() or t.is_neg()):
        t = t.resolve_conj().resolve_neg()
    if t.is_cuda:
        torch.cuda.current_stream(t.device).synchronize()
    return t


def to_host(t):
    """A CPU tensor as what the host path takes: an ndarray view (zero-copy) or a scipy.sparse.csr_matrix."""
    import torch
    if t.layout == torch.sparse_csr:
        import scipy.sparse as scs
        return scs.csr_matrix((t.values().numpy(), t.col_indices().numpy(), t.crow_indices().numpy()),
                              shape=tuple(t.shape))
    return t.numpy()


def kind(t):
    """'dense', 'bytes' or 'sparse': the operator a prepared tensor goes to."""
    import torch
    if t.layout == torch.sparse_csr:
        return 'sparse'
    return 'bytes' if str(t.dtype).split('.')[-1] in _BYTES else 'dense'


def storage_room(t):
    """Bytes from the tensor's first element to the end of its storage."""
    return t.untyped_storage().nbytes() - t.storage_offset() * t.element_size()


def export(v, like, transpose=False):
    """The selected vectors of `v` as a tensor on `like`'s device -- shape (nvec, dim), or its transposed view
    (dim, nvec) as ``Vectors.data().T`` -- copied device to device (torch.empty + rlh_d2d / rlh_copy2d)."""
    import torch
    if v is None:
        return None
    m, n = v.nvec(), v.dimension()
    es = v.data_size()
    out = torch.empty((m, n), dtype=getattr(torch, np.dtype(v.data_type()).name), device=like.device)
    if out.is_cuda:                 # (the allocator may hand out a block that work on torch's stream still reads)
        torch.cuda.current_stream(out.device).synchronize()
    if m > 0 and n > 0:
        L = _lib.lib()
        if v.ld() == n:
            _lib.check(L.rlh_d2d(out.data_ptr(), v.data_ptr(), m * n * es))
        else:
            _lib.check(L.rlh_copy2d(out.data_ptr(), n * es, v.data_ptr(), v.ld() * es, n * es, m, 2))
    return out.T if transpose else out


def small(a, like):
    """A small host array the solver has fetched anyway (the singular values) as a tensor on `like`'s device."""
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=like.device)


def finish():
    """The library stream synchronised: what `export` wrote is then safe on any stream."""
    _lib.check(_lib.lib().rlh_sync())


def vectors_from(t, dtype=None, transpose=False):
    """Vectors holding the rows of a 2D device tensor (of its transpose if asked), as `dtype`: one device copy."""
    from .vectors import Vectors
    import torch
    t = t.detach()
    if transpose:
        t = t.T
    if dtype is not None:
        t = t.to(getattr(torch, np.dtype(dtype).name))
    t = t.resolve_conj().resolve_neg().contiguous()
    if t.is_cuda:
        torch.cuda.current_stream(t.device).synchronize()
    m, n = t.shape
    dt = numpy_type(t)
    v = Vectors(n, m, dt)
    if m > 0 and n > 0:
        es = t.element_size()
        _lib.check(_lib.lib().rlh_copy2d(v.data_ptr(), v.ld() * es, t.data_ptr(), n * es, n * es, m, 2))
        finish()                    # `t` may be a temporary: the copy has run before it goes
    return v
