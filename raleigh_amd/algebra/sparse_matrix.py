"""Sparse data matrix bound to the MI355X backend: the sparse counterpart of ``AMatrix``
(dense_matrix.py).  ``SparseAMatrix(a)`` takes any scipy.sparse matrix or array, converts it to
canonical CSR once and hands the interfaces (truncated_svd, pca, LowerRankApproximation) a device
operator (hip.SparseMatrix) with the products A X and A^H Y; the data are never densified.  There is no
``as_vectors()``: nothing in the interfaces needs the rows as vectors.
"""

import numpy as np

from .dense_matrix import _ACCEPTED, _DeviceHandle


class SparseAMatrix:

    def __init__(self, a, arch='hip'):
        if str(arch)[:3] not in _ACCEPTED:
            raise RuntimeError("raleigh_amd provides only arch='hip' (MI355X); got %r" % (arch,))
        from .hip import SparseMatrix
        self._arch = arch
        self._matrix = SparseMatrix(a)

    def as_operator(self):
        return self._matrix

    def gpu(self):
        return _DeviceHandle

    def arch(self):
        return self._arch

    def shape(self):
        return self._matrix.shape()

    def data_type(self):
        return self._matrix.data_type()

    def dots(self):
        """Squared norms of the rows."""
        return self._matrix.dots()

    def frobenius2(self):
        """Squared Frobenius norm (sum of the squared row norms)."""
        return float(np.sum(np.abs(self.dots())))

    def scale(self):
        """Largest entry in modulus."""
        return self._matrix.absmax()
