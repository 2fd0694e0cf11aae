"""8-bit data matrix bound to the MI355X backend: the counterpart of ``AMatrix`` (dense_matrix.py) for uint8 /
int8 data.  ``ByteAMatrix(a)`` takes a C-contiguous 2D ndarray of bytes and hands the interfaces
(truncated_svd, pca, LowerRankApproximation) a device operator (hip.ByteMatrix) with the products A X and
A^T Y on float32 vectors; the data are never widened, on the host or on the device.  There is no
``as_vectors()``: nothing in the interfaces needs the rows as vectors.  One GPU only: row-sharded 8-bit data
are not offered (dist.ShardedAMatrix refuses an array of bytes).
"""

import numpy as np

from .dense_matrix import _ACCEPTED, _DeviceHandle


class ByteAMatrix:

    def __init__(self, a, arch='hip'):
        if str(arch)[:3] not in _ACCEPTED:
            raise RuntimeError("raleigh_amd provides only arch='hip' (MI355X); got %r" % (arch,))
        from .hip import ByteMatrix
        self._arch = arch
        self._matrix = ByteMatrix(a)

    def as_operator(self):
        return self._matrix

    def gpu(self):
        return _DeviceHandle

    def arch(self):
        return self._arch

    def shape(self):
        return self._matrix.shape()

    def data_type(self):
        """float32: the type of the vectors and of every result."""
        return self._matrix.data_type()

    def dots(self):
        """Squared norms of the rows (exact integers as float64)."""
        return self._matrix.dots()

    def frobenius2(self):
        """Squared Frobenius norm (sum of the squared row norms)."""
        return float(np.sum(self.dots()))

    def scale(self):
        """Largest entry in modulus."""
        return self._matrix.absmax()
