"""tests/fake_device_operator.py's stand-in library plus the six rlh_fsai_* entry points (the factorised sparse
approximate inverse) in NumPy / SciPy, with the checks, their order and the messages of the real library: TEST
INFRASTRUCTURE ONLY.  The local systems are solved by numpy.linalg in double; "device" pointers are host addresses."""

import ctypes

import numpy as np
import scipy.sparse as sp

from fake_lib import _DT, _addr, _block, _flat
import fake_device_operator
from fake_device_operator import as_device  # noqa: F401


def rsqrt_rounded(d):
    """d^(-1/2) correctly rounded to double: the longdouble value rounded, then moved to a neighbour where the exact
    comparison d m^2 <> 1 at the midpoint m says so (rounding twice, 64 then 53 bits, misses about one value in 2^11)."""
    from fractions import Fraction
    g = float(1 / np.sqrt(np.longdouble(d)))
    for _ in range(2):
        up, down = float(np.nextafter(g, np.inf)), float(np.nextafter(g, 0.0))
        if Fraction(d) * ((Fraction(g) + Fraction(up)) / 2) ** 2 < 1:
            g = up
        elif Fraction(d) * ((Fraction(g) + Fraction(down)) / 2) ** 2 > 1:
            g = down
        else:
            break
    return g


class _Fsai:
    def __init__(self, g, code, truncated):
        self.g, self.gh, self.code, self.truncated = g, sp.csr_matrix(g.conj().T), code, truncated


class FakeFsaiLib(fake_device_operator.FakeDeviceOperatorLib):

    def __init__(self):
        super().__init__()
        self._fsai = {}

    def _fsai_build(self, name, ph, code, n, ip, ix, va, max_row):
        if ip[0] != 0:
            return self._fail(name + ': indptr[0] must be 0')
        d = np.diff(ip)
        if np.any(d < 0):
            return self._fail(name + ': indptr decreases at row %d' % int(np.argmax(d < 0)))
        nnz = int(ip[-1])
        rows = np.repeat(np.arange(n), d)
        bad = (ix < 0) | (ix >= n)
        if bad.any():
            return self._fail(name + ': column index out of range in row %d' % int(rows[bad].min()))
        if nnz > 1:
            bad = (np.diff(ix) <= 0) & (rows[1:] == rows[:-1])
            if bad.any():
                return self._fail(name + ': the columns of row %d must ascend strictly (no duplicates)' % int(rows[1:][bad].min()))
        stored = set(zip(rows.tolist(), ix.tolist()))
        for i in range(n):
            if (i, i) not in stored:
                return self._fail(name + ': row %d does not store its diagonal entry' % i)
        for i, j in zip(rows.tolist(), ix.tolist()):
            if j < i and (j, i) not in stored:
                return self._fail(name + ': the stored structure is not symmetric: entry (%d, %d) has no partner (%d, %d); '
                                  'the device build creates no entries' % (i, j, j, i))
        wide = np.complex128 if np.dtype(_DT[code]).kind == 'c' else np.float64
        upper = rows <= ix                       # the upper triangle defines the matrix: nothing below it is read
        u = sp.csr_matrix((va[upper].astype(wide), (rows[upper], ix[upper])), shape=(n, n))
        full = sp.csr_matrix(u + sp.triu(u, k=1).conj().T)
        dense = full.toarray() if n <= 4096 else None
        gp, gi, gv, truncated = [0], [], [], 0
        for i in range(n):
            p = ix[ip[i]:ip[i + 1]]
            p = p[p <= i]
            if len(p) > max_row:
                truncated += 1
                p = p[-max_row:]
            k = len(p)
            s = dense[np.ix_(p, p)] if dense is not None else full[p][:, p].toarray()
            try:
                np.linalg.cholesky(s)
            except np.linalg.LinAlgError:
                return self._fail(name + ': local block of row %d is not positive definite' % i)
            if k == 1:
                g = np.array([rsqrt_rounded(float(s[0, 0].real))], dtype=wide)
            else:
                e = np.zeros(k, dtype=wide)
                e[-1] = 1
                y = np.linalg.solve(s, e)
                g = np.conj(y) / np.sqrt(y[-1].real)
                g[-1] = g[-1].real
            gi.extend(p.tolist())
            gv.extend(g.tolist())
            gp.append(len(gi))
        g = sp.csr_matrix((np.array(gv, dtype=wide).astype(_DT[code]), np.array(gi, dtype=np.int32),
                           np.array(gp, dtype=np.int64)), shape=(n, n))
        h = self._next_handle
        self._next_handle += 1
        self._fsai[h] = _Fsai(g, code, truncated)
        ph._obj.value = h
        return 0

    def _fsai_args(self, name, ph, code, n, indptr, max_row):
        ph._obj.value = None
        if code not in _DT:
            return self._fail(name + ': unknown dtype %d' % code)
        if not 0 <= n < 2 ** 31 - 1:
            return self._fail(name + ': the size must lie in [0, 2^31 - 1)')
        if not 1 <= max_row <= 64:
            return self._fail(name + ': max_row must lie in [1, 64], got %d' % max_row)
        if not _addr(indptr):
            return self._fail(name + ': null indptr')
        return 0

    def rlh_fsai_create_device(self, ph, code, n, index_bits, indptr, indices, values, max_row):
        self._count('fsai_create_device')
        name = 'rlh_fsai_create_device'
        if self._fsai_args(name, ph, code, n, indptr, max_row):
            return 1
        if index_bits not in (32, 64):
            return self._fail(name + ': index_bits must be 32 or 64, got %d' % index_bits)
        it = np.int32 if index_bits == 32 else np.int64
        ip = _flat(indptr, it, n + 1).astype(np.int64)
        nnz = max(int(ip[-1]), 0)
        return self._fsai_build(name, ph, code, n, ip, _flat(indices, it, nnz).astype(np.int64),
                                _flat(values, _DT[code], nnz).copy(), max_row)

    def rlh_fsai_create(self, ph, code, n, indptr, indices, values, max_row):
        self._count('fsai_create')
        name = 'rlh_fsai_create'
        if self._fsai_args(name, ph, code, n, indptr, max_row):
            return 1
        ip = _flat(indptr, np.int64, n + 1).copy()
        nnz = max(int(ip[-1]), 0)
        return self._fsai_build(name, ph, code, n, ip, _flat(indices, np.int32, nnz).astype(np.int64),
                                _flat(values, _DT[code], nnz).copy(), max_row)

    def rlh_fsai_destroy(self, h):
        self._fsai.pop(_addr(h), None)
        return 0

    def rlh_fsai_info(self, h, n, nnz, longest, truncated, nbytes, seconds):
        if not _addr(h):
            return self._fail('rlh_fsai_info: null handle')
        f = self._fsai[_addr(h)]
        es = np.dtype(_DT[f.code]).itemsize
        lens = np.diff(f.g.indptr)
        for p, v in ((n, f.g.shape[0]), (nnz, f.g.nnz), (longest, int(lens.max()) if lens.size else 0),
                     (truncated, f.truncated), (nbytes, 2 * f.g.nnz * (es + 4) + 16 * (f.g.shape[0] + 1))):
            if p is not None:
                ctypes.cast(p, ctypes.POINTER(ctypes.c_int64))[0] = v
        if seconds is not None:
            ctypes.cast(seconds, ctypes.POINTER(ctypes.c_double))[0] = 0.0
        return 0

    def rlh_fsai_get(self, h, indptr, indices, values):
        if not _addr(h):
            return self._fail('rlh_fsai_get: null handle')
        f = self._fsai[_addr(h)]
        n, nnz = f.g.shape[0], f.g.nnz
        _flat(indptr, np.int64, n + 1)[:] = f.g.indptr
        _flat(indices, np.int32, nnz)[:] = f.g.indices
        _flat(values, _DT[f.code], nnz)[:] = f.g.data
        return 0

    def rlh_fsai_apply(self, h, m, X, ldx, Y, ldy):
        self._count('fsai_apply')
        if not _addr(h):
            return self._fail('rlh_fsai_apply: null handle')
        f = self._fsai[_addr(h)]
        n = f.g.shape[0]
        if m < 0:
            return self._fail('rlh_fsai_apply: negative number of vectors')
        if m == 0 or n == 0:
            return 0
        if ldx < n or ldy < n:
            return self._fail('rlh_fsai_apply: Matrix and vectors dimensions incompatible')
        x = _block(X, f.code, n, m, ldx)
        w = np.asarray(f.g @ x.T).astype(_DT[f.code])
        _block(Y, f.code, n, m, ldy)[:, :] = np.asarray(f.gh @ w).T.astype(_DT[f.code])
        return 0


def install():
    from raleigh_amd import _lib
    fake = FakeFsaiLib()
    _lib.set_library(fake)
    return fake
