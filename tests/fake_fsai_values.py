"""tests/fake_fsai_shard.py's stand-in library plus the four rlh_fsvalues_* entry points (new matrix values on the
pattern an approximate inverse already has) in NumPy, with the checks, their order and the messages of the real library:
TEST INFRASTRUCTURE ONLY.  "Device" pointers are host addresses.

An update is the numeric phase of the stand-in's own build on the pattern the handle keeps: the checks of a build on the
new arrays without the partner check, the Hermitian matrix the upper triangle defines (a position it does not store is
zero), then `fake_fsai.solve_row` once per row on the kept columns, rounded to the storage type.  Nothing is committed
before every row has succeeded.  rlh_fsvalues_plan makes the plan's rounded copies again from the handle's G."""

import ctypes

import numpy as np
import scipy.sparse as sp

from fake_lib import _DT, _addr, _flat
import fake_csr_input
import fake_fsai
import fake_fsai_shard
from fake_fsai_work import stored_type
from fake_fsai import as_device  # noqa: F401


class FakeFsaiValuesLib(fake_fsai_shard.FakeFsaiShardLib):

    def _values_update(self, name, f, ip, ix, va, cap=None):
        """The checks on the arrays as they came, the solves, the commit.  cap: the entries the index and value arrays
        can hold (None: not known)."""
        n = f.g.shape[0]
        if msg := fake_csr_input.message(name + ': ', ip, ix, n, cap):
            return self._fail(msg)
        rows = np.repeat(np.arange(n), np.diff(ip))
        has_diag = np.zeros(n, dtype=bool)
        has_diag[rows[rows == ix]] = True
        if not has_diag.all():
            return self._fail(name + ': row %d does not store its diagonal entry' % int(np.argmin(has_diag)))
        wide = np.complex128 if np.dtype(_DT[f.code]).kind == 'c' else np.float64
        upper = rows <= ix                       # the upper triangle defines the matrix: nothing below it is read
        u = sp.csr_matrix((va[upper].astype(wide), (rows[upper], ix[upper])), shape=(n, n))
        full = sp.csr_matrix(u + sp.triu(u, k=1).conj().T)
        dense = full.toarray() if n <= 4096 else None
        g0, gv = f.g, []
        try:
            for i in range(n):
                p = g0.indices[g0.indptr[i]:g0.indptr[i + 1]].astype(np.int64)
                gv.extend(fake_fsai.solve_row(i, dense[np.ix_(p, p)] if dense is not None else full[p][:, p].toarray()).tolist())
        except fake_fsai._NotPd as e:
            return self._fail(name + ': local block of row %d is not positive definite' % e.args[0])
        g = sp.csr_matrix((np.array(gv, dtype=wide).astype(_DT[f.code]), g0.indices.copy(), g0.indptr.copy()), shape=(n, n))
        f.g, f.gh = g, sp.csr_matrix(g.conj().T)
        f.updates = getattr(f, 'updates', 0) + 1
        return 0

    def rlh_fsvalues_update_device(self, h, index_bits, indptr, indices, values):
        self._count('fsvalues_update_device')
        name = 'rlh_fsvalues_update_device'
        if not _addr(h):
            return self._fail(name + ': null handle')
        if not _addr(indptr):
            return self._fail(name + ': null indptr')
        if index_bits not in (32, 64):
            return self._fail(name + ': index_bits must be 32 or 64, got %d' % index_bits)
        f = self._fsai[_addr(h)]
        n = f.g.shape[0]
        if n == 0:
            f.updates = getattr(f, 'updates', 0) + 1
            return 0
        it = np.int32 if index_bits == 32 else np.int64
        ip = _flat(indptr, it, n + 1).astype(np.int64)
        nnz = max(int(ip[-1]), 0)
        if not _addr(indices) or not _addr(values):
            return self._values_update(name, f, ip, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=_DT[f.code]), cap=0)
        return self._values_update(name, f, ip, _flat(indices, it, nnz).astype(np.int64), _flat(values, _DT[f.code], nnz).copy())

    def rlh_fsvalues_update(self, h, indptr, indices, values):
        self._count('fsvalues_update')
        name = 'rlh_fsvalues_update'
        if not _addr(h):
            return self._fail(name + ': null handle')
        if not _addr(indptr):
            return self._fail(name + ': null indptr')
        f = self._fsai[_addr(h)]
        n = f.g.shape[0]
        ip = _flat(indptr, np.int64, n + 1).copy()
        if msg := fake_csr_input.indptr_message(name + ': ', ip):
            return self._fail(msg)
        nnz = int(ip[-1])
        if nnz and not (_addr(indices) and _addr(values)):
            return self._fail(name + ': null indices or values')
        if n == 0:
            f.updates = getattr(f, 'updates', 0) + 1
            return 0
        return self._values_update(name, f, ip, _flat(indices, np.int32, nnz).astype(np.int64), _flat(values, _DT[f.code], nnz).copy())

    def rlh_fsvalues_plan(self, p, h):
        self._count('fsvalues_plan')
        name = 'rlh_fsvalues_plan'
        if not _addr(p):
            return self._fail(name + ': null plan')
        if not _addr(h):
            return self._fail(name + ': null handle')
        plan, f = self._plans[_addr(p)], self._fsai[_addr(h)]
        n = f.g.shape[0]
        if plan.code != f.code:
            return self._fail(name + ": the plan's dtype (%d) is not the handle's (%d)" % (plan.code, f.code))
        if plan.n != n:
            return self._fail(name + ': the plan has %d rows, the handle %d' % (plan.n, n))
        if n == 0:
            return 0
        if plan.g.nnz != f.g.nnz:
            return self._fail(name + ': the plan holds %d entries of G, the handle %d' % (plan.g.nnz, f.g.nnz))
        for which, mine, its in (('G', plan.g, f.g), ('G^H', plan.gh, f.gh)):
            other = np.flatnonzero(np.diff(mine.indptr) != np.diff(its.indptr))
            if other.size:
                return self._fail(name + ': row %d of %s has another length in the plan than in the handle' % (other[0], which))
        wide = np.complex128 if np.dtype(_DT[f.code]).kind == 'c' else np.float64
        v = np.dtype(stored_type(np.dtype(_DT[f.code]), plan.work))
        plan.g = sp.csr_matrix(f.g.astype(v).astype(wide))
        plan.gh = sp.csr_matrix(plan.g.conj().T)
        return 0

    def rlh_fsvalues_info(self, h, updates, seconds):
        if not _addr(h):
            return self._fail('rlh_fsvalues_info: null handle')
        f = self._fsai[_addr(h)]
        if updates is not None:
            ctypes.cast(updates, ctypes.POINTER(ctypes.c_int64))[0] = getattr(f, 'updates', 0)
        if seconds is not None:
            ctypes.cast(seconds, ctypes.POINTER(ctypes.c_double))[0] = 0.0
        return 0


def install():
    from raleigh_amd import _lib
    fake = FakeFsaiValuesLib()
    _lib.set_library(fake)
    return fake
