"""tests/fake_fsai_filter.py's stand-in library (a FakeFsaiWorkLib with post-filtration) plus the seven rlh_fsshard_*
entry points (the approximate inverse's application on a row shard) in NumPy, with the checks, their order and the
messages of the real library: TEST INFRASTRUCTURE ONLY.  "Device" pointers are host addresses.

The rounding model is that of tests/fake_fsai_work.py: the values of G_loc and GH_loc rounded once to V; W = G~_loc [X ;
XH] formed in float64 / complex128 and rounded once to Wt; Y = G~H_loc W formed in float64 / complex128 and rounded to T.
W is kept as the library keeps it, [tile][n_own + n_whalo][8] of Wt (bfloat16 as its 16 bits), so that what
rlh_fsshard_pack writes and rlh_fsshard_halo reads are the bytes that travel; the halo rows start as NaN (bfloat16:
0x7fc0) at every rlh_fsshard_first.  rlh_fsshard_pack checks its indices, which here lie in host memory."""

import ctypes

import numpy as np
import scipy.sparse as sp

from fake_lib import _DT, _addr, _block, _flat
import fake_fsai_filter
from fake_fsai_work import bf16_round, layout_counts, stored_type
from fake_fsai import as_device  # noqa: F401


class _Shard:
    def __init__(self, code, work, n_own, n_xhalo, n_whalo, g, gh):
        self.code, self.work, self.n_own, self.n_xhalo, self.n_whalo = code, work, n_own, n_xhalo, n_whalo
        dt = np.dtype(_DT[code])
        self.v = np.dtype(stored_type(dt, work))
        self.g, self.gh = g, gh                            # V values held in float64 / complex128
        self.wt = np.dtype(np.uint16) if work == 2 else (dt if work == 0 else self.v)
        self.slots = self.tail = 0
        if n_own:
            for mat in (g, gh):
                a, b = layout_counts(np.diff(mat.indptr))
                self.slots, self.tail = self.slots + a, self.tail + b
        self.w, self.w_bytes = None, 0
        self.m_first, self.placed = -1, 0

    def encode(self, w):
        """(rows, 8 * tiles) wide values -> [tile][row][8] of Wt."""
        rows = w.shape[0]
        if self.work == 2:
            stored = (bf16_round(w).view(np.uint32) >> 16).astype(np.uint16).reshape(w.shape)
        else:
            stored = w.astype(self.wt)
        return np.ascontiguousarray(stored.reshape(rows, w.shape[1] // 8, 8).transpose(1, 0, 2))

    def decode(self, stored):
        """[tile][row][8] of Wt -> (rows, 8 * tiles) wide values."""
        if self.work == 2:
            stored = (stored.astype(np.uint32) << 16).view(np.float32)
        return stored.transpose(1, 0, 2).reshape(stored.shape[1], 8 * stored.shape[0]).astype(self.g.dtype)


class FakeFsaiShardLib(fake_fsai_filter.FakeFsaiFilterLib):

    def __init__(self):
        super().__init__()
        self._shards = {}

    def rlh_fsshard_create(self, pp, code, work, n_own, n_xhalo, n_whalo, g_indptr, g_indices, g_values, gh_indptr, gh_indices,
                           gh_values):
        self._count('fsshard_create')
        name = 'rlh_fsshard_create'
        if pp is None:
            return self._fail(name + ': null plan pointer')
        pp._obj.value = None
        if code not in _DT:
            return self._fail(name + ': unknown dtype %d' % code)
        if work not in (0, 1, 2):
            return self._fail(name + ': work must be 0 (native), 1 (float32) or 2 (bf16), got %d' % work)
        dt = np.dtype(_DT[code])
        if work == 2 and dt.kind == 'c':
            return self._fail(name + ': bfloat16 work blocks are for real types only')
        if n_own < 0 or n_xhalo < 0 or n_whalo < 0:
            return self._fail(name + ': negative size')
        if not _addr(g_indptr) or not _addr(gh_indptr):
            return self._fail(name + ': null indptr')
        ptrs = []
        for which, indptr in (('G', g_indptr), ('G^H', gh_indptr)):
            ip = _flat(indptr, np.int64, n_own + 1).copy()
            down = np.flatnonzero(np.diff(ip) < 0)
            if ip[0] != 0 or down.size:
                return self._fail(name + ': indptr of %s must start at 0 and not decrease (row %d)'
                                  % (which, 0 if ip[0] != 0 else down[0]))
            ptrs.append(ip)
        if (ptrs[0][-1] and not (_addr(g_indices) and _addr(g_values))) or (ptrs[1][-1] and not (_addr(gh_indices) and _addr(gh_values))):
            return self._fail(name + ': null indices or values')
        wide = np.complex128 if dt.kind == 'c' else np.float64
        v = np.dtype(stored_type(dt, work))
        mats = []
        for which, ip, indices, values, halo in (('G', ptrs[0], g_indices, g_values, n_xhalo), ('G^H', ptrs[1], gh_indices, gh_values, n_whalo)):
            nnz = int(ip[-1])
            ix = _flat(indices, np.int32, nnz).copy()
            va = _flat(values, dt, nnz).astype(v).astype(wide)
            rows = np.repeat(np.arange(n_own), np.diff(ip))
            bad = rows[(ix < 0) | (ix >= n_own + halo)]
            if n_own and bad.size:
                return self._fail(name + ': broken layout of %s: column index out of range in row %d' % (which, bad.min()))
            mats.append(sp.csr_matrix((va, ix, ip), shape=(n_own, n_own + halo)))
        p = self._next_handle
        self._next_handle += 1
        self._shards[p] = _Shard(code, work, n_own, n_xhalo, n_whalo, *mats)
        pp._obj.value = p
        return 0

    def rlh_fsshard_first(self, p, m, X, ldx, XH, ldxh):
        self._count('fsshard_first')
        name = 'rlh_fsshard_first'
        if not _addr(p):
            return self._fail(name + ': null plan')
        s = self._shards[_addr(p)]
        if m < 0:
            return self._fail(name + ': negative number of vectors')
        if m > 0 and s.n_own > 0:
            if not _addr(X):
                return self._fail(name + ': null pointer')
            if not _addr(XH) and s.n_xhalo:
                return self._fail(name + ': null halo block with %d halo rows' % s.n_xhalo)
            if ldx < s.n_own or (_addr(XH) and ldxh < s.n_xhalo):
                return self._fail(name + ': Matrix and vectors dimensions incompatible')
        s.m_first, s.placed = -1, 0
        if m > 0:
            tiles, wrows = -(-m // 8), s.n_own + s.n_whalo
            wide = s.g.dtype
            w = np.full((wrows, tiles * 8), np.nan, dtype=wide)
            if s.n_own:
                x = _block(X, s.code, s.n_own, m, ldx).T.astype(wide)
                if s.n_xhalo:
                    x = np.vstack([x, _block(XH, s.code, s.n_xhalo, m, ldxh).T.astype(wide)])
                with np.errstate(invalid='ignore', over='ignore'):
                    w[:s.n_own, :m] = np.asarray(s.g @ x)
                w[:s.n_own, m:] = 0
            with np.errstate(invalid='ignore', over='ignore'):
                s.w = s.encode(w)
            s.w_bytes = max(s.w_bytes, s.w.nbytes)
        s.m_first = m
        return 0

    def rlh_fsshard_pack(self, p, m, nidx, d_idx, out):
        self._count('fsshard_pack')
        name = 'rlh_fsshard_pack'
        if not _addr(p):
            return self._fail(name + ': null plan')
        s = self._shards[_addr(p)]
        if m < 0 or nidx < 0:
            return self._fail(name + ': negative size')
        if nidx > s.n_own:
            return self._fail(name + ': %d rows asked of %d own rows' % (nidx, s.n_own))
        if s.m_first != m:
            return self._fail(name + ': no rlh_fsshard_first with %d vectors came before' % m)
        if m == 0 or nidx == 0:
            return 0
        if not _addr(d_idx) or not _addr(out):
            return self._fail(name + ': null pointer')
        idx = _flat(d_idx, np.int64, nidx)
        if idx.min() < 0 or idx.max() >= s.n_own:
            return self._fail(name + ': row index out of range')
        tiles = s.w.shape[0]
        _flat(out, s.wt, tiles * nidx * 8).reshape(tiles, nidx, 8)[:] = s.w[:, idx, :]
        return 0

    def rlh_fsshard_halo(self, p, m, first, count, src):
        self._count('fsshard_halo')
        name = 'rlh_fsshard_halo'
        if not _addr(p):
            return self._fail(name + ': null plan')
        s = self._shards[_addr(p)]
        if m < 0 or first < 0 or count < 0:
            return self._fail(name + ': negative size')
        if first + count > s.n_whalo:
            return self._fail(name + ': rows %d .. %d of %d halo rows' % (first, first + count, s.n_whalo))
        if s.m_first != m:
            return self._fail(name + ': no rlh_fsshard_first with %d vectors came before' % m)
        if m > 0 and count > 0:
            if not _addr(src):
                return self._fail(name + ': null pointer')
            tiles = s.w.shape[0]
            s.w[:, s.n_own + first:s.n_own + first + count, :] = _flat(src, s.wt, tiles * count * 8).reshape(tiles, count, 8)
        s.placed += count
        return 0

    def rlh_fsshard_second(self, p, m, Y, ldy):
        self._count('fsshard_second')
        name = 'rlh_fsshard_second'
        if not _addr(p):
            return self._fail(name + ': null plan')
        s = self._shards[_addr(p)]
        if m < 0:
            return self._fail(name + ': negative number of vectors')
        if s.m_first < 0:
            return self._fail(name + ': no rlh_fsshard_first came before')
        if s.m_first != m:
            return self._fail(name + ': the last rlh_fsshard_first had %d vectors, not %d' % (s.m_first, m))
        if s.placed < s.n_whalo:
            return self._fail(name + ': halo rows missing (%d of %d placed)' % (s.placed, s.n_whalo))
        if m == 0 or s.n_own == 0:
            return 0
        if not _addr(Y):
            return self._fail(name + ': null pointer')
        if ldy < s.n_own:
            return self._fail(name + ': Matrix and vectors dimensions incompatible')
        with np.errstate(invalid='ignore', over='ignore'):
            y = np.asarray(s.gh @ s.decode(s.w))[:, :m]
            _block(Y, s.code, s.n_own, m, ldy)[:, :] = y.T.astype(_DT[s.code])
        return 0

    def rlh_fsshard_info(self, p, work, slots, tail, nbytes, w_row_bytes):
        if not _addr(p):
            return self._fail('rlh_fsshard_info: null plan')
        s = self._shards[_addr(p)]
        n = s.n_own
        held = s.w_bytes
        if n:
            held += (s.slots + s.tail) * (4 + s.v.itemsize) + 2 * (12 * n + 8 + 12 * (-(-n // 64) + 1))
        if work is not None:
            ctypes.cast(work, ctypes.POINTER(ctypes.c_int))[0] = s.work
        for ptr, v in ((slots, s.slots), (tail, s.tail), (nbytes, held), (w_row_bytes, 8 * s.wt.itemsize)):
            if ptr is not None:
                ctypes.cast(ptr, ctypes.POINTER(ctypes.c_int64))[0] = v
        return 0

    def rlh_fsshard_destroy(self, p):
        self._shards.pop(_addr(p), None)
        return 0


def install():
    from raleigh_amd import _lib
    fake = FakeFsaiShardLib()
    _lib.set_library(fake)
    return fake
