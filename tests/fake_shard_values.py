"""tests/fake_fsai.py's stand-in library plus the new values of a row shard (rlh_shardvalues_pack, rlh_shardvalues_refill,
rlh_shardvalues_info: what csrc/fsai_apply.hip exports beyond tests/fake_fsai_apply.py) in NumPy, with the checks, their
order and the messages of the real library: TEST INFRASTRUCTURE ONLY.  "Device" pointers are host addresses.

A shard of the stand-in keeps G_loc and GH_loc as SciPy CSR matrices whose `data` lie in the order given to
rlh_fsshard_create, rounded to V and held in float64 / complex128: a refill writes that array, rounding as creation did."""

import ctypes

import numpy as np

from fake_lib import _DT, _addr, _flat
import fake_fsai
from fake_fsai_apply import put, wide_type


class FakeShardValuesLib(fake_fsai.FakeFsaiLib):

    def __init__(self):
        super().__init__()
        self._refills = {}

    def rlh_shardvalues_pack(self, h, first_row, count, d_pos, d_out):
        self._count('shardvalues_pack')
        name = 'rlh_shardvalues_pack'
        if not _addr(h):
            return self._fail(name + ': null handle')
        if count < 0:
            return self._fail(name + ': negative size')
        f = self._fsai[_addr(h)]
        n = f.g.shape[0]
        if not 0 <= first_row <= n:
            return self._fail(name + ': first row %d of a handle of %d rows' % (first_row, n))
        if count == 0:
            return 0
        if not _addr(d_pos) or not _addr(d_out):
            return self._fail(name + ': null pointer')
        base = int(f.g.indptr[first_row])
        entries = f.g.nnz - base
        pos = _flat(d_pos, np.int64, count)
        inside = (pos >= 0) & (pos < entries)
        out = _flat(d_out, _DT[f.code], count)
        out[:] = 0
        out[inside] = f.g.data[base + pos[inside]]
        return 0

    def rlh_shardvalues_refill(self, p, h, first_row, d_src, n_recv, d_recv):
        self._count('shardvalues_refill')
        name = 'rlh_shardvalues_refill'
        if not _addr(p):
            return self._fail(name + ': null plan')
        if not _addr(h):
            return self._fail(name + ': null handle')
        s, f = self._shards[_addr(p)], self._fsai[_addr(h)]
        n = f.g.shape[0]
        if s.code != f.code:
            return self._fail(name + ": the plan's dtype (%d) is not the handle's (%d)" % (s.code, f.code))
        if n_recv < 0:
            return self._fail(name + ': negative size')
        if first_row < 0 or n - first_row != s.n_own:
            return self._fail(name + ': the plan has %d own rows, the handle %d from row %d on' % (s.n_own, n - first_row, first_row))
        count = self._refills.get(_addr(p), 0)
        if s.n_own == 0:
            self._refills[_addr(p)] = count + 1
            return 0
        if not _addr(d_src) and s.gh.nnz:
            return self._fail(name + ': null source list')
        if not _addr(d_recv) and n_recv:
            return self._fail(name + ': null block of received values')
        base = int(f.g.indptr[first_row])
        entries = f.g.nnz - base
        if entries != s.g.nnz:
            return self._fail(name + ': the plan holds %d entries of G, the handle %d from row %d on' % (s.g.nnz, entries, first_row))
        other = np.flatnonzero(np.diff(s.g.indptr) != np.diff(f.g.indptr[first_row:]))
        if other.size:
            return self._fail(name + ': row %d of G has another length in the plan than in the handle' % other[0])
        src = _flat(d_src, np.int64, s.gh.nnz)
        bad = np.flatnonzero((src < -n_recv) | (src >= entries))
        if bad.size:
            return self._fail(name + ': entry %d of G^H has its source outside [-%d, %d)' % (bad[0], n_recv, entries))
        dt = np.dtype(_DT[f.code])
        wide = wide_type(dt)
        own = f.g.data[base:]
        recv = _flat(d_recv, dt, n_recv) if n_recv else np.zeros(0, dtype=dt)
        picked = np.where(src >= 0, own[np.maximum(src, 0)], recv[np.maximum(-1 - src, 0)] if n_recv else 0)
        s.g.data[:] = own.astype(s.v).astype(wide)
        s.gh.data[:] = np.conj(picked).astype(dt).astype(s.v).astype(wide)
        self._refills[_addr(p)] = count + 1
        return 0

    def rlh_shardvalues_info(self, p, updates, seconds):
        if not _addr(p):
            return self._fail('rlh_shardvalues_info: null plan')
        put(updates, ctypes.c_int64, self._refills.get(_addr(p), 0))
        put(seconds, ctypes.c_double, 0.0)
        return 0


def install():
    from raleigh_amd import _lib
    fake = FakeShardValuesLib()
    _lib.set_library(fake)
    return fake
