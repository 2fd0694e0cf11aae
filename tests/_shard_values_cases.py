"""New matrix values on a row shard's kept pattern (rlh_shardvalues_pack, rlh_shardvalues_refill, rlh_shardvalues_info,
ShardedApproximateInverse(updatable=True).update_values / update_local_rows): cases shared by the CPU tier
(tests/fake_shard_values.py) and the GPU tier.  Matrices, helpers and bounds come from tests/_fsai_shard_cases.py (`sc`) and
tests/_fsai_values_cases.py (`vc`); no tolerance is introduced here.

The raw-ABI cases run in ONE process without collectives: the test plays all the shards (`World`).  Shard s of a cut
matrix gets what ShardedApproximateInverse._setup gives a rank: a builder handle on A[E, E] (E: the lower rows its rows
reference, then its own rows), the plan of its rows of G and of G^H, per lower shard the positions of the entries sent to
it and for every entry of GH_loc its source.  After rlh_fsvalues_update_device on every builder the plan of a shard is
refilled from its own builder and from what rlh_shardvalues_pack made on the higher shards' builders, and must then
apply THE BITS of a plan that rlh_fsshard_create makes from the intended arrays (formed on the host from the fetched
builders) -- on the same x, x-halo block and W-halo block, so that every value of both layouts is read.  Nothing is
compared within a tolerance."""

import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import _fsai_cases as base
import _fsai_levels_cases as lv
import _fsai_shard_cases as sc
import _fsai_values_cases as vc
from _fsai_cases import _L, _check, dev, fetch, last_error
from _fsai_shard_cases import PAIRS, WORKS, bits, random_block, shard_create, w_row_bytes  # noqa: F401
from _fsai_values_cases import live, revalued

M = 11                                  # vectors of an application
BLOCKS_PER_CU = vc.BLOCKS_PER_CU        # the refill's kernels: 256 threads, at most 8 workgroups per CU, grid-stride loops;
ROWS_PER_BLOCK = vc.ROWS_PER_BLOCK      # one pass covers CU * 8 * 256 rows (the fills: 4 slices of 64 rows per workgroup) or entries


def refill_info(p):
    updates, sec = ctypes.c_int64(-1), ctypes.c_double(-1.0)
    _check(_L().rlh_shardvalues_info(p, ctypes.byref(updates), ctypes.byref(sec)))
    return updates.value, sec.value


def extended(A, cuts, s):
    """(below, A[E, E]) of shard s, as ShardedApproximateInverse._setup forms them."""
    r0, r1 = cuts[s], cuts[s + 1]
    loc = sp.csr_matrix(A[r0:r1])
    below = np.unique(loc.indices[loc.indices < r0]).astype(np.int64)
    E = np.concatenate([below, np.arange(r0, r1, dtype=np.int64)])
    a_ext = sp.csr_matrix(sp.csr_matrix(A[E])[:, E])
    a_ext.sort_indices()
    return below, E, a_ext


class World:
    """The builders of all shards of A cut at `cuts` (level-1 builds unless `config` says otherwise)."""

    def __init__(self, A, cuts, config=vc.LEVEL_1):
        self.dt, self.cuts, self.count = A.dtype, list(cuts), len(cuts) - 1
        self.ext = [extended(A, cuts, s) for s in range(self.count)]
        self.handles = [vc.made(a_ext, config, bits=32) for _, _, a_ext in self.ext]
        self.first = [int(below.size) for below, _, _ in self.ext]

    def update(self, B):
        for s in range(self.count):
            _check(vc.update(self.handles[s], extended(B, self.cuts, s)[2], bits=32))

    def own_entries(self, s):
        """(row pointers, global rows, global columns, values) of shard s's rows of G in the builder's order."""
        G = base.get(self.handles[s], self.dt.type)
        own = sp.csr_matrix(G[self.first[s]:])
        E = self.ext[s][1]
        gp = own.indptr.astype(np.int64)
        grow = np.repeat(np.arange(self.cuts[s], self.cuts[s + 1], dtype=np.int64), np.diff(gp))
        return gp, grow, E[own.indices], np.ascontiguousarray(own.data, dtype=self.dt)

    def shard(self, s):
        """What a rank keeps for shard s, from the builders' current values: dict with the arrays of rlh_fsshard_create (g,
        gh), the halo sizes, `moves` [(higher shard q, positions in q's entries)] and `source` for every entry of GH_loc."""
        r0, r1 = self.cuts[s], self.cuts[s + 1]
        n_own = r1 - r0
        gp, grow, gi, gv = self.own_entries(s)
        keep = gi >= r0
        x_ids = np.unique(gi[~keep])
        g_idx = np.where(keep, gi - r0, n_own + np.searchsorted(x_ids, gi)).astype(np.int32)
        parts, moves = [(grow[keep], gi[keep], gv[keep])], []
        for q in range(s + 1, self.count):
            _, qrow, qi, qv = self.own_entries(q)
            mine = (qi >= r0) & (qi < r1)
            if mine.any():
                moves.append((q, np.flatnonzero(mine).astype(np.int64)))
                parts.append((qrow[mine], qi[mine], qv[mine]))
        n_recv = sum(pos.size for _, pos in moves)
        hi, hj = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        hv = np.conj(np.concatenate([p[2] for p in parts])).astype(self.dt)
        order = np.lexsort((hi, hj))
        source = np.concatenate([np.flatnonzero(keep), -1 - np.arange(n_recv, dtype=np.int64)])[order].astype(np.int64)
        hi, hj, hv = hi[order], hj[order], np.ascontiguousarray(hv[order])
        hp = np.zeros(n_own + 1, dtype=np.int64)
        np.cumsum(np.bincount(hj - r0, minlength=n_own), out=hp[1:])
        inside = hi < r1
        w_ids = np.unique(hi[~inside])
        h_idx = np.where(inside, hi - r0, n_own + np.searchsorted(w_ids, hi)).astype(np.int32)
        return dict(n_own=n_own, n_xhalo=int(x_ids.size), n_whalo=int(w_ids.size), g=(gp, g_idx, gv), gh=(hp, h_idx, hv),
                    moves=moves, source=source, n_recv=n_recv)

    def plan(self, f, work):
        rc, p = shard_create(self.dt, WORKS[work], f['n_own'], f['n_xhalo'], f['n_whalo'], f['g'], f['gh'])
        assert rc == 0 and p.value, last_error()
        return p

    def packed(self, f):
        """The received block of shard f: rlh_shardvalues_pack on every higher shard's builder, in ascending order."""
        es = self.dt.itemsize
        recv = dev(np.full(max(f['n_recv'], 1), np.nan, dtype=self.dt))
        at = 0
        for q, pos in f['moves']:
            d_pos = dev(pos)
            _check(_L().rlh_shardvalues_pack(self.handles[q], self.first[q], pos.size, d_pos.ptr, recv.ptr + at * es))
            _check(_L().rlh_sync())
            at += pos.size
        return recv

    def refill(self, p, s, f, recv, first=None, source=None, n_recv=None):
        """rc of rlh_shardvalues_refill on shard s's builder with f's lists (or the given ones)."""
        src = dev(f['source'] if source is None else source)
        n_recv = f['n_recv'] if n_recv is None else n_recv
        return _L().rlh_shardvalues_refill(p, self.handles[s], self.first[s] if first is None else first, src.ptr, n_recv,
                                           recv.ptr if n_recv else None)

    def destroy(self):
        for h in self.handles:
            base.destroy(h)


def halo_block(rng, dt, work, tiles, count):
    """A W-halo block [tile][count][8] of Wt with finite values, as bytes."""
    x = rng.standard_normal(tiles * count * 8)
    if work == 'bf16':
        return (x.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16).view(np.uint8)
    wt = np.dtype(dt if work == 'native' else sc.stored_type(dt, work))
    if wt.kind == 'c':
        x = x + 1j * rng.standard_normal(x.size)
    return np.ascontiguousarray(x.astype(wt)).view(np.uint8)


def applied(p, dt, work, f, m=M):
    """The bits a plan of the sizes of f applies to a fixed x, x-halo block and W-halo block."""
    L, dt = _L(), np.dtype(dt)
    n_own, nx, nw = f['n_own'], f['n_xhalo'], f['n_whalo']
    rng = np.random.default_rng(31)
    X, XH = dev(random_block(rng, m, n_own, dt)), dev(random_block(rng, m, max(nx, 1), dt))
    WH = dev(halo_block(rng, dt, work, -(-m // 8), max(nw, 1)))
    Y = dev(np.full(m * n_own, np.nan, dtype=dt))
    _check(L.rlh_fsshard_first(p, m, X.ptr, n_own, XH.ptr if nx else None, max(nx, 1)))
    if nw:
        _check(L.rlh_fsshard_halo(p, m, 0, nw, WH.ptr))
    _check(L.rlh_fsshard_second(p, m, Y.ptr, n_own))
    _check(L.rlh_sync())
    y = fetch(Y, m * n_own, dt)
    assert np.all(np.isfinite(y))
    return bits(y).copy()


def refilled_is_fresh(A, B, cuts, work, shards=None, m=M, need_tail=False):
    """Every shard in `shards`: old bits before the refill, the bits of the fresh plan of the intended arrays after it."""
    W = World(A, cuts)
    made = []
    try:
        shards = range(W.count) if shards is None else shards
        old = {s: W.shard(s) for s in shards}
        plans = {s: W.plan(old[s], work) for s in shards}
        made.extend(plans.values())
        before = {s: applied(plans[s], A.dtype, work, old[s], m) for s in shards}
        W.update(B)
        mixed = False
        for s in shards:
            f = W.shard(s)
            for key in ('n_own', 'n_xhalo', 'n_whalo', 'n_recv'):
                assert f[key] == old[s][key]
            assert np.array_equal(f['source'], old[s]['source']) and np.array_equal(f['g'][1], old[s]['g'][1])
            assert not np.array_equal(bits(f['g'][2]), bits(old[s]['g'][2]))
            mixed = mixed or (np.any(f['source'] >= 0) and np.any(f['source'] < 0))
            if need_tail:
                assert sc.shard_info(plans[s])['tail'] > 0
            assert np.array_equal(applied(plans[s], A.dtype, work, f, m), before[s])     # not refilled: the old values
            assert refill_info(plans[s]) == (0, 0.0)
            recv = W.packed(f)
            held = live()
            assert W.refill(plans[s], s, f, recv) == 0, last_error()
            assert live() == held                                   # the scratch is gone
            got = refill_info(plans[s])
            assert got[0] == 1 and got[1] >= 0.0
            fresh = W.plan(f, work)
            made.append(fresh)
            new = applied(plans[s], A.dtype, work, f, m)
            assert np.array_equal(new, applied(fresh, A.dtype, work, f, m)) and not np.array_equal(new, before[s])
            info, info_fresh = sc.shard_info(plans[s]), sc.shard_info(fresh)
            assert (info['slots'], info['tail'], info['bytes']) == (info_fresh['slots'], info_fresh['tail'], info_fresh['bytes'])
            del recv
        assert mixed
    finally:
        for p in made:
            _L().rlh_fsshard_destroy(p)
        W.destroy()


# ---------------------------------------------------------------- 1. the main case
def three_shards(code, work):
    A = sc.global_matrix(base.TYPES[code], 500)
    refilled_is_fresh(A, revalued(A, 101), (0, 171, 339, 500), work)


# ---------------------------------------------------------------- 2. sizes
def small_shards(n_own, work):
    """A first shard of one row and a second of n_own rows with that row as its halo (_fsai_shard_cases.edges_small)."""
    n = n_own + 1
    A = base._with_profile(n, (1, 2, 9), np.float64, 60 + n)
    refilled_is_fresh(A, revalued(A, 102), (0, 1, n), work)


def long_rows(work):
    """The arrowhead matrix of _fsai_shard_cases.long_rows: row 0 of G^H holds n entries, 1049 of them received, most of
    them in the tail."""
    A = sc.arrowhead()
    n = A.shape[0]
    refilled_is_fresh(A, revalued(A, 103), (0, 1000, n), work, shards=(0,), m=3, need_tail=True)


def no_rows():
    """n_own = 0: a valid refill that does nothing, from a handle whose rows all lie below first_row."""
    A = lv.lap('d')
    n = A.shape[0]
    h = vc.made(A, vc.LEVEL_1)
    zero = np.zeros(1, dtype=np.int64)
    none = np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float64)
    rc, p = shard_create(np.float64, 0, 0, 0, 0, (zero,) + none, (zero,) + none)
    assert rc == 0, last_error()
    try:
        assert _L().rlh_shardvalues_refill(p, h, n, None, 0, None) == 0, last_error()
        assert refill_info(p)[0] == 1
        assert _L().rlh_shardvalues_pack(h, n, 0, None, None) == 0, last_error()
        assert _L().rlh_shardvalues_refill(p, h, n - 1, None, 0, None) != 0
        assert 'rlh_shardvalues_refill: the plan has 0 own rows, the handle 1 from row %d on' % (n - 1) in last_error()
    finally:
        _L().rlh_fsshard_destroy(p)
        base.destroy(h)


# ---------------------------------------------------------------- 3. the grid-stride loops past their first trip
def loops(rows):
    """A tridiagonal matrix cut (0, 64, 64 + rows, 128 + rows): the middle shard has `rows` own rows, one row below and one
    received entry.  On the GPU tier rows is one more than a whole pass of the refill's kernels."""
    n = rows + 128
    A = lv.band(np.full(n, 1), np.float64, 104)
    refilled_is_fresh(A, revalued(A, 105), (0, 64, 64 + rows, n), 'native', shards=(1,), m=1)


# ---------------------------------------------------------------- 4. refusals leave the plan as it was
def refusals():
    L = _L()
    A = sc.global_matrix(np.float64, 500)
    B = revalued(A, 106)
    cuts = (0, 171, 339, 500)
    name = 'rlh_shardvalues_refill'
    W = World(A, cuts)
    others, plans = [], []
    try:
        s = 1
        old = W.shard(s)
        p = W.plan(old, 'native')
        plans.append(p)
        before = applied(p, A.dtype, 'native', old)
        W.update(B)
        f = W.shard(s)
        recv = W.packed(f)
        z = vc.made(base.matrix('z'), vc.LEVEL_1)
        others.append(z)
        src, pos, out = dev(f['source']), dev(np.zeros(4, dtype=np.int64)), dev(np.zeros(4))
        level = live()
        entries, n_recv = int(f['g'][1].size), f['n_recv']
        assert n_recv > 0

        def refused(text, rc):
            assert rc != 0, text
            assert '%s: %s' % (name, text) in last_error(), (text, last_error())
            assert live() == level and refill_info(p) == (0, 0.0)
            assert np.array_equal(applied(p, A.dtype, 'native', old), before)

        def changed(k, v):
            src = f['source'].copy()
            src[k] = v
            return src
        first = W.first[s]
        n_ext = first + f['n_own']
        refused('the plan has %d own rows, the handle %d from row %d on' % (f['n_own'], n_ext - first - 1, first + 1),
                W.refill(p, s, f, recv, first=first + 1))
        refused('the plan has %d own rows, the handle %d from row -1 on' % (f['n_own'], n_ext + 1), W.refill(p, s, f, recv, first=-1))
        # a row of another length with the same number of entries; then another number of entries
        gp, g_idx, gv = old['g']
        lens = np.diff(gp)
        r = int(np.flatnonzero(lens[:-1] >= 2)[3])
        moved = gp.copy()
        moved[r + 1] -= 1                                           # row r gives its last entry to row r + 1
        fewer = (gp.copy(), g_idx[:-1], gv[:-1])
        fewer[0][-1] -= 1
        for arrays, text in (((moved, g_idx, gv), 'row %d of G has another length in the plan than in the handle' % r),
                             (fewer, 'the plan holds %d entries of G, the handle %d from row %d on' % (entries - 1, entries, first))):
            q = W.plan(dict(old, g=arrays), 'native')
            plans.append(q)
            was = applied(q, A.dtype, 'native', old)
            held = live()
            rc = W.refill(q, s, f, recv)
            assert rc != 0 and '%s: %s' % (name, text) in last_error(), last_error()
            assert live() == held and refill_info(q) == (0, 0.0) and np.array_equal(applied(q, A.dtype, 'native', old), was)
            L.rlh_fsshard_destroy(plans.pop())
        assert live() == level
        # the sources
        k = int(f['source'].size // 2)
        refused('entry %d of G^H has its source outside [-%d, %d)' % (k, n_recv, entries), W.refill(p, s, f, recv, source=changed(k, entries)))
        refused('entry 0 of G^H has its source outside [-%d, %d)' % (n_recv, entries), W.refill(p, s, f, recv, source=changed(0, -n_recv - 1)))
        two = changed(k, entries)
        two[k + 5] = -n_recv - 7
        refused('entry %d of G^H has its source outside' % k, W.refill(p, s, f, recv, source=two))
        # dtype, nulls
        refused("the plan's dtype", L.rlh_shardvalues_refill(p, z, 0, src.ptr, n_recv, recv.ptr))
        refused('null plan', L.rlh_shardvalues_refill(None, W.handles[s], first, src.ptr, n_recv, recv.ptr))
        refused('null handle', L.rlh_shardvalues_refill(p, None, first, src.ptr, n_recv, recv.ptr))
        refused('null source list', L.rlh_shardvalues_refill(p, W.handles[s], first, None, n_recv, recv.ptr))
        refused('null block of received values', L.rlh_shardvalues_refill(p, W.handles[s], first, src.ptr, n_recv, None))
        refused('negative size', L.rlh_shardvalues_refill(p, W.handles[s], first, src.ptr, -1, recv.ptr))
        assert L.rlh_shardvalues_info(None, None, None) != 0 and 'rlh_shardvalues_info: null plan' in last_error()
        for call, text in ((lambda: L.rlh_shardvalues_pack(None, 0, 4, pos.ptr, out.ptr), 'null handle'),
                           (lambda: L.rlh_shardvalues_pack(W.handles[s], 0, -1, pos.ptr, out.ptr), 'negative size'),
                           (lambda: L.rlh_shardvalues_pack(W.handles[s], n_ext + 1, 4, pos.ptr, out.ptr),
                            'first row %d of a handle of %d rows' % (n_ext + 1, n_ext)),
                           (lambda: L.rlh_shardvalues_pack(W.handles[s], 0, 4, None, out.ptr), 'null pointer'),
                           (lambda: L.rlh_shardvalues_pack(W.handles[s], 0, 4, pos.ptr, None), 'null pointer')):
            assert call() != 0 and 'rlh_shardvalues_pack: ' + text in last_error(), (text, last_error())
        # after all that a good refill works
        assert W.refill(p, s, f, recv) == 0, last_error()
        assert refill_info(p)[0] == 1 and live() == level
        fresh = W.plan(f, 'native')
        plans.append(fresh)
        assert np.array_equal(applied(p, A.dtype, 'native', f), applied(fresh, A.dtype, 'native', f))
    finally:
        for p in plans:
            L.rlh_fsshard_destroy(p)
        for h in others:
            base.destroy(h)
        W.destroy()


# ---------------------------------------------------------------- 5. the contract of pack
def pack_contract():
    A = sc.global_matrix(np.complex128, 500)
    cuts = (0, 171, 339, 500)
    W = World(A, cuts)
    try:
        s = 2
        _, _, _, gv = W.own_entries(s)
        first, entries = W.first[s], gv.size
        pos = np.array([0, entries - 1, entries, -1, 7, 2 ** 40, -2 ** 40, 3], dtype=np.int64)
        out, d_pos = dev(np.full(pos.size, np.nan, dtype=A.dtype)), dev(pos)
        _check(_L().rlh_shardvalues_pack(W.handles[s], first, pos.size, d_pos.ptr, out.ptr))
        _check(_L().rlh_sync())
        got = fetch(out, pos.size, A.dtype)
        inside = (pos >= 0) & (pos < entries)
        want = np.where(inside, gv[np.where(inside, pos, 0)], 0)
        assert np.array_equal(bits(got), bits(want.astype(A.dtype)))
        # from the first row on: the positions count the handle's entries
        whole = base.get(W.handles[s], A.dtype.type)
        _check(_L().rlh_shardvalues_pack(W.handles[s], 0, pos.size, d_pos.ptr, out.ptr))
        _check(_L().rlh_sync())
        inside = (pos >= 0) & (pos < whole.nnz)
        want = np.where(inside, whole.data[np.where(inside, pos, 0)], 0)
        assert np.array_equal(bits(fetch(out, pos.size, A.dtype)), bits(want.astype(A.dtype)))
    finally:
        W.destroy()


# ---------------------------------------------------------------- 6. device memory (GPU tier)
def device_memory_class(comm):
    """live() is the same before and after an update, and at its starting level once the updatable object is gone."""
    import gc
    from raleigh_amd.algebra.hip.dist import ShardedApproximateInverse
    A = sc.global_matrix(np.float64, 500)
    gc.collect()                                                  # (what earlier cases left in reference cycles goes now, not below)
    first = live()
    T = ShardedApproximateInverse(A, comm, levels=2, updatable=True)
    plain = ShardedApproximateInverse(A, comm, levels=2)
    assert T.device_bytes() > plain.device_bytes()
    del plain
    gc.collect()
    held = live()
    for k in range(2):
        T.update_values(revalued(A, 130 + k))
        assert live() == held
    del T
    gc.collect()
    assert live() == first, (live(), first, held)


# ---------------------------------------------------------------- the class, on a process group
N_CLASS = 500
CLASS_TYPES = (np.float64, np.complex128)


def _applied_class(T, A, comm, off):
    from raleigh_amd.algebra.hip.dist import ShardedVectors
    x = random_block(np.random.default_rng(57), M, A.shape[0], A.dtype)
    X = ShardedVectors(x, comm=comm, offsets=off)
    Y = X.new_vectors(M)
    T.apply(X, Y)
    return bits(Y.data()).copy()


def _same_csr(a, b):
    return np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and np.array_equal(bits(a.data), bits(b.data))


def class_levels(A, comm, off, single_work=None, works=('native',)):
    """(a) and (d): level patterns -- after an update G and the application are those of a fresh object on the same
    partition, bit for bit, by either entry form; at level 1 the rows are those of the single-process build."""
    from raleigh_amd.algebra.hip.dist import ShardedApproximateInverse
    from raleigh_amd.algebra.hip.precond import ApproximateInverse
    from raleigh_amd.algebra.hip.sparse import full_from_upper
    B = revalued(A, 110)
    r0, r1 = int(off[comm.rank]), int(off[comm.rank + 1])
    for levels in (1, 2):
        for work in works:
            T = ShardedApproximateInverse(A, comm, offsets=off, levels=levels, work=work, updatable=True)
            assert (T.updates, T.update_seconds) == (0, 0.0) and T.updatable
            G0, y0 = T.csr(), _applied_class(T, A, comm, off)
            kept = (T.nnz, T.fill, T.longest_row, T.dropped_entries, T.setup_seconds, T.halo_rows())
            fresh = ShardedApproximateInverse(B, comm, offsets=off, levels=levels, work=work)
            want, y_want = fresh.csr(), _applied_class(fresh, B, comm, off)
            T.update_values(B)
            assert T.updates == 1 and T.update_seconds > 0.0
            assert _same_csr(T.csr(), want) and not _same_csr(T.csr(), G0)
            y = _applied_class(T, B, comm, off)
            assert np.array_equal(y, y_want) and not np.array_equal(y, y0)
            assert _same_csr(sc.gathered_csr(T, comm), sc.gathered_csr(fresh, comm))
            assert (T.nnz, T.fill, T.longest_row, T.dropped_entries, T.setup_seconds, T.halo_rows()) == kept
            if levels == 1:
                whole = ApproximateInverse(B, work=single_work).csr()
                assert _same_csr(T.csr(), sp.csr_matrix(whole[r0:r1, :]))
            # (d) back to A by this rank's rows, on an object made from them
            rows = sp.csr_matrix(full_from_upper(A)[r0:r1, :])
            T.update_local_rows(rows)
            assert T.updates == 2 and _same_csr(T.csr(), G0) and np.array_equal(_applied_class(T, A, comm, off), y0)
            U = ShardedApproximateInverse.from_local_rows(rows, r0, A.shape[0], comm, off, levels=levels, work=work, updatable=True)
            U.update_local_rows(sp.csr_matrix(full_from_upper(B)[r0:r1, :]))
            assert _same_csr(U.csr(), want) and np.array_equal(_applied_class(U, B, comm, off), y_want)


def class_by_value(A, comm, off):
    """(b): patterns chosen by value -- the pattern stays, every row has the defining property for A' on it."""
    from raleigh_amd.algebra.hip.dist import ShardedApproximateInverse
    B = revalued(A, 111)
    for kw in (dict(steps=2, step_size=2), dict(drop=0.1)):
        T = ShardedApproximateInverse(A, comm, offsets=off, updatable=True, **kw)
        G0 = sc.gathered_csr(T, comm)
        T.update_values(B)
        G = sc.gathered_csr(T, comm)
        assert np.array_equal(G.indptr, G0.indptr) and np.array_equal(G.indices, G0.indices) and not np.array_equal(bits(G.data), bits(G0.data))
        vc.check_all(G, G0, vc.wide_dense(B), A.dtype.type)
        assert T.updates == 1 and (T.steps, T.drop) == (kw.get('steps', 0), kw.get('drop', 0.0))


def class_refused(A, comm, off):
    """(c): A' is not positive definite in the LAST rank's block only; every rank raises, nothing changes; then a good
    update works.  Size and type are refused before anything else."""
    from raleigh_amd import _lib
    from raleigh_amd.algebra.hip.dist import ShardedApproximateInverse
    T = ShardedApproximateInverse(A, comm, offsets=off, levels=2, updatable=True)
    G0, y0 = T.csr(), _applied_class(T, A, comm, off)
    B = revalued(A, 112)
    C = B.copy().tolil()
    i = A.shape[0] - 20
    C[i, i] = -3.0
    C = sp.csr_matrix(C).astype(A.dtype)
    C.sort_indices()
    last = comm.size - 1
    assert i >= int(off[last])
    if comm.rank == last:
        with pytest.raises(_lib.RlhError, match='local block of row %d is not positive definite' % (i - int(off[last]) + T._below.size)):
            T.update_values(C)
    else:
        with pytest.raises(RuntimeError, match='rank %d refused the new matrix' % last):
            T.update_values(C)
    assert T.updates == 0 and _same_csr(T.csr(), G0) and np.array_equal(_applied_class(T, A, comm, off), y0)
    with pytest.raises(ValueError, match='built for a matrix of size %d' % A.shape[0]):
        T.update_values(sp.csr_matrix(A[:400, :400]))
    with pytest.raises(ValueError, match='built for a matrix of type'):
        T.update_values(A.astype(np.complex64))
    with pytest.raises(ValueError, match='got rows of shape'):
        T.update_local_rows(sp.csr_matrix(A[:3]))
    assert T.updates == 0 and _same_csr(T.csr(), G0) and np.array_equal(_applied_class(T, A, comm, off), y0)
    T.update_values(B)
    fresh = ShardedApproximateInverse(B, comm, offsets=off, levels=2)
    assert T.updates == 1 and _same_csr(T.csr(), fresh.csr()) and np.array_equal(_applied_class(T, B, comm, off), _applied_class(fresh, B, comm, off))


def class_not_updatable(A, comm, off):
    from raleigh_amd.algebra.hip.dist import ShardedApproximateInverse
    T = ShardedApproximateInverse(A, comm, offsets=off)
    assert not T.updatable and (T.updates, T.update_seconds) == (0, 0.0)
    with pytest.raises(RuntimeError, match='updatable=True'):
        T.update_values(A)
    with pytest.raises(RuntimeError, match='updatable=True'):
        T.update_local_rows(A)
