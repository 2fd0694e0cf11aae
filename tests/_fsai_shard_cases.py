"""The approximate inverse on row-sharded blocks (rlh_fsshard_*, ShardedApproximateInverse): cases shared by the CPU tier
(tests/fake_fsai.py) and the GPU tier.  Matrices, helpers and the bound of an application come from
tests/_fsai_work_cases.py and tests/_fsai_cases.py.

The raw-ABI cases run in ONE process without collectives: the test plays all the shards.  G is the level-1 build of the
whole matrix; shard s owns the rows [cut[s], cut[s + 1]) and gets G_loc (those rows of G; a column below cut[s] is a
row of its x-halo block) and GH_loc (those rows of G^H, conjugated; a column from cut[s + 1] on is a halo row of W),
both in ascending global column order.  One application is the choreography of ShardedApproximateInverse.apply: the
x-halo rows by rlh_gather_rows from the whole block, rlh_fsshard_first on every shard, the halo rows of W by
rlh_fsshard_pack on the owner's plan -> rlh_fsshard_halo, rlh_fsshard_second on every shard.

THE BOUND is the one derived in tests/_fsai_work_cases.py, ((a + b + 2) uT' + 2 uW') |G~|^H |G~| |X| with a and b the
longest row of the GLOBAL G and G^H: a shard's row of G_loc is a row of G and its row of GH_loc a row of G^H, summed in
a fixed order of their own, and W is rounded once wherever it was computed; packing and placing move bits.
"""

import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from _fsai_cases import N, TYPES, _L, _check, _with_profile, create, destroy, dev, fetch, get, last_error, matrix
from _fsai_work_cases import (GUARD, PAIRS, VECTORS, WORKS, Reference, arrowhead, bits, padded, random_block, run,  # noqa: F401
                              stored_type, with_plan)


def _code(dt):
    from raleigh_amd import _lib
    return _lib.DTYPE_CODE[np.dtype(dt).type]


def _ptr(a):
    from raleigh_amd import _lib
    return _lib.host_ptr(a)


# ---------------------------------------------------------------- the raw entry points
def shard_create(dt, work, n_own, n_xhalo, n_whalo, g, gh):
    """(rc, plan); g, gh: (indptr, indices, values) host arrays (None: a null pointer)."""
    p = ctypes.c_void_p(12345)
    args = [None if a is None else _ptr(a) for a in tuple(g) + tuple(gh)]
    return _L().rlh_fsshard_create(ctypes.byref(p), _code(dt), work, n_own, n_xhalo, n_whalo, *args), p


def shard_info(p):
    work, slots, tail, nbytes, wrb = (ctypes.c_int(-1), ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_int64(-1),
                                      ctypes.c_int64(-1))
    _check(_L().rlh_fsshard_info(p, ctypes.byref(work), ctypes.byref(slots), ctypes.byref(tail), ctypes.byref(nbytes),
                                 ctypes.byref(wrb)))
    return dict(work=work.value, slots=slots.value, tail=tail.value, bytes=nbytes.value, w_row_bytes=wrb.value)


def w_row_bytes(dt, work):
    if work == 'bf16':
        return 16
    return 8 * np.dtype(dt if work == 'native' else stored_type(dt, work)).itemsize


class Shard:
    """One shard's arrays and plan; extra: x-halo rows appended that no entry references."""

    def __init__(self, G, GH, r0, r1, work, extra=0):
        dt = G.dtype
        self.r0, self.r1, self.n_own = r0, r1, r1 - r0
        parts = []
        for mat, halo_is_low in ((G, True), (GH, False)):
            loc = sp.csr_matrix(mat[r0:r1])
            loc.sort_indices()
            cols = loc.indices.astype(np.int64)
            own = (cols >= r0) if halo_is_low else (cols < r1)
            assert np.all((cols < r1) if halo_is_low else (cols >= r0))
            ids = np.unique(cols[~own])
            idx = np.where(own, cols - r0, self.n_own + np.searchsorted(ids, cols)).astype(np.int32)
            parts.append((ids, (loc.indptr.astype(np.int64), idx, np.ascontiguousarray(loc.data, dtype=dt))))
        (self.x_ids, self.g), (self.w_ids, self.gh) = parts
        self.n_xhalo, self.n_whalo = self.x_ids.size + extra, self.w_ids.size
        self.nnz = (self.g[1].size, self.gh[1].size)
        rc, self.plan = shard_create(dt, WORKS[work], self.n_own, self.n_xhalo, self.n_whalo, self.g, self.gh)
        assert rc == 0 and self.plan.value, last_error()
        self.x_idx = dev(self.x_ids)                           # global rows of the x-halo block, on the device

    def destroy(self):
        _L().rlh_fsshard_destroy(self.plan)


class Shards:
    def __init__(self, G, cuts, work, extra=0):
        G = sp.csr_matrix(G)
        G.sort_indices()
        GH = sp.csr_matrix(G.conj().T)
        GH.sort_indices()
        self.dt, self.work, self.cuts = G.dtype, work, list(cuts)
        self.wrb = w_row_bytes(G.dtype, work)
        self.parts = [Shard(G, GH, cuts[s], cuts[s + 1], work, extra) for s in range(len(cuts) - 1)]
        for s in self.parts:
            assert shard_info(s.plan)['w_row_bytes'] == self.wrb and shard_info(s.plan)['work'] == WORKS[work]
        # the sends of W: for shard s and each owner q of its halo rows, (q, device list of q's own rows, first, count)
        self.w_moves = []
        for s in self.parts:
            owner = np.searchsorted(self.cuts, s.w_ids, side='right') - 1
            moves = []
            for q in np.unique(owner):
                at = np.flatnonzero(owner == q)
                moves.append((int(q), dev(s.w_ids[at] - self.cuts[q]), int(at[0]), int(at.size)))
            self.w_moves.append(moves)

    def owners(self):
        """Per shard (owners of its x-halo rows, owners of its W-halo rows)."""
        return [(set(np.searchsorted(self.cuts, s.x_ids, side='right') - 1), set(np.searchsorted(self.cuts, s.w_ids, side='right') - 1))
                for s in self.parts]

    def run(self, m, X, ldx, Y, ldy):
        """The whole application on column-major device blocks of the GLOBAL dimension (pointers); returns 0 or the
        first non-zero code."""
        L, es, code = _L(), self.dt.itemsize, _code(self.dt)
        keep = []
        for s in self.parts:
            ldh = max(s.n_xhalo, 1)
            XH = dev(np.full(ldh * max(m, 1), np.nan, dtype=self.dt))       # (rows past the referenced ones stay NaN)
            keep.append(XH)
            if s.x_ids.size and m:
                _check(L.rlh_gather_rows(code, s.x_ids.size, s.x_idx.ptr, m, X, ldx, XH.ptr, ldh))
            rc = L.rlh_fsshard_first(s.plan, m, X + s.r0 * es, ldx, XH.ptr if s.n_xhalo else None, ldh)
            if rc:
                return rc
        tiles = -(-m // 8)
        for s, moves in zip(self.parts, self.w_moves):
            for q, idx, first, count in moves:
                out = dev(np.zeros(max(tiles * count * self.wrb, 16), dtype=np.uint8))
                keep.append(out)
                rc = L.rlh_fsshard_pack(self.parts[q].plan, m, count, idx.ptr, out.ptr)
                rc = rc or L.rlh_fsshard_halo(s.plan, m, first, count, out.ptr)
                if rc:
                    return rc
        for s in self.parts:
            rc = L.rlh_fsshard_second(s.plan, m, Y + s.r0 * es, ldy)
            if rc:
                return rc
        _check(L.rlh_sync())
        return 0

    def destroy(self):
        for s in self.parts:
            s.destroy()


def with_shards(G, cuts, work, body, extra=0):
    sh = Shards(G, cuts, work, extra)
    try:
        return body(sh)
    finally:
        sh.destroy()


def level1(A):
    """G of a level-1 build of A."""
    rc, h = create(A, bits=32)
    _check(rc)
    try:
        return get(h, A.dtype.type)
    finally:
        destroy(h)


def checked(apply, ref, n, vectors, seed, alone=()):
    """The checks of _fsai_work_cases.checked_application for apply(m, X, ldx, Y, ldy) on device pointers."""
    dt = ref.dt
    es = dt.itemsize
    ld, ldy = n + 5, n + 8
    rng = np.random.default_rng(seed)
    xs = random_block(rng, max(vectors), n, dt)
    exact = ref.exact(xs)
    worst = 0.0
    for m in vectors:
        x = xs[:m]
        hx, hy = padded(x, ld), np.full((m + GUARD) * ldy, np.nan, dtype=dt)
        X, Y = dev(hx), dev(hy)
        assert apply(m, X.ptr, ld, Y.ptr, ldy) == 0, last_error()
        y = fetch(Y, hy.size, dt).reshape(m + GUARD, ldy)
        assert np.array_equal(bits(fetch(X, hx.size, dt)), bits(hx))                # X is unchanged
        assert np.all(np.isnan(y[:, n:])) and np.all(np.isnan(y[m:, :]))            # guards
        worst = max(worst, ref.check(x, y[:m, :n], exact[:m]))
        Y2 = dev(hy)                                                                # again: equal bits
        assert apply(m, X.ptr, ld, Y2.ptr, ldy) == 0, last_error()
        assert np.array_equal(bits(fetch(Y2, hy.size, dt)), bits(y.reshape(-1)))
        # the same block one element further on (X and Y only element-aligned)
        X1, Y1 = dev(padded(x, ld, lead=1)), dev(np.full(hy.size + 1, np.nan, dtype=dt))
        assert apply(m, X1.ptr + es, ld, Y1.ptr + es, ldy) == 0, last_error()
        y1 = fetch(Y1, hy.size + 1, dt)
        assert np.isnan(y1[0]) and np.array_equal(bits(y1[1:]), bits(y.reshape(-1)))
        if alone and m == alone[0]:
            for j in alone[1]:
                Yj = dev(np.full(ldy + 1, np.nan, dtype=dt))
                assert apply(1, X.ptr + j * ld * es, ld, Yj.ptr, ldy) == 0, last_error()
                yj = fetch(Yj, ldy + 1, dt)
                assert np.array_equal(bits(yj[:n]), bits(y[j, :n])) and np.all(np.isnan(yj[n:])), j
        assert apply(m, X.ptr, ld, X.ptr, ld) == 0, last_error()                    # in place
        z = fetch(X, hx.size, dt).reshape(m + GUARD, ld)
        assert np.array_equal(bits(z[:m, :n]), bits(y[:m, :n]))
        assert np.all(np.isnan(z[:, n:])) and np.all(np.isnan(z[m:, :]))
    print('largest error / bound: %.3g (a = %d, b = %d, coefficient %.3g)' % (worst, ref.a, ref.b, ref.coef))


# ---------------------------------------------------------------- 1: one shard is the existing plan
def one_shard(code, work):
    A = matrix(code)
    dt = np.dtype(TYPES[code])
    ld = N + 3

    def body(h, p, G):
        def inner(sh):
            assert sh.parts[0].n_xhalo == 0 and sh.parts[0].n_whalo == 0
            xs = random_block(np.random.default_rng(51), 17, N, dt)
            for m in (1, 8, 17):
                hx, hy = padded(xs[:m], ld), np.full((m + GUARD) * ld, np.nan, dtype=dt)
                X, Y, Y2 = dev(hx), dev(hy), dev(hy)
                assert run(p, m, X.ptr, ld, Y.ptr, ld) == 0, last_error()
                assert sh.run(m, X.ptr, ld, Y2.ptr, ld) == 0, last_error()
                assert np.array_equal(bits(fetch(Y2, hy.size, dt)), bits(fetch(Y, hy.size, dt)))
        with_shards(G, (0, N), work, inner)
    with_plan(A, work, body)


# ---------------------------------------------------------------- 2: three shards
def three_shards(code, work):
    G = level1(matrix(code))
    cuts = (0, 211, 590, N)
    assert all(c % 8 for c in cuts[1:])

    def body(sh):
        for s in sh.parts[1:]:
            assert s.x_ids.size >= 100
        for s in sh.parts[:-1]:
            assert s.w_ids.size >= 100
        checked(sh.run, Reference(G, TYPES[code], work), N, VECTORS, 52, alone=(33, (0, 7, 8, 32)))
    with_shards(G, cuts, work, body)


# ---------------------------------------------------------------- 3: halo rows from two owners
def two_owners(work):
    G = level1(matrix('d'))
    cuts = (0, 155, 310, 465, 620, N)

    def body(sh):
        own = sh.owners()
        assert any(len(x) == 2 for x, _ in own) and any(len(w) == 2 for _, w in own), own
        checked(sh.run, Reference(G, np.float64, work), N, (1, 17), 53, alone=(17, (0, 16)))
    with_shards(G, cuts, work, body)


# ---------------------------------------------------------------- 4: unreferenced halo rows are never read
def unreferenced_rows(work):
    G = level1(matrix('d'))
    cuts = (0, 211, 590, N)
    m, ld = 9, N + 5
    x = random_block(np.random.default_rng(54), m, N, np.float64)
    out = []
    for extra in (0, 2):                                     # two more x-halo rows, NaN, that no entry references
        def body(sh):
            assert all(s.n_xhalo == s.x_ids.size + extra for s in sh.parts)
            X, Y = dev(padded(x, ld)), dev(np.full((m + GUARD) * ld, np.nan))
            assert sh.run(m, X.ptr, ld, Y.ptr, ld) == 0, last_error()
            return fetch(Y, (m + GUARD) * ld, np.float64).reshape(m + GUARD, ld)[:m, :N]
        out.append(with_shards(G, cuts, work, body, extra=extra))
    assert np.all(np.isfinite(out[0])) and np.array_equal(bits(out[0]), bits(out[1]))


# ---------------------------------------------------------------- 5: long rows through the tail, with halo columns
def long_rows(work):
    A = arrowhead()
    n = A.shape[0]
    G = level1(A)
    assert n == 2049

    def body(sh):
        assert sh.parts[0].w_ids.size == n - 1000 and sh.parts[0].gh[0][1] == n       # row 0 of G^H: 1049 halo columns
        for s in sh.parts:
            f = shard_info(s.plan)                           # (before the first product: W is not there yet)
            sv = np.dtype(stored_type(np.float64, work)).itemsize
            assert f['bytes'] <= 2 * sum(s.nnz) * (4 + sv) + 64 * s.n_own + 4096
        assert shard_info(sh.parts[0].plan)['tail'] > 0
        ref = Reference(G, np.float64, work)
        assert ref.b == n
        checked(sh.run, ref, n, (1, 17), 55, alone=(17, (0, 16)))
    with_shards(G, (0, 1000, n), work, body)


# ---------------------------------------------------------------- 6: edges
def edges_empty():
    dt = np.float64
    zero = np.zeros(1, dtype=np.int64)
    none = np.zeros(0, dtype=np.int32), np.zeros(0, dtype=dt)
    for work in WORKS.values():
        rc, p = shard_create(dt, work, 0, 0, 0, (zero,) + none, (zero,) + none)      # n_own = 0: a valid empty plan
        assert rc == 0 and p.value, last_error()
        f = shard_info(p)
        assert f['slots'] == 0 and f['tail'] == 0 and f['work'] == work and f['bytes'] == 0
        Y = dev(np.full(4, np.nan))
        assert _L().rlh_fsshard_first(p, 3, Y.ptr, 0, None, 0) == 0, last_error()
        assert _L().rlh_fsshard_pack(p, 3, 0, None, None) == 0, last_error()
        assert _L().rlh_fsshard_second(p, 3, Y.ptr, 0) == 0, last_error()
        _check(_L().rlh_sync())
        assert np.all(np.isnan(fetch(Y, 4, dt)))
        _L().rlh_fsshard_destroy(p)
    assert _L().rlh_fsshard_destroy(None) == 0
    # m = 0 on the three shards of the n = 777 matrix: nothing is touched
    G = level1(matrix('d'))

    def body(sh):
        hy = np.full(N + 5, np.nan)
        X, Y = dev(np.ones(N + 5)), dev(hy)
        assert sh.run(0, X.ptr, N + 5, Y.ptr, N + 5) == 0, last_error()
        assert np.all(np.isnan(fetch(Y, hy.size, dt)))
    with_shards(G, (0, 211, 590, N), 'native', body)


def edges_small(n_own, work):
    """A first shard of one row and a second of n_own rows with that row as its halo."""
    n = n_own + 1
    A = _with_profile(n, (1, 2, 9), np.float64, 60 + n)
    G = level1(A)

    def body(sh):
        assert sh.parts[1].n_own == n_own and sh.parts[1].n_xhalo == 1 and sh.parts[0].n_whalo >= 1
        checked(sh.run, Reference(G, np.float64, work), n, (1, 9), 56, alone=(9, (0, 8)))
    with_shards(G, (0, 1, n), work, body)


# ---------------------------------------------------------------- 7: refusals
def _refused(rc, p, text):
    assert rc != 0 and not p.value, text
    assert text in last_error(), (text, last_error())


def refusals(host_indices):
    """host_indices: the stand-in sees the index list of rlh_fsshard_pack and refuses a bad one; the library, whose list
    lies in device memory, does not follow it and delivers the row as zeros (include/rlhip.h)."""
    L = _L()
    dt = np.float64
    G = level1(matrix('d'))
    GH = sp.csr_matrix(G.conj().T)
    GH.sort_indices()
    s = Shard(G, GH, 211, 590, 'native')
    z = Shard(level1(matrix('z')), sp.csr_matrix(level1(matrix('z')).conj().T), 0, N, 'native')
    try:
        g, gh, sizes = s.g, s.gh, (s.n_own, s.n_xhalo, s.n_whalo)
        assert L.rlh_fsshard_create(None, _code(dt), 0, *sizes, *[_ptr(a) for a in g + gh]) != 0
        assert 'rlh_fsshard_create: null plan pointer' in last_error()
        _refused(*shard_create(dt, 0, *sizes, (None,) + g[1:], gh), 'rlh_fsshard_create: null indptr')
        _refused(*shard_create(dt, 0, *sizes, g, (None,) + gh[1:]), 'rlh_fsshard_create: null indptr')
        _refused(*shard_create(dt, 0, *sizes, (g[0], None, g[2]), gh), 'rlh_fsshard_create: null indices or values')
        _refused(*shard_create(dt, 0, *sizes, g, (gh[0], gh[1], None)), 'rlh_fsshard_create: null indices or values')
        _refused(*shard_create(dt, 3, *sizes, g, gh), 'rlh_fsshard_create: work must be 0 (native), 1 (float32) or 2 (bf16), got 3')
        _refused(*shard_create(dt, -1, *sizes, g, gh), 'rlh_fsshard_create: work must be')
        _refused(*shard_create(np.complex128, 2, z.n_own, 0, 0, z.g, z.gh), 'rlh_fsshard_create: bfloat16 work blocks are for real types only')
        _refused(*shard_create(dt, 0, -1, 0, 0, g, gh), 'rlh_fsshard_create: negative size')
        _refused(*shard_create(dt, 0, sizes[0], -1, sizes[2], g, gh), 'rlh_fsshard_create: negative size')
        # a column >= n_own + n_xhalo: one halo row fewer than the last column needs; row: the first that references it
        last = s.n_own + s.n_xhalo - 1
        row = int(np.searchsorted(g[0], np.flatnonzero(g[1] == last)[0], side='right') - 1)
        _refused(*shard_create(dt, 0, s.n_own, s.n_xhalo - 1, s.n_whalo, g, gh),
                 'rlh_fsshard_create: broken layout of G: column index out of range in row %d' % row)
        last = s.n_own + s.n_whalo - 1
        row = int(np.searchsorted(gh[0], np.flatnonzero(gh[1] == last)[0], side='right') - 1)
        _refused(*shard_create(dt, 0, s.n_own, s.n_xhalo, s.n_whalo - 1, g, gh),
                 'rlh_fsshard_create: broken layout of G^H: column index out of range in row %d' % row)
        ip = g[0].copy()
        ip[50] = ip[49] - 1
        _refused(*shard_create(dt, 0, *sizes, (ip,) + g[1:], gh), 'rlh_fsshard_create: indptr of G must start at 0 and not decrease (row 49)')
        ip = gh[0].copy()
        ip[0] = 1
        _refused(*shard_create(dt, 0, *sizes, g, (ip,) + gh[1:]), 'rlh_fsshard_create: indptr of G^H must start at 0 and not decrease (row 0)')
        # the order of an application
        m, ld = 3, N
        X = dev(np.ones(m * ld))
        XH = dev(np.ones(m * s.n_xhalo))
        p = s.plan
        x_own = X.ptr + s.r0 * 8
        for call, text in ((lambda: L.rlh_fsshard_second(p, m, x_own, ld), 'rlh_fsshard_second: no rlh_fsshard_first came before'),
                           (lambda: L.rlh_fsshard_first(None, m, x_own, ld, XH.ptr, s.n_xhalo), 'rlh_fsshard_first: null plan'),
                           (lambda: L.rlh_fsshard_first(p, -1, x_own, ld, XH.ptr, s.n_xhalo), 'rlh_fsshard_first: negative number of vectors'),
                           (lambda: L.rlh_fsshard_first(p, m, None, ld, XH.ptr, s.n_xhalo), 'rlh_fsshard_first: null pointer'),
                           (lambda: L.rlh_fsshard_first(p, m, x_own, ld, None, s.n_xhalo),
                            'rlh_fsshard_first: null halo block with %d halo rows' % s.n_xhalo),
                           (lambda: L.rlh_fsshard_first(p, m, x_own, s.n_own - 1, XH.ptr, s.n_xhalo),
                            'rlh_fsshard_first: Matrix and vectors dimensions incompatible'),
                           (lambda: L.rlh_fsshard_first(p, m, x_own, ld, XH.ptr, s.n_xhalo - 1),
                            'rlh_fsshard_first: Matrix and vectors dimensions incompatible')):
            assert call() != 0 and text in last_error(), (text, last_error())
        assert L.rlh_fsshard_first(p, m, x_own, ld, XH.ptr, s.n_xhalo) == 0, last_error()
        tiles, wrb = 1, 64
        idx = dev(np.arange(4, dtype=np.int64))
        out = dev(np.zeros(tiles * max(s.n_whalo, 4) * wrb, dtype=np.uint8))
        for call, text in ((lambda: L.rlh_fsshard_second(p, m + 1, x_own, ld), 'rlh_fsshard_second: the last rlh_fsshard_first had 3 vectors, not 4'),
                           (lambda: L.rlh_fsshard_second(p, m, x_own, ld), 'rlh_fsshard_second: halo rows missing (0 of %d placed)' % s.n_whalo),
                           (lambda: L.rlh_fsshard_pack(p, m + 1, 4, idx.ptr, out.ptr), 'rlh_fsshard_pack: no rlh_fsshard_first with 4 vectors came before'),
                           (lambda: L.rlh_fsshard_pack(p, m, 4, None, out.ptr), 'rlh_fsshard_pack: null pointer'),
                           (lambda: L.rlh_fsshard_pack(p, m, s.n_own + 1, idx.ptr, out.ptr),
                            'rlh_fsshard_pack: %d rows asked of %d own rows' % (s.n_own + 1, s.n_own)),
                           (lambda: L.rlh_fsshard_pack(None, m, 4, idx.ptr, out.ptr), 'rlh_fsshard_pack: null plan'),
                           (lambda: L.rlh_fsshard_halo(p, m, s.n_whalo - 1, 2, out.ptr),
                            'rlh_fsshard_halo: rows %d .. %d of %d halo rows' % (s.n_whalo - 1, s.n_whalo + 1, s.n_whalo)),
                           (lambda: L.rlh_fsshard_halo(p, m, 0, 2, None), 'rlh_fsshard_halo: null pointer'),
                           (lambda: L.rlh_fsshard_halo(p, m + 1, 0, 2, out.ptr), 'rlh_fsshard_halo: no rlh_fsshard_first with 4 vectors came before'),
                           (lambda: L.rlh_fsshard_halo(p, m, -1, 2, out.ptr), 'rlh_fsshard_halo: negative size')):
            assert call() != 0 and text in last_error(), (text, last_error())
        # a part of the halo rows is still "missing"; all of them are not
        assert L.rlh_fsshard_halo(p, m, 0, s.n_whalo - 1, out.ptr) == 0, last_error()
        assert L.rlh_fsshard_second(p, m, x_own, ld) != 0
        assert 'rlh_fsshard_second: halo rows missing (%d of %d placed)' % (s.n_whalo - 1, s.n_whalo) in last_error()
        assert L.rlh_fsshard_halo(p, m, s.n_whalo - 1, 1, out.ptr) == 0, last_error()
        Y = dev(np.full(m * ld, np.nan))
        for call, text in ((lambda: L.rlh_fsshard_second(p, m, None, ld), 'rlh_fsshard_second: null pointer'),
                           (lambda: L.rlh_fsshard_second(p, m, Y.ptr, s.n_own - 1), 'rlh_fsshard_second: Matrix and vectors dimensions incompatible'),
                           (lambda: L.rlh_fsshard_second(None, m, Y.ptr, ld), 'rlh_fsshard_second: null plan')):
            assert call() != 0 and text in last_error(), (text, last_error())
        assert L.rlh_fsshard_second(p, m, Y.ptr, ld) == 0, last_error()
        _check(L.rlh_sync())
        y = fetch(Y, m * ld, dt).reshape(m, ld)
        assert np.all(np.isfinite(y[:, :s.n_own])) and np.all(np.isnan(y[:, s.n_own:]))
        assert np.array_equal(fetch(X, m * ld, dt), np.ones(m * ld))
        # a new rlh_fsshard_first forgets the rows placed
        assert L.rlh_fsshard_first(p, m, x_own, ld, XH.ptr, s.n_xhalo) == 0, last_error()
        assert L.rlh_fsshard_second(p, m, Y.ptr, ld) != 0 and 'halo rows missing (0 of' in last_error()
        # an index of rlh_fsshard_pack outside the own rows
        bad = dev(np.array([0, s.n_own, 5, -1], dtype=np.int64))
        good = dev(np.array([0, 1, 5, 2], dtype=np.int64))
        o1, o2 = dev(np.full(4 * wrb, 255, dtype=np.uint8)), dev(np.full(4 * wrb, 255, dtype=np.uint8))
        assert L.rlh_fsshard_pack(p, m, 4, good.ptr, o2.ptr) == 0, last_error()
        rc = L.rlh_fsshard_pack(p, m, 4, bad.ptr, o1.ptr)
        if host_indices:
            assert rc != 0 and 'rlh_fsshard_pack: row index out of range' in last_error()
        else:
            assert rc == 0, last_error()
            _check(L.rlh_sync())
            a, b = fetch(o1, 4 * wrb, np.uint8).reshape(4, wrb), fetch(o2, 4 * wrb, np.uint8).reshape(4, wrb)
            assert np.array_equal(a[[0, 2]], b[[0, 2]]) and not np.any(a[[1, 3]])
        assert L.rlh_fsshard_info(None, None, None, None, None, None) != 0 and 'rlh_fsshard_info: null plan' in last_error()
    finally:
        s.destroy()
        z.destroy()


# ---------------------------------------------------------------- 8: device memory (GPU tier)
def device_memory():
    def live():
        nbytes, nblocks = ctypes.c_int64(-1), ctypes.c_int64(-1)
        _check(_L().rlh_device_live(ctypes.byref(nbytes), ctypes.byref(nblocks)))
        return nbytes.value, nblocks.value
    G = level1(matrix('d'))
    GH = sp.csr_matrix(G.conj().T)
    GH.sort_indices()
    first = live()
    s = Shard(G, GH, 211, 590, 'bf16')
    held = live()
    f = shard_info(s.plan)
    assert held[0] - first[0] == f['bytes'] > 0             # (the upload of the host arrays is gone; the test's own buffers do not count)
    assert f['bytes'] <= 2 * sum(s.nnz) * (4 + 4) + 64 * s.n_own + 4096
    X = dev(np.ones(33 * N))
    XH = dev(np.ones(33 * s.n_xhalo))
    for m in (8, 33):                                       # W (own and halo rows) grows once
        assert _L().rlh_fsshard_first(s.plan, m, X.ptr, N, XH.ptr, s.n_xhalo) == 0, last_error()
        assert shard_info(s.plan)['bytes'] == f['bytes'] + ((m + 7) // 8) * (s.n_own + s.n_whalo) * 16
    del X, XH
    s.destroy()
    del s
    assert live() == first


# ---------------------------------------------------------------- the class, on a process group
def global_matrix(dt, n=1000):
    return _with_profile(n, (1, 2, 9, 30), dt, 7)


def both_constructors(A, comm, off, **kw):
    """ShardedApproximateInverse of the global matrix and of this rank's rows of it."""
    from raleigh_amd.algebra.hip.dist import ShardedApproximateInverse
    from raleigh_amd.algebra.hip.sparse import full_from_upper
    r0, r1 = int(off[comm.rank]), int(off[comm.rank + 1])
    yield ShardedApproximateInverse(A, comm, offsets=off, **kw)
    rows = sp.csr_matrix(full_from_upper(A)[r0:r1, :])
    yield ShardedApproximateInverse.from_local_rows(rows, r0, A.shape[0], comm, off, **kw)


def class_level1(A, comm, off, single_work=None):
    """(a): at level 1 the own rows are those of the single-process build, bit for bit, with and without drop."""
    from raleigh_amd.algebra.hip.precond import ApproximateInverse
    r0, r1 = int(off[comm.rank]), int(off[comm.rank + 1])
    for drop in (0.0, 0.02):
        whole = ApproximateInverse(A, drop=drop, work=single_work)
        G = whole.csr()
        want = sp.csr_matrix(G[r0:r1, :])
        removed = None
        if drop:
            removed = int(ApproximateInverse(A, work=single_work).csr()[r0:r1, :].nnz - want.nnz)
            assert whole.dropped_entries > 0
        for T in both_constructors(A, comm, off, drop=drop):
            got = T.csr()
            assert got.shape == (r1 - r0, A.shape[0]) and got.dtype == A.dtype
            assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
            assert np.array_equal(bits(got.data), bits(want.data))
            assert T.nnz == whole.nnz and T.longest_row == whole.longest_row and abs(T.fill - whole.fill) < 1e-15
            assert T.size() == A.shape[0] and T.data_type() == A.dtype and T.setup_seconds >= 0
            if drop:
                assert T.dropped_entries == removed
            else:
                assert T.dropped_entries == 0


def class_rows_defined(A, comm, off, **kw):
    """(b): every own row is the minimiser on its own pattern (_fsai_cases.check_row), lower triangular, diagonal last."""
    from _fsai_cases import check_row, hermitian_from_upper
    F = hermitian_from_upper(A).tocsr()
    wide = np.clongdouble if A.dtype.kind == 'c' else np.longdouble
    r0 = int(off[comm.rank])
    for T in both_constructors(A, comm, off, **kw):
        G = T.csr()
        for i in range(G.shape[0]):
            p = G.indices[G.indptr[i]:G.indptr[i + 1]]
            assert p.size and p[-1] == r0 + i and np.all(np.diff(p) > 0)
            check_row(G, i, p, F[p][:, p].toarray().astype(wide), A.dtype)


def gathered_csr(T, comm):
    parts = [None] * comm.size
    comm.dist.all_gather_object(parts, T.csr(), group=comm.group)
    return sp.csr_matrix(sp.vstack(parts, format='csr'))


def class_application(A, comm, off, works, m=11):
    """(c) and (d): apply on ShardedVectors within the bound for the G assembled from all ranks; the halo counts."""
    from raleigh_amd.algebra.hip.dist import ShardedVectors
    n = A.shape[0]
    x = random_block(np.random.default_rng(57), m, n, A.dtype)
    forced = comm.size == 1 and comm.force
    for work in works:
        for T in both_constructors(A, comm, off, work=work):
            xh, wh = T.halo_rows()
            assert (xh > 0) == (comm.rank > 0 or forced) and (wh > 0) == (comm.rank < comm.size - 1 or forced), (xh, wh)
            ref = Reference(gathered_csr(T, comm), A.dtype, work)
            X = ShardedVectors(x, comm=comm, offsets=off)
            Y = X.new_vectors(m)
            T.apply(X, Y)
            y = Y.data()
            ref.check(x, y)
            assert np.array_equal(bits(X.data()), bits(x))
            T.apply(X, X)                                   # in place
            assert np.array_equal(bits(X.data()), bits(y))
            assert T.device_bytes() > 0 and T.algorithmic_bytes(m) > 0
            with pytest.raises(ValueError, match='vectors differ'):
                T.apply(X, X.new_vectors(m - 1))
            with pytest.raises(ValueError, match='data types differ'):
                T.apply(X, ShardedVectors(n, m, np.complex64, comm=comm, offsets=off))
            with pytest.raises(ValueError, match='dimensions incompatible'):
                T.apply(X, ShardedVectors(n + 64, m, A.dtype.type, comm=comm))
            with pytest.raises(ValueError, match='row-sharded'):
                from raleigh_amd.algebra.hip import Vectors
                T.apply(Vectors(n, m, A.dtype.type), Y)


def class_refusals(A, comm, off):
    from raleigh_amd.algebra.hip.dist import ShardedApproximateInverse
    with pytest.raises(ValueError, match='work must be'):
        ShardedApproximateInverse(A, comm, offsets=off, work=None)
    with pytest.raises(ValueError, match='work must be'):
        ShardedApproximateInverse(A, comm, offsets=off, work='float16')
    with pytest.raises(ValueError, match='real matrices only'):
        ShardedApproximateInverse(A.astype(np.complex128), comm, offsets=off, work='bf16')
    with pytest.raises(ValueError, match='max_row'):
        ShardedApproximateInverse(A, comm, offsets=off, max_row=65)


def class_end_to_end(comm, work='native'):
    """(e): the assertion of test_sharded_driver_with_forced_collectives, with the sharded approximate inverse."""
    from raleigh_amd.interfaces import partial_hevp
    from raleigh_amd.algebra.hip.dist import ShardedApproximateInverse, ShardedSparseMatrix, ShardedVectors
    from oracle.sparse import lap3d, lap3d_eigenvalues
    A = lap3d(12, 12, 12, 1.0, 1.01, 1.02)
    op = ShardedSparseMatrix(A, comm)
    T = ShardedApproximateInverse(A, comm, work=work)
    np.random.seed(1)
    lmd, x, status = partial_hevp(None, T=T, which=4, tol=1e-6, verb=-1, operator=op,
                                  vectors=lambda nn, data_type: ShardedVectors(nn, 0, data_type, comm=comm))
    assert status == 0, status
    assert np.allclose(lmd[:4], lap3d_eigenvalues(12, 12, 12, 1.0, 1.01, 1.02, 4), rtol=1e-10), lmd[:4]
    return partial_hevp.last['iterations']
