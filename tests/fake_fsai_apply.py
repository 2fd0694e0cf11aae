"""What csrc/fsai_apply.hip exports, in NumPy, as a mixin of tests/fake_fsai.py's stand-in library: the approximate
inverse's own application with a float32 or bfloat16 work block (rlh_fsapply_*), the application on a row shard
(rlh_fsshard_*) and the refresh of a plan after new values (rlh_fsvalues_plan), with the checks, their order and the
messages of the real library: TEST INFRASTRUCTURE ONLY.  "Device" pointers are host addresses.

The rounding model: G~ = G rounded once to V; W = G~ X formed in float64 / complex128 and rounded once to Wt (bfloat16:
round to nearest even on the float32 bits); Y = G~^H W formed in float64 / complex128 and rounded to T.  The numbers
rlh_fsapply_info reports are those of the library's layout rule (slices of 64 rows; a slice's width is the largest w
with rows * w <= 2 * sum min(len, w); the rest of a row is tail), priced at 4 + sizeof V per slot or tail entry plus the
per-row and per-slice arrays.

A shard keeps W as the library keeps it, [tile][n_own + n_whalo][8] of Wt (bfloat16 as its 16 bits), so that what
rlh_fsshard_pack writes and rlh_fsshard_halo reads are the bytes that travel; the halo rows start as NaN (bfloat16:
0x7fc0) at every rlh_fsshard_first.  rlh_fsshard_pack checks its indices, which here lie in host memory."""

import ctypes

import numpy as np
import scipy.sparse as sp

from fake_lib import _DT, _addr, _block, _flat


def bf16_round(a):
    """float64 / float32 values rounded to float32, then to bfloat16 (nearest even), as float32."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return u.view(np.float32)


def stored_type(dt, work):
    """V: the type of the stored values of G."""
    dt = np.dtype(dt)
    if work == 0:
        return dt.type
    return np.complex64 if dt.kind == 'c' else np.float32


def layout_counts(lens):
    """(slots, tail entries) of the library's layout for rows of these lengths."""
    lens = np.asarray(lens, dtype=np.int64)
    slots = tail = 0
    for s in range(0, lens.size, 64):
        part = lens[s:s + 64]
        w = 0
        for cand in range(1, int(part.max()) + 1 if part.size else 1):
            if part.size * cand <= 2 * int(np.minimum(part, cand).sum()):
                w = cand
            else:
                break                    # (2 sum min(len, w) - rows w is concave in w: the good widths are an interval)
        slots += part.size * w
        tail += int(np.maximum(part - w, 0).sum())
    return slots, tail


def wide_type(dt):
    """The type sums are formed in: float64 / complex128."""
    return np.complex128 if np.dtype(dt).kind == 'c' else np.float64


def put(ptr, ctype, value):
    """*ptr = value where the caller passed an output pointer."""
    if ptr is not None:
        ctypes.cast(ptr, ctypes.POINTER(ctype))[0] = value


def _both_layouts(g, gh):
    """(slots, tail entries) of G and G^H together."""
    a, b = layout_counts(np.diff(g.indptr)), layout_counts(np.diff(gh.indptr))
    return a[0] + b[0], a[1] + b[1]


def _layout_bytes(slots, tail, v, n):
    return (slots + tail) * (4 + v.itemsize) + 2 * (12 * n + 8 + 12 * (-(-n // 64) + 1))


def _work_message(name, work, dt):
    """What is wrong with the `work` of a plan for type dt, or None."""
    if work not in (0, 1, 2):
        return name + ': work must be 0 (native), 1 (float32) or 2 (bf16), got %d' % work
    if work == 2 and np.dtype(dt).kind == 'c':
        return name + ': bfloat16 work blocks are for real types only'
    return None


class _Plan:
    def __init__(self, f, work):
        self.code, self.work, self.n = f.code, work, f.g.shape[0]
        self.v = np.dtype(stored_type(_DT[f.code], work))
        self.take_values(f)
        self.slots, self.tail = _both_layouts(self.g, self.gh)
        self.w_bytes = 0

    def take_values(self, f):
        """The plan's rounded copies of the handle's G and G^H."""
        self.g = sp.csr_matrix(f.g.astype(self.v).astype(wide_type(_DT[f.code])))
        self.gh = sp.csr_matrix(self.g.conj().T)

    def round_w(self, w):
        if self.work == 0:
            return w.astype(_DT[self.code])
        if self.work == 1:
            return w.astype(self.v)
        return bf16_round(w)

    def w_itemsize(self):
        return 2 if self.work == 2 else (np.dtype(_DT[self.code]).itemsize if self.work == 0 else self.v.itemsize)


class _Shard:
    def __init__(self, code, work, n_own, n_xhalo, n_whalo, g, gh):
        self.code, self.work, self.n_own, self.n_xhalo, self.n_whalo = code, work, n_own, n_xhalo, n_whalo
        dt = np.dtype(_DT[code])
        self.v = np.dtype(stored_type(dt, work))
        self.g, self.gh = g, gh                            # V values held in float64 / complex128
        self.wt = np.dtype(np.uint16) if work == 2 else (dt if work == 0 else self.v)
        self.slots, self.tail = _both_layouts(g, gh) if n_own else (0, 0)
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


class FakeFsaiApplyMixin:
    """Needs the host class's `_fsai` (the handles of fake_fsai.py), `_fail`, `_count` and `_next_handle`."""

    def __init__(self):
        super().__init__()
        self._plans = {}
        self._shards = {}

    def _new_handle(self, table, obj, out):
        h = self._next_handle
        self._next_handle += 1
        table[h] = obj
        out._obj.value = h
        return 0

    # ---------------------------------------------------------------- rlh_fsapply_*
    def rlh_fsapply_create(self, pp, h, work):
        self._count('fsapply_create')
        if pp is None:
            return self._fail('rlh_fsapply_create: null plan pointer')
        pp._obj.value = None
        if not _addr(h):
            return self._fail('rlh_fsapply_create: null handle')
        f = self._fsai[_addr(h)]
        if msg := _work_message('rlh_fsapply_create', work, _DT[f.code]):
            return self._fail(msg)
        return self._new_handle(self._plans, _Plan(f, work), pp)

    def rlh_fsapply_run(self, p, m, X, ldx, Y, ldy):
        self._count('fsapply_run')
        if not _addr(p):
            return self._fail('rlh_fsapply_run: null plan')
        plan = self._plans[_addr(p)]
        n = plan.n
        if m < 0:
            return self._fail('rlh_fsapply_run: negative number of vectors')
        if m == 0 or n == 0:
            return 0
        if not _addr(X) or not _addr(Y):
            return self._fail('rlh_fsapply_run: null pointer')
        if ldx < n or ldy < n:
            return self._fail('rlh_fsapply_run: Matrix and vectors dimensions incompatible')
        x = _block(X, plan.code, n, m, ldx)
        wide = plan.g.dtype
        with np.errstate(invalid='ignore', over='ignore'):
            w = plan.round_w(np.asarray(plan.g @ x.T.astype(wide))).astype(wide)
            _block(Y, plan.code, n, m, ldy)[:, :] = np.asarray(plan.gh @ w).T.astype(_DT[plan.code])
        plan.w_bytes = max(plan.w_bytes, -(-m // 8) * 8 * n * plan.w_itemsize())
        return 0

    def rlh_fsapply_info(self, p, work, slots, tail, nbytes):
        if not _addr(p):
            return self._fail('rlh_fsapply_info: null plan')
        plan = self._plans[_addr(p)]
        put(work, ctypes.c_int, plan.work)
        for ptr, v in ((slots, plan.slots), (tail, plan.tail),
                       (nbytes, _layout_bytes(plan.slots, plan.tail, plan.v, plan.n) + plan.w_bytes)):
            put(ptr, ctypes.c_int64, v)
        return 0

    def rlh_fsapply_destroy(self, p):
        self._plans.pop(_addr(p), None)
        return 0

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
        plan.take_values(f)
        return 0

    # ---------------------------------------------------------------- rlh_fsshard_*
    def rlh_fsshard_create(self, pp, code, work, n_own, n_xhalo, n_whalo, g_indptr, g_indices, g_values, gh_indptr, gh_indices,
                           gh_values):
        self._count('fsshard_create')
        name = 'rlh_fsshard_create'
        if pp is None:
            return self._fail(name + ': null plan pointer')
        pp._obj.value = None
        if code not in _DT:
            return self._fail(name + ': unknown dtype %d' % code)
        dt = np.dtype(_DT[code])
        if msg := _work_message(name, work, dt):
            return self._fail(msg)
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
        v = np.dtype(stored_type(dt, work))
        mats = []
        for which, ip, indices, values, halo in (('G', ptrs[0], g_indices, g_values, n_xhalo), ('G^H', ptrs[1], gh_indices, gh_values, n_whalo)):
            nnz = int(ip[-1])
            ix = _flat(indices, np.int32, nnz).copy()
            va = _flat(values, dt, nnz).astype(v).astype(wide_type(dt))
            rows = np.repeat(np.arange(n_own), np.diff(ip))
            bad = rows[(ix < 0) | (ix >= n_own + halo)]
            if n_own and bad.size:
                return self._fail(name + ': broken layout of %s: column index out of range in row %d' % (which, bad.min()))
            mats.append(sp.csr_matrix((va, ix, ip), shape=(n_own, n_own + halo)))
        return self._new_handle(self._shards, _Shard(code, work, n_own, n_xhalo, n_whalo, *mats), pp)

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
        held = s.w_bytes + (_layout_bytes(s.slots, s.tail, s.v, s.n_own) if s.n_own else 0)
        put(work, ctypes.c_int, s.work)
        for ptr, v in ((slots, s.slots), (tail, s.tail), (nbytes, held), (w_row_bytes, 8 * s.wt.itemsize)):
            put(ptr, ctypes.c_int64, v)
        return 0

    def rlh_fsshard_destroy(self, p):
        self._shards.pop(_addr(p), None)
        return 0
