"""tests/fake_fsai.py's stand-in library plus the four rlh_fsapply_* entry points (the approximate inverse's own
application with a float32 or bfloat16 work block) in NumPy, with the checks and messages of the real library: TEST
INFRASTRUCTURE ONLY.  "Device" pointers are host addresses.

The rounding model: G~ = G rounded once to V; W = G~ X formed in float64 / complex128 and rounded once to Wt (bfloat16:
round to nearest even on the float32 bits); Y = G~^H W formed in float64 / complex128 and rounded to T.  The numbers
rlh_fsapply_info reports are those of the library's layout rule (slices of 64 rows; a slice's width is the largest w
with rows * w <= 2 * sum min(len, w); the rest of a row is tail), priced at 4 + sizeof V per slot or tail entry plus the
per-row and per-slice arrays."""

import ctypes

import numpy as np
import scipy.sparse as sp

from fake_lib import _DT, _addr, _block
import fake_fsai
from fake_fsai import as_device  # noqa: F401


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


class _Plan:
    def __init__(self, f, work):
        self.code, self.work, self.n = f.code, work, f.g.shape[0]
        dt = np.dtype(_DT[f.code])
        wide = np.complex128 if dt.kind == 'c' else np.float64
        self.v = np.dtype(stored_type(dt, work))
        self.g = sp.csr_matrix(f.g.astype(self.v).astype(wide))
        self.gh = sp.csr_matrix(self.g.conj().T)
        self.slots, self.tail = 0, 0
        for mat in (self.g, self.gh):
            a, b = layout_counts(np.diff(mat.indptr))
            self.slots, self.tail = self.slots + a, self.tail + b
        self.w_bytes = 0

    def round_w(self, w):
        if self.work == 0:
            return w.astype(_DT[self.code])
        if self.work == 1:
            return w.astype(self.v)
        return bf16_round(w)

    def w_itemsize(self):
        return 2 if self.work == 2 else (np.dtype(_DT[self.code]).itemsize if self.work == 0 else self.v.itemsize)


class FakeFsaiWorkLib(fake_fsai.FakeFsaiLib):

    def __init__(self):
        super().__init__()
        self._plans = {}

    def rlh_fsapply_create(self, pp, h, work):
        self._count('fsapply_create')
        if pp is None:
            return self._fail('rlh_fsapply_create: null plan pointer')
        pp._obj.value = None
        if not _addr(h):
            return self._fail('rlh_fsapply_create: null handle')
        if work not in (0, 1, 2):
            return self._fail('rlh_fsapply_create: work must be 0 (native), 1 (float32) or 2 (bf16), got %d' % work)
        f = self._fsai[_addr(h)]
        if work == 2 and np.dtype(_DT[f.code]).kind == 'c':
            return self._fail('rlh_fsapply_create: bfloat16 work blocks are for real types only')
        p = self._next_handle
        self._next_handle += 1
        self._plans[p] = _Plan(f, work)
        pp._obj.value = p
        return 0

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
        n = plan.n
        held = (plan.slots + plan.tail) * (4 + plan.v.itemsize) + 2 * (12 * n + 8 + 12 * (-(-n // 64) + 1)) + plan.w_bytes
        if work is not None:
            ctypes.cast(work, ctypes.POINTER(ctypes.c_int))[0] = plan.work
        for ptr, v in ((slots, plan.slots), (tail, plan.tail), (nbytes, held)):
            if ptr is not None:
                ctypes.cast(ptr, ctypes.POINTER(ctypes.c_int64))[0] = v
        return 0

    def rlh_fsapply_destroy(self, p):
        self._plans.pop(_addr(p), None)
        return 0


def install():
    from raleigh_amd import _lib
    fake = FakeFsaiWorkLib()
    _lib.set_library(fake)
    return fake
