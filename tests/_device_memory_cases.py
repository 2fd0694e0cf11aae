"""Device-memory ownership of the handle types (rlh_csr, rlh_spd, rlh_bytes, rlh_sptrsv, rlh_fsai) through the raw C ABI:
how each handle is created, used in the ways that allocate lazily, and destroyed, for tests/test_device_memory_gpu.py.
Run as a program (`python _device_memory_cases.py teardown`) it creates one handle of each type, finalizes the library and
destroys the handles afterwards: the teardown order of an interpreter that drops the context first."""

import ctypes
import functools
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LAYOUT = {0: 'sell', 1: 'well', 2: 'wide'}


def L():
    from raleigh_amd import _lib
    return _lib.lib()


def check(rc):
    from raleigh_amd import _lib
    _lib.check(rc)


def host_ptr(a):
    from raleigh_amd import _lib
    return _lib.host_ptr(a)


def code_of(dt):
    from raleigh_amd import _lib
    return _lib.DTYPE_CODE[np.dtype(dt).type]


def live():
    """(bytes, blocks) the library holds for its handles and builds."""
    nbytes, nblocks = ctypes.c_int64(-1), ctypes.c_int64(-1)
    check(L().rlh_device_live(ctypes.byref(nbytes), ctypes.byref(nblocks)))
    return nbytes.value, nblocks.value


def dev(a):
    """A device copy of a host array in a buffer of Python's own (rlh_malloc: not counted by rlh_device_live)."""
    from raleigh_amd.algebra.hip.memory import DeviceBuffer
    a = np.ascontiguousarray(a)
    buf = DeviceBuffer(max(a.nbytes, 16), zero=False)
    if a.nbytes:
        check(L().rlh_h2d(buf.ptr, host_ptr(a), a.nbytes))
    return buf


def block(rows, ld, dt, seed=3):
    """A device block of `rows` vectors with leading dimension ld (and 64 elements to spare), random."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(rows * ld + 64)
    if np.dtype(dt).kind == 'c':
        a = a + 1j * rng.standard_normal(a.size)
    return dev(a.astype(dt))


class Env:
    """Environment switches of the library for the length of a with block."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.pop(k, None) for k in self.kw}
        os.environ.update({k: v for k, v in self.kw.items() if v is not None})

    def __exit__(self, *a):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


# ---------------------------------------------------------------- matrices
@functools.lru_cache(maxsize=None)
def matrix(name):
    from oracle.sparse import lap3d
    rng = np.random.default_rng(31)
    if name == 'random300':                       # symmetric, no locality: sliced ELL when asked for
        R = sp.random(300, 300, density=0.02, random_state=np.random.RandomState(5), format='csr')
        A = sp.csr_matrix(R + R.T + sp.identity(300))
    elif name == 'stencil':                       # 57 blocks of 1024 rows: stacks when RLH_SPMM_STACK=2 asks for them
        A = lap3d(50, 50, 23, 1.0, 1.01, 1.02)
    elif name == 'stencil_z':
        A = sp.csr_matrix(lap3d(50, 50, 23, 1.0, 1.01, 1.02).astype(np.complex128))
        S = sp.triu(A, k=1)
        A = sp.csr_matrix(A + 0.5j * S - 0.5j * S.T)
    elif name == 'small_stencil':
        A = lap3d(16, 15, 14, 1.0, 1.01, 1.02)
    elif name == 'fsai':
        A = lap3d(12, 12, 12, 1.0, 1.01, 1.02)
    elif name == 'shard':                         # 512 own rows, 1024 columns: block 0 stays below column 512, block 1 reads the halo
        rows = [[i, i + 3, i + 40] if i < 256 else [i - 200, i, 600 + (i * 7) % 400] for i in range(512)]
        ip = np.arange(0, 3 * 512 + 1, 3)
        A = sp.csr_matrix((rng.standard_normal(3 * 512), np.concatenate(rows), ip), shape=(512, 1024))
    elif name == 'data':                          # 500 x 300, 10 entries per row
        ix = np.concatenate([np.sort(rng.choice(300, 10, replace=False)) for _ in range(500)])
        A = sp.csr_matrix((rng.standard_normal(5000), ix, np.arange(0, 5001, 10)), shape=(500, 300))
    else:
        raise KeyError(name)
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A


def arrays(A, index=np.int64, col=np.int32):
    return A.indptr.astype(index), A.indices.astype(col), np.ascontiguousarray(A.data)


def changed(a, pos, val):
    b = a.copy()
    b[pos] = val
    return b


def swapped(a, i, j):
    b = a.copy()
    b[i], b[j] = a[j], a[i]
    return b


def without(A, k):
    """A with its stored entry k removed."""
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    keep = np.arange(A.nnz) != k
    B = sp.csr_matrix((A.data[keep], (rows[keep], A.indices[keep])), shape=A.shape)
    B.sort_indices()
    return B


# ---------------------------------------------------------------- rlh_csr
def csr_create(A, how, mirror=0, indices=None):
    """(rc, handle): how = 'host' (rlh_csr_create), 'upper' (rlh_csr_create_upper on the upper triangle) or 'device'."""
    h = ctypes.c_void_p()
    code = code_of(A.dtype)
    if how == 'device':
        ip, ix, va = arrays(A, np.int64, np.int64)
        bufs = [dev(ip), dev(ix if indices is None else indices), dev(va)]
        rc = L().rlh_csr_create_device(ctypes.byref(h), code, A.shape[0], A.shape[1], 64, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, mirror)
    elif how == 'upper':
        ip, ix, va = arrays(sp.triu(A, format='csr'))
        rc = L().rlh_csr_create_upper(ctypes.byref(h), code, A.shape[0], host_ptr(ip), host_ptr(ix), host_ptr(va))
    else:
        ip, ix, va = arrays(A)
        rc = L().rlh_csr_create(ctypes.byref(h), code, A.shape[0], A.shape[1], host_ptr(ip), host_ptr(ix), host_ptr(va))
    return rc, h


def csr_facts(h):
    """(layout, stacks, device_bytes) of a handle."""
    lay, stored, ratio = ctypes.c_int(), ctypes.c_int64(), ctypes.c_double()
    check(L().rlh_csr_layout(h, ctypes.byref(lay), ctypes.byref(stored), ctypes.byref(ratio)))
    stacks, a, b = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
    check(L().rlh_csr_stacks(h, ctypes.byref(stacks), ctypes.byref(a), ctypes.byref(b)))
    nb = ctypes.c_int64()
    check(L().rlh_csr_info(h, None, None, None, ctypes.byref(nb)))
    return LAYOUT[lay.value], stacks.value, nb.value


def csr_use(h, A, m=4):
    """rlh_spmm, then parts 1 and 2 at two own / halo boundaries (the second rebuilds the part schedules)."""
    n, dt = A.shape[1], A.dtype
    es, ld = dt.itemsize, n + 8
    x, y = block(m, ld, dt), block(m, ld, dt, 4)
    check(L().rlh_spmm(h, m, x.ptr, ld, n, None, 0, y.ptr, ld))
    for n_own in (n // 16 * 8, n // 16 * 8 + 64):
        for part in (1, 2):
            check(L().rlh_spmm_part(h, part, m, x.ptr, ld, n_own, x.ptr + n_own * es, ld, y.ptr, ld))
    check(L().rlh_sync())


def csr_destroy(h):
    check(L().rlh_csr_destroy(h))


# ---------------------------------------------------------------- rlh_spd
def spd_create(A, device, indices=None):
    h = ctypes.c_void_p()
    if device:
        ip, ix, va = arrays(A, np.int64, np.int64)
        bufs = [dev(ip), dev(ix if indices is None else indices), dev(va)]
        rc = L().rlh_spd_create_device(ctypes.byref(h), code_of(A.dtype), A.shape[0], A.shape[1], 64, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr)
    else:
        ip, ix, va = arrays(A)
        rc = L().rlh_spd_create(ctypes.byref(h), code_of(A.dtype), A.shape[0], A.shape[1], host_ptr(ip), host_ptr(ix), host_ptr(va))
    return rc, h


def spd_bytes(h):
    """(device_bytes, workspace_bytes)"""
    nb, ws = ctypes.c_int64(), ctypes.c_int64()
    check(L().rlh_spd_info(h, None, None, None, ctypes.byref(nb)))
    check(L().rlh_spd_stats(h, ctypes.byref(ws), None))
    return nb.value, ws.value


def spd_apply(h, A, m):
    x, y = block(m, A.shape[1], A.dtype), block(m, A.shape[0], A.dtype, 4)
    check(L().rlh_spd_apply(h, 0, m, x.ptr, A.shape[1], y.ptr, A.shape[0], None, None))
    check(L().rlh_sync())


def spd_row_sumsq(h, A):
    out = np.zeros(A.shape[0])
    check(L().rlh_spd_row_sumsq(h, host_ptr(out)))
    return out


def spd_absmax(h):
    v = ctypes.c_double()
    check(L().rlh_spd_absmax(h, ctypes.byref(v)))
    return v.value


def spd_destroy(h):
    check(L().rlh_spd_destroy(h))


# ---------------------------------------------------------------- rlh_bytes
def byte_matrix(rows, cols):
    return np.random.default_rng(rows + cols).integers(0, 256, (rows, cols), dtype=np.uint8)


def bytes_create(D, device):
    """(rc, handle, what keeps a borrowed matrix alive)"""
    h = ctypes.c_void_p()
    if device:
        buf = dev(D)
        return L().rlh_bytes_create_device(ctypes.byref(h), 0, D.shape[0], D.shape[1], buf.ptr, D.shape[1]), h, buf
    return L().rlh_bytes_create(ctypes.byref(h), 0, D.shape[0], D.shape[1], host_ptr(D), D.shape[1]), h, None


def bytes_sizes(h):
    """(device_bytes, workspace_bytes)"""
    nb, ws = ctypes.c_int64(), ctypes.c_int64()
    check(L().rlh_bytes_info(h, None, None, ctypes.byref(nb), ctypes.byref(ws)))
    return nb.value, ws.value


def bytes_apply(h, D, m=4):
    x, y = block(m, D.shape[1], np.float32), block(m, D.shape[0], np.float32, 4)
    check(L().rlh_bytes_apply(h, 0, m, x.ptr, D.shape[1], y.ptr, D.shape[0], None, None))
    check(L().rlh_sync())


def bytes_norms(h, D):
    out, v = np.zeros(D.shape[0]), ctypes.c_double()
    check(L().rlh_bytes_row_sumsq(h, host_ptr(out)))
    check(L().rlh_bytes_absmax(h, ctypes.byref(v)))
    return out, v.value


def bytes_destroy(h):
    check(L().rlh_bytes_destroy(h))


# ---------------------------------------------------------------- rlh_sptrsv
@functools.lru_cache(maxsize=None)
def factor_arrays(n=2000):
    """The storage of the unit lower and the upper factor of the staircase family of tests/_sptrsv_cases.py."""
    import _sptrsv_cases as trsv
    fam = trsv.family('staircase', 'd', n)
    return [(fam[k].storage(), fam[k].lower, fam[k].unit) for k in ('Lu', 'U')]


def trsv_create(which, n=2000):
    (ip, ix, va), lower, unit = factor_arrays(n)[which]
    h = ctypes.c_void_p()
    return L().rlh_sptrsv_create(ctypes.byref(h), code_of(np.float64), n, host_ptr(ip), host_ptr(ix), host_ptr(va),
                                 1 if lower else 0, 1 if unit else 0), h


def trsv_solve(handles, m, n=2000):
    b, x = block(m, n, np.float64), block(m, n, np.float64, 4)
    ops = (ctypes.c_void_p * len(handles))(*[h.value for h in handles])
    check(L().rlh_sptrsv_solve_chain(len(handles), ops, None, None, m, b.ptr, n, x.ptr, n))
    check(L().rlh_sync())


def trsv_destroy(h):
    check(L().rlh_sptrsv_destroy(h))


# ---------------------------------------------------------------- rlh_fsai
FSAI_KINDS = {'plain': ('', {}), 'levels': ('_levels', dict(levels=2)), 'adaptive': ('_adaptive', dict(levels=1, steps=2, step_size=4))}


def fsai_create(A, kind, host, indices=None):
    import _fsai_cases as fsai
    entry, kw = FSAI_KINDS[kind]
    return fsai.create(A, entry, host=host, indices=indices, **kw)


def fsai_apply(h, A, m=4):
    n = A.shape[0]
    x, y = block(m, n, A.dtype), block(m, n, A.dtype, 4)
    check(L().rlh_fsai_apply(h, m, x.ptr, n, y.ptr, n))
    check(L().rlh_sync())


def fsai_destroy(h):
    check(L().rlh_fsai_destroy(h))


# ---------------------------------------------------------------- one small cycle of each type (repeats, teardown)
def small_handles():
    """[(handle, use, destroy)] of one handle of each type."""
    out = []
    A = matrix('random300')
    with Env(RLH_SPMM_FORMAT='sell'):
        rc, h = csr_create(A, 'device')
    check(rc)
    out.append((h, lambda h=h, A=A: csr_use(h, A), csr_destroy))
    D = matrix('data')
    rc, h = spd_create(D, True)
    check(rc)
    out.append((h, lambda h=h, D=D: spd_apply(h, D, 4), spd_destroy))
    B = byte_matrix(100, 70)
    rc, h, _ = bytes_create(B, False)
    check(rc)
    out.append((h, lambda h=h, B=B: bytes_apply(h, B), bytes_destroy))
    rc, h = trsv_create(0)
    check(rc)
    out.append((h, lambda h=h: trsv_solve([h], 16), trsv_destroy))
    F = matrix('fsai')
    rc, h = fsai_create(F, 'plain', False)
    check(rc)
    out.append((h, lambda h=h, F=F: fsai_apply(h, F), fsai_destroy))
    return out


def teardown():
    handles = small_handles()
    for h, use, _ in handles:
        use()
    assert live()[1] > 0
    check(L().rlh_finalize())
    for h, _, destroy in handles:
        destroy(h)
    return 0


if __name__ == '__main__':
    assert sys.argv[1:] == ['teardown']
    sys.exit(teardown())
