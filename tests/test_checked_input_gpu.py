"""GPU tier: the checked input that every builder from CSR arrays in device memory goes through (csrc/device_build.h:
the checks of indptr and of the columns, one status record, the messages) -- rlh_csr_create_device with mirror_upper
0 and 1, rlh_spd_create_device, rlh_fsai_create_device and rlh_fsvalues_update_device, at both index widths, through
the raw C ABI.  Every refusal is compared with its whole text."""

import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

N = 300              # past the first workgroup of the indptr check (256 rows) and of the columns check (4 rows)
LONG = 100           # the row with more than 64 stored entries: the 64-lane loop over a row takes a second trip
TARGETS = ['csr', 'csr_mirror', 'spd', 'fsai', 'update']
NAMES = {'csr': 'rlh_csr_create_device', 'csr_mirror': 'rlh_csr_create_device', 'spd': 'rlh_spd_create_device',
         'fsai': 'rlh_fsai_create_device', 'update': 'rlh_fsvalues_update_device'}


def _L():
    from raleigh_amd import _lib
    return _lib.lib()


def _check(rc):
    from raleigh_amd import _lib
    _lib.check(rc)


def _dev(a):
    """A device copy of a host array (kept alive by the returned buffer)."""
    from raleigh_amd.algebra.hip.memory import DeviceBuffer
    from raleigh_amd import _lib
    a = np.ascontiguousarray(a)
    buf = DeviceBuffer(max(a.nbytes, 16), zero=False)
    if a.nbytes:
        _check(_L().rlh_h2d(buf.ptr, _lib.host_ptr(a), a.nbytes))
    return buf


def _matrix():
    """Symmetric, strictly diagonally dominant with a positive diagonal (so positive definite): five diagonals and row
    / column LONG joined to 80 further columns, 85 stored entries in that row."""
    rng = np.random.default_rng(22)
    i = np.arange(N)
    pairs = [(i[:-1], i[1:]), (i[:-2], i[2:]), (np.full(80, LONG), LONG + 10 + 2 * np.arange(80))]
    r, c = np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])
    U = sp.csr_matrix((-rng.uniform(0.5, 1.0, r.size), (r, c)), shape=(N, N))
    A = sp.csr_matrix(U + U.T)
    A = sp.csr_matrix(A + sp.diags(np.asarray(abs(A).sum(axis=1)).ravel() + 1.0))
    A.sort_indices()
    assert A.indptr[LONG + 1] - A.indptr[LONG] == 85
    return A


A = _matrix()
IP, IX = A.indptr.astype(np.int64), A.indices.astype(np.int64)


@pytest.fixture(scope='module')
def inverse():
    """The approximate inverse whose values the 'update' target renews."""
    rc, h = _create('fsai', 64, IP, IX)
    _check(rc)
    yield h
    _L().rlh_fsai_destroy(h)


def _create(target, bits, ip, ix, n=N, n_cols=None, inverse=None, values=None):
    """(rc, handle) of the target's entry point on device copies of the arrays; 'update': (rc, None)."""
    from raleigh_amd import _lib
    it = np.int32 if bits == 32 else np.int64
    bufs = [_dev(ip.astype(it)), _dev(ix.astype(it)), _dev(A.data if values is None else values)]
    ptrs = [b.ptr for b in bufs]
    n_cols = n if n_cols is None else n_cols
    h = ctypes.c_void_p(12345)
    D = _lib.DTYPE_CODE[np.float64]
    if target in ('csr', 'csr_mirror'):
        return _L().rlh_csr_create_device(ctypes.byref(h), D, n, n_cols, bits, *ptrs, int(target == 'csr_mirror')), h
    if target == 'spd':
        return _L().rlh_spd_create_device(ctypes.byref(h), D, n, n_cols, bits, *ptrs), h
    if target == 'fsai':
        return _L().rlh_fsai_create_device(ctypes.byref(h), D, n, bits, *ptrs, 8), h
    return _L().rlh_fsvalues_update_device(inverse, bits, *ptrs), None


def _refused(target, bits, ix, text, inverse, ip=IP):
    rc, h = _create(target, bits, ip, ix, inverse=inverse)
    assert rc != 0 and (h is None or not h.value), (target, bits, text)
    assert _L().rlh_last_error().decode() == NAMES[target] + ': ' + text, (target, bits)


def _valid(target, bits, inverse):
    """(f) A valid build of the target's kind; the number of stored entries (of G for the approximate inverse: rows of
    at most 8 entries, all of them kept) and, for an update, the count of updates say that it took place."""
    L = _L()
    count = ctypes.c_int64(-1)
    if target == 'update':
        before = ctypes.c_int64(-1)
        _check(L.rlh_fsvalues_info(inverse, ctypes.byref(before), None))
    rc, h = _create(target, bits, IP, IX, inverse=inverse)
    _check(rc)
    if target == 'update':
        _check(L.rlh_fsvalues_info(inverse, ctypes.byref(count), None))
        assert count.value == before.value + 1
        return
    assert h.value
    if target in ('csr', 'csr_mirror'):
        _check(L.rlh_csr_info(h, None, None, ctypes.byref(count), None))
        L.rlh_csr_destroy(h)
    elif target == 'spd':
        _check(L.rlh_spd_info(h, None, None, ctypes.byref(count), None))
        L.rlh_spd_destroy(h)
    else:
        _check(L.rlh_fsai_info(h, None, ctypes.byref(count), None, None, None, None))
        L.rlh_fsai_destroy(h)
        rows = np.repeat(np.arange(N), np.diff(IP))
        per_row = np.bincount(rows[IX <= rows], minlength=N)
        assert count.value == int(np.minimum(per_row, 8).sum())
        return
    assert count.value == A.nnz


def _broken(*violations):
    """IX with violations (kind, row, offset) at entry IP[row] + offset: 'range' puts the column N there, 'negative' the
    column -1, 'order' the column of the entry before.  Returns the columns and the entries touched."""
    ix, at = IX.copy(), []
    for kind, row, offset in violations:
        k = int(IP[row]) + offset
        assert 0 < offset < IP[row + 1] - IP[row]
        ix[k] = {'range': N, 'negative': -1, 'order': IX[k - 1]}[kind]
        at.append(k)
    return ix, at


def _text(kind, target, row, k):
    """The message of a violation found in `row` at entry k: rlh_spd_create_device names the entry, the others the row."""
    if kind == 'order':
        return ('the columns of a row must ascend strictly (no duplicates): entry %d' % k if target == 'spd'
                else 'the columns of row %d must ascend strictly (no duplicates)' % row)
    return 'column index out of range at entry %d' % k if target == 'spd' else 'column index out of range in row %d' % row


# (a) past the 64th entry of the long row; (b) in row 0 and in the last row
SINGLE = [(kind, row, offset) for row, offset in ((LONG, 70), (0, 1), (N - 1, 2)) for kind in ('range', 'order')]
SINGLE.append(('negative', LONG, 64))


@pytest.mark.parametrize('bits', [32, 64])
@pytest.mark.parametrize('target', TARGETS)
def test_one_violation(target, bits, inverse):
    for kind, row, offset in SINGLE:
        ix, (k,) = _broken((kind, row, offset))
        _refused(target, bits, ix, _text(kind, target, row, k), inverse)
        _valid(target, bits, inverse)


@pytest.mark.parametrize('bits', [32, 64])
@pytest.mark.parametrize('target', TARGETS)
def test_two_violations(target, bits, inverse):
    """(c) Two codes at once: the smaller code (out of range) is reported although its row comes later.  (d) One code
    twice: the smaller position is reported.  Both are deterministic whatever the order in which the waves run: every
    finding goes through one atomicMin on (code << 56) | position, so the record holds the smallest of all."""
    ix, (_, k) = _broken(('order', 3, 1), ('range', 200, 2))
    _refused(target, bits, ix, _text('range', target, 200, k), inverse)
    _valid(target, bits, inverse)
    ix, (k, _) = _broken(('range', 7, 1), ('range', 150, 3))
    _refused(target, bits, ix, _text('range', target, 7, k), inverse)
    _valid(target, bits, inverse)


@pytest.mark.parametrize('bits', [32, 64])
@pytest.mark.parametrize('target', ['csr_mirror', 'fsai'])
def test_missing_partner(target, bits, inverse):
    """(e) Without the stored entry (LONG, 268), past the 64th of the long row, the entry (268, LONG) has no partner."""
    i, j = 268, LONG
    rows = np.repeat(np.arange(N), np.diff(IP))
    keep = ~((rows == j) & (IX == i))
    assert keep.sum() == A.nnz - 1
    B = sp.csr_matrix((A.data[keep], (rows[keep], IX[keep])), shape=A.shape)
    B.sort_indices()
    rc, h = _create(target, bits, B.indptr.astype(np.int64), B.indices.astype(np.int64), values=B.data)
    assert rc != 0 and not h.value
    assert _L().rlh_last_error().decode() == ('%s: the stored structure is not symmetric: entry (%d, %d) has no partner '
                                              '(%d, %d); the device build creates no entries' % (NAMES[target], i, j, j, i))
    _valid(target, bits, inverse)


@pytest.mark.parametrize('bits', [32, 64])
def test_indptr_violations(bits, inverse):
    """The indptr check past its first workgroup (row 290), on every target."""
    ip = IP.copy()
    ip[291] = ip[290] - 1
    for target in TARGETS:
        _refused(target, bits, IX, 'indptr decreases at row 290', inverse, ip=ip)
        _valid(target, bits, inverse)


@pytest.mark.parametrize('bits', [32, 64])
def test_empty_inputs(bits):
    """(g) No rows, and rows without entries, with any number of columns: valid builds."""
    L = _L()
    none = np.zeros(0, dtype=np.int64)
    for n_rows, n_cols in ((0, 0), (0, 5), (3, 0), (3, 7), (N, 2)):
        ip = np.zeros(n_rows + 1, dtype=np.int64)
        rc, h = _create('spd', bits, ip, none, n=n_rows, n_cols=n_cols)
        _check(rc)
        count = ctypes.c_int64(-1)
        _check(L.rlh_spd_info(h, None, None, ctypes.byref(count), None))
        assert h.value and count.value == 0
        for transp, (nx, ny) in enumerate(((n_cols, n_rows), (n_rows, n_cols))):
            if nx and ny:                                   # a product with the empty operator: zeros
                x, y = _dev(np.ones(nx)), _dev(np.full(ny, 7.5))
                _check(L.rlh_spd_apply(h, transp, 1, x.ptr, nx, y.ptr, ny, None, None))
                from raleigh_amd import _lib
                out = np.empty(ny)
                _check(L.rlh_d2h(_lib.host_ptr(out), y.ptr, out.nbytes))
                assert not out.any()
        L.rlh_spd_destroy(h)
        if n_cols != 2:
            rc, h = _create('csr', bits, ip, none, n=n_rows, n_cols=n_cols)
            _check(rc)
            assert h.value
            L.rlh_csr_destroy(h)
    rc, h = _create('fsai', bits, np.zeros(1, dtype=np.int64), none, n=0)
    _check(rc)
    assert h.value
    _check(_create('update', bits, np.zeros(1, dtype=np.int64), none, n=0, inverse=h)[0])
    L.rlh_fsai_destroy(h)
