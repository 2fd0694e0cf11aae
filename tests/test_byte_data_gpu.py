"""GPU tier: the 8-bit data operator (rlh_bytes_*: bytes in HBM, products on the bfloat16 matrix cores with the
block split exactly into three bfloat16 planes) against float64 NumPy, and the cases of tests/_byte_data_cases.py
on the device."""

import ctypes

import numpy as np
import pytest

import _byte_data_cases as cases

pytestmark = pytest.mark.gpu

_KINDS = [np.uint8, np.int8]
# every value of {1, 37, 64, 300, 1000, 4099} as the number of rows and as the number of columns
_SHAPES = [(1, 1), (1, 4099), (4099, 1), (37, 64), (64, 37), (64, 64), (300, 1000), (1000, 300), (37, 4099),
           (4099, 300), (300, 37), (1000, 1000), (4099, 4099)]
_BLOCKS = [1, 7, 32, 64, 130]
E = 2.0 ** -24


def _data(rng, shape, dt):
    lo, hi = (0, 256) if dt == np.uint8 else (-128, 128)
    return rng.integers(lo, hi, size=shape).astype(dt)


def _block(rng, m, n):
    """m vectors of dimension n, the columns of the block scaled over 1e-8 .. 1e8."""
    x = rng.standard_normal((m, n)) * 10.0 ** rng.uniform(-8, 8, size=(m, 1))
    return x.astype(np.float32)


def _apply(op, x, transp, window, u=None, c=None):
    """y = Op(A) x (- u c^T) through the device operator, on windows (offset, padded leading dimension) of bigger
    blocks if `window`."""
    from raleigh_amd.algebra.hip import Vectors
    from raleigh_amd.algebra.hip.memory import DeviceBuffer
    from raleigh_amd import _lib
    m = x.shape[0]
    M, N = op.shape()
    ny = N if transp else M
    off = 3 if window else 0
    xs = np.zeros((m + 2 * off, x.shape[1]), dtype=np.float32)
    xs[off:off + m] = x
    X = Vectors(xs)
    X.select(m, off)
    Y = Vectors(ny, m + 2 * off, np.float32)
    Y.select(m, off)
    U = cb = None
    if c is not None:
        cb = DeviceBuffer(max(c.nbytes, 16))
        cc = np.ascontiguousarray(c)
        _lib.check(_lib.lib().rlh_h2d(cb.ptr, _lib.host_ptr(cc), cc.nbytes))
        if u is not None:
            U = Vectors(u[None, :])
    op.apply_r1(X, Y, transp, U, None if cb is None else cb.ptr)
    return Y.data()


def _check(y, A64, x, transp, u=None, c=None, worst=None):
    """|Y - Y64| <= 3.1 (K + 2) e (|A| |X| + |u| |c|) elementwise, e = 2^-24: three exact products per term summed
    in float32 in any order (gamma_3K of the dot-product bound, times 1 + 2^-8 + 2^-16 for |h| + |m| + |l|), plus
    the final subtraction; and the normwise 2e-4 of test_dense_apply_vs_oracle."""
    op = A64.T if transp else A64
    K = op.shape[1]
    x64 = x.astype(np.float64)
    ref = (op @ x64.T).T
    mag = (np.abs(op) @ np.abs(x64).T).T
    if c is not None:
        uu = np.ones(op.shape[0]) if u is None else u.astype(np.float64)
        ref = ref - c.astype(np.float64)[:, None] * uu[None, :]
        mag = mag + np.abs(c.astype(np.float64))[:, None] * np.abs(uu)[None, :]
    assert y.shape == ref.shape and y.dtype == np.float32
    err = np.abs(y.astype(np.float64) - ref)
    bound = 3.1 * (K + 2) * E * mag
    ratio = float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny))) if err.size else 0.0
    if worst is not None:
        worst[0] = max(worst[0], ratio)
    assert np.all(err <= bound), ratio
    nrm = np.linalg.norm(ref)
    if nrm > 0:
        assert np.linalg.norm(err) / nrm < 2e-4


@pytest.mark.parametrize('dt', _KINDS)
def test_products_against_float64(dt):
    from raleigh_amd.algebra.hip import ByteMatrix
    rng = np.random.default_rng(11)
    worst = [0.0]
    for (M, N) in _SHAPES:
        A8 = _data(rng, (M, N), dt)
        A64 = A8.astype(np.float64)
        op = ByteMatrix(A8)
        for m in _BLOCKS:
            for transp in (False, True):
                nx, ny = (M, N) if transp else (N, M)
                x = _block(rng, m, nx)
                _check(_apply(op, x, transp, window=(m != 32)), A64, x, transp, worst=worst)
                c = _block(rng, 1, m)[0]
                u = rng.standard_normal(ny).astype(np.float32)
                _check(_apply(op, x, transp, True, u, c), A64, x, transp, u, c, worst=worst)
                _check(_apply(op, x, transp, False, None, c), A64, x, transp, None, c, worst=worst)
    print('largest error / bound:', worst[0])


def test_unaligned_blocks_and_zero_sizes():
    """The C ABI itself: blocks at addresses and leading dimensions that are no multiples of 16 bytes, zero sizes
    (which return 0 and touch nothing), and argument errors (an error code and a message)."""
    from raleigh_amd import _lib
    from raleigh_amd.algebra.hip import ByteMatrix
    from raleigh_amd.algebra.hip.memory import DeviceBuffer
    L = _lib.lib()
    rng = np.random.default_rng(3)
    M, N, m = 203, 1001, 5
    A8 = _data(rng, (M, N), np.int8)
    op = ByteMatrix(A8)
    for transp in (False, True):
        nx, ny = (M, N) if transp else (N, M)
        ldx, ldy = nx + 3, ny + 1
        x = _block(rng, m, nx)
        xs = np.zeros((m, ldx), dtype=np.float32)
        xs[:, :nx] = x
        xb, yb = DeviceBuffer(4 * (m * ldx + 1)), DeviceBuffer(4 * (m * ldy + 1))
        _lib.check(L.rlh_h2d(xb.ptr + 4, _lib.host_ptr(xs), xs.nbytes))
        _lib.check(L.rlh_bytes_apply(op._h, int(transp), m, xb.ptr + 4, ldx, yb.ptr + 4, ldy, None, None))
        ys = np.zeros((m, ldy), dtype=np.float32)
        _lib.check(L.rlh_sync())
        _lib.check(L.rlh_d2h(_lib.host_ptr(ys), yb.ptr + 4, ys.nbytes))
        _check(ys[:, :ny].copy(), A8.astype(np.float64), x, transp)
        assert L.rlh_bytes_apply(op._h, int(transp), 0, None, ldx, None, ldy, None, None) == 0
        assert L.rlh_bytes_apply(op._h, int(transp), m, xb.ptr, nx - 1, yb.ptr, ldy, None, None) != 0
        assert b'incompatible' in L.rlh_last_error()
        assert L.rlh_bytes_apply(op._h, int(transp), m, xb.ptr, ldx, yb.ptr, ldy, yb.ptr, None) != 0
    assert L.rlh_bytes_apply(op._h, 2, m, None, 1, None, 1, None, None) != 0
    assert L.rlh_bytes_apply(None, 0, m, None, 1, None, 1, None, None) != 0
    h = ctypes.c_void_p()
    assert L.rlh_bytes_create(ctypes.byref(h), 2, 4, 4, _lib.host_ptr(A8), 4) != 0
    assert L.rlh_bytes_create(ctypes.byref(h), 0, 4, 4, _lib.host_ptr(A8), 3) != 0
    for shape in ((0, 5), (5, 0), (0, 0)):
        z = ByteMatrix(np.zeros(shape, dtype=np.uint8))
        assert z.shape() == shape and z.absmax() == 0.0 and z.dots().shape == (shape[0],)
        if shape == (5, 0):          # an empty sum: the rank-one term alone
            cb, yb = DeviceBuffer(16), DeviceBuffer(4 * 2 * 8)
            cc = np.array([1.0, 2.0], dtype=np.float32)
            _lib.check(L.rlh_h2d(cb.ptr, _lib.host_ptr(cc), cc.nbytes))
            _lib.check(L.rlh_bytes_apply(z._h, 0, 2, cb.ptr, 1, yb.ptr, 8, None, cb.ptr))
            _lib.check(L.rlh_sync())
            ys = np.zeros((2, 8), dtype=np.float32)
            _lib.check(L.rlh_d2h(_lib.host_ptr(ys), yb.ptr, ys.nbytes))
            assert np.array_equal(ys[:, :5], -np.array([[1.0] * 5, [2.0] * 5], dtype=np.float32))
            assert not ys[:, 5:].any()


@pytest.mark.parametrize('dt', _KINDS)
def test_exact_products_bit_for_bit(dt):
    """Where every partial sum is exactly representable the result is the float64 product rounded to float32, bit
    for bit: A and the three-plane split are exact, not just accurate.  (a) small integers times a power of two
    per vector, K = 256 (bfloat16-exact: the planes m and l vanish); (b) 12-bit integers, K = 16 (h and m);
    (c) 24-bit integers against entries 0 / 1, two per row (all three planes)."""
    from raleigh_amd.algebra.hip import ByteMatrix
    rng = np.random.default_rng(5)
    for K, xmax, amax in ((256, 16, None), (16, 4096, None), (2, 2 ** 23, 1)):
        for transp in (False, True):
            shape = (K, 200) if transp else (200, K)
            A8 = _data(rng, shape, dt) if amax is None else rng.integers(0, 2, size=shape).astype(dt)
            x = rng.integers(-xmax + 1, xmax, size=(33, K)).astype(np.float64)
            x *= 2.0 ** rng.integers(-30, 30, size=(33, 1))
            x32 = x.astype(np.float32)
            assert np.array_equal(x32.astype(np.float64), x)
            op = A8.astype(np.float64)
            ref = ((op.T if transp else op) @ x.T).T
            ref32 = ref.astype(np.float32)
            assert np.array_equal(ref32.astype(np.float64), ref)
            y = _apply(ByteMatrix(A8), x32, transp, True)
            assert np.array_equal(y.view(np.uint32), ref32.view(np.uint32)), (K, transp)


@pytest.mark.parametrize('dt', _KINDS)
def test_determinism(dt):
    from raleigh_amd.algebra.hip import ByteMatrix
    rng = np.random.default_rng(1)
    A8 = _data(rng, (3000, 5000), dt)
    op1, op2 = ByteMatrix(A8), ByteMatrix(A8)
    for transp in (False, True):
        x = _block(rng, 64, 3000 if transp else 5000)
        y1 = _apply(op1, x, transp, False)
        y2 = _apply(op1, x, transp, False)
        y3 = _apply(op2, x, transp, False)
        assert np.array_equal(y1.view(np.uint8), y2.view(np.uint8))
        assert np.array_equal(y1.view(np.uint8), y3.view(np.uint8))
    assert op1.workspace_bytes() > 0          # the reduction was split: several partial tiles summed in a fixed order


def test_memory():
    """The data take at most half of what Matrix holds for them as float32 (a condition); one copy of the bytes
    serves both products."""
    from raleigh_amd.algebra.hip import ByteMatrix
    rng = np.random.default_rng(2)
    M, N = 5000, 2003
    op = ByteMatrix(_data(rng, (M, N), np.uint8))
    for transp in (False, True):
        _apply(op, _block(rng, 130, M if transp else N), transp, False)
    held = op.device_bytes() - op.workspace_bytes()
    n16 = (N + 15) // 16 * 16
    print('data bytes held:', held, 'single copy' if held <= M * n16 + 2 ** 20 else 'two copies')
    assert held <= 2 * M * n16 + 2 ** 20
    assert held >= M * N


def test_known_values_at_size():
    """62 500 x 40 000 (one GPU's shard of the largest configuration, 2.5 GB as bytes): the ten largest singular
    values against the exactly known ones of constant blocks."""
    from raleigh_amd.interfaces import truncated_svd
    from raleigh_amd.synthetic import byte_blocks
    blocks = [(5000 - 300 * b, 3000 - 150 * b, 250 - 15 * b) for b in range(12)]
    A8, sigma = byte_blocks(blocks, shape=(62500, 40000), seed=7)
    u, s, vt = truncated_svd(A8, nsv=10)
    assert len(s) >= 10 and s.dtype == np.float32
    print('largest deviation / sigma_0:', np.max(np.abs(s[:10] - sigma[:10])) / sigma[0])
    assert np.max(np.abs(s[:10] - sigma[:10])) <= cases.TOL * sigma[0]


def test_pca_at_size_matches_float32_path():
    """62 500 x 4 096 pictures (1 GB as float32): pca(npc=50) on the bytes against the float32 path."""
    from raleigh_amd.interfaces import pca
    from raleigh_amd.synthetic import byte_images
    A8 = byte_images(62500, 4096, 50, seed=3)
    mean, trans, comps = pca(A8, npc=50, svtol=1e-8)
    sig = pca.last['sigma']
    assert trans.dtype == np.float32 and trans.shape == (62500, 50) and comps.shape == (50, 4096)
    fmean, ftrans, fcomps = pca(A8.astype(np.float32), npc=50, svtol=1e-8)
    fsig = pca.last['sigma']
    print('largest deviation / sigma_0:', np.max(np.abs(sig - fsig)) / fsig[0])
    assert np.max(np.abs(sig - fsig)) <= cases.TOL * fsig[0]
    assert np.max(np.abs(mean - fmean)) <= cases.TOL * np.abs(fmean).max()


@pytest.mark.parametrize('name', sorted(cases.IMAGES))
def test_pca_matches(name):
    cases.pca_matches(name)


@pytest.mark.parametrize('bytes_first', [False, True])
def test_pca_have(bytes_first):
    cases.pca_have(bytes_first)


def test_pca_batches():
    cases.pca_batches()


@pytest.mark.parametrize('name', sorted(cases.IMAGES))
def test_truncated_svd_matches(name):
    cases.truncated_svd_matches(name)


@pytest.mark.parametrize('shape', [None, (700, 600)])
def test_truncated_svd_norms(shape):
    cases.truncated_svd_norms(shape)


@pytest.mark.parametrize('signed', [False, True])
def test_known_values(signed):
    cases.known_values(signed)


def test_operator_surface():
    cases.operator_surface()


def test_refusals():
    cases.refusals()
