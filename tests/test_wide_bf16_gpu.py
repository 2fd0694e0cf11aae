"""GPU tier: the fused Chebyshev step on bfloat16 work blocks against float32 operators in the 256-row interleaved
layout (wide_cheb_bf16_kernel, reached through rlh_spmm_cheb_bf16_part), cases of tests/_wide_bf16_cases.py.

Every block is a Bf16Block with one guard vector past m; its padding rows (n .. ld - 1) and the guard vector hold the
NaN pattern 0x7fc0 and must come back unchanged, y and b must come back unchanged bit for bit, and no NaN may appear
in p.  Every test here fails without the kernel: the library refuses the layout (RlhError) and supports_bf16() is
false."""

import ctypes
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import ops
import _wide_bf16_cases as cases

pytestmark = pytest.mark.gpu


def _L():
    from raleigh_amd import _lib
    return _lib.lib()


def _check(rc):
    from raleigh_amd import _lib
    _lib.check(rc)


class _Env:
    """Environment of a build or a launch (the library reads it at the call); restored on exit."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        for k, v in self.kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _upload(values, m, rows_alloc=None):
    """A Bf16Block of m vectors + a guard vector: values (m, n) in it, the NaN pattern everywhere else."""
    from raleigh_amd import _lib
    from raleigh_amd.algebra.hip.sparse import Bf16Block
    n = values.shape[1] if rows_alloc is None else rows_alloc
    blk = Bf16Block(n, m + 1)
    img = np.full((m + 1, blk.ld), cases.NAN16, dtype=np.uint16)
    img[:m, :values.shape[1]] = ops.bf16_bits(values[:m])
    _check(_L().rlh_h2d(blk.ptr(), _lib.host_ptr(img), img.nbytes))
    return blk, img


def _download(blk, m):
    from raleigh_amd import _lib
    out = np.empty((m + 1, blk.ld), dtype=np.uint16)
    _check(_L().rlh_d2h(_lib.host_ptr(out), blk.ptr(), out.nbytes))
    return out


def _step(op, m, y, p, b, coeff, rows, **kw):
    """One step on fresh blocks; returns p's rows as float32 after the checks every call must pass."""
    (yb, y0), (pb, p0), (bb, b0) = _upload(y, m), _upload(p, m), _upload(b, m)
    op.cheb_step_bf16(m, yb, pb, bb, *coeff, **kw)
    assert np.array_equal(_download(yb, m), y0) and np.array_equal(_download(bb, m), b0)        # inputs untouched
    p1 = _download(pb, m)
    assert np.array_equal(p1[m], p0[m]) and np.array_equal(p1[:, rows:], p0[:, rows:])          # guard vector, padding rows
    got = ops.bf16_from_bits(p1[:m, :rows])
    assert not np.any(np.isnan(got))
    return got


_BUILD_ENV = {'d1': {'RLH_WIDE_PAIR': 0}}


@functools.lru_cache(maxsize=None)
def _operator(name, exact=False, fmt='wide'):
    """Host-built operator of the full CSR (kept for the module: the launch variants are chosen at call time)."""
    from raleigh_amd.algebra.hip import CsrOperator
    with _Env(RLH_SPMM_FORMAT=fmt, **_BUILD_ENV.get(name, {})):
        op = CsrOperator(cases.matrix(name, exact))
    if fmt == 'wide':
        assert op.layout()[0] == 'wide' and op.bf16_ready()
    return op


def _device_bytes(op):
    nb = ctypes.c_int64()
    _check(_L().rlh_csr_info(op._h, None, None, None, ctypes.byref(nb)))
    return nb.value


def _half_positions():
    """Bytes of half the position array of the unpaired handle of (d)."""
    return (_operator('d1').layout()[1] // (8 * 256) + 4) * 128 * 16


def test_row_pair_form_is_taken():
    """(d) The C ABI does not say how many rows a thread owns, so the pair form is told by the handle's size: the paired
    layout stores one 16-byte piece of positions per row PAIR and chunk, the unpaired one per row and chunk (chunks = stored
    slots / (8 * 256) + the build's 4 chunks of padding), so the handle of the same matrix built with RLH_WIDE_PAIR=0 is
    larger by half its positions.  (tests/test_device_operator_gpu.py::test_pairing_rule_applies tells it the same way; the
    device-built handle of (d) is held to the size of the paired host-built one in test_device_built.)"""
    paired, single = _device_bytes(_operator('d')), _device_bytes(_operator('d1'))
    assert single - paired > 0.9 * _half_positions(), (paired, single)


def _variants(m):
    """(NV, VS, VEC) to force: every instantiation that the launcher can reach for this m (VS matters from NV = 16 on;
    the row-pair form has one VS per NV and ignores it)."""
    out = []
    for nv in (8, 16, 32):
        for vs in ((1,) if nv == 8 else (1, 2)):
            for vec in (1, 0):
                out.append((nv, vs, vec))
    return out


@pytest.mark.parametrize('m', cases.VECTORS)
@pytest.mark.parametrize('name', cases.NAMES)
def test_rounding_bound(name, m):
    """1. |got - ref| <= 2^-8 |ref| + (L + 4) 2^-24 (|cy y| + |cp p| + |cb| (|b| + sum |a| |y|)) for every element,
    ref in float64 on the same bfloat16 inputs (cases.rounding_bound: derived, not measured)."""
    A = cases.matrix(name)
    n = A.shape[0]
    y, p, b = cases.inputs(name)
    ref, mag = cases.rounding_reference(name)
    bound = cases.rounding_bound(A, ref[:m], mag[:m])
    op = _operator(name)
    worst = 0.0
    for nv, vs, vec in _variants(m):
        with _Env(RLH_WIDE_NV=nv, RLH_WIDE_VS=vs, RLH_SPMM_VEC=vec):
            got = _step(op, m, y, p, b, cases.COEFF, n)
        err = np.abs(got.astype(np.float64) - ref[:m])
        worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
        assert np.all(err <= bound), (name, m, nv, vs, vec, worst)
    print('%s m=%d: largest error / bound %.3f' % (name, m, worst))


@pytest.mark.parametrize('name', cases.NAMES)
def test_exact(name):
    """2. Small integers: every partial sum is an integer below 256, so p is the exact result whatever the order of
    the sums; compared as values (+-0)."""
    n = cases.matrix(name, True).shape[0]
    y, p, b = cases.inputs(name, True)
    want = cases.exact_reference(name)
    op = _operator(name, True)
    for m in cases.VECTORS:
        for vec in (1, 0):
            with _Env(RLH_SPMM_VEC=vec):
                got = _step(op, m, y, p, b, (1.0, -1.0, 1.0), n)
            assert np.array_equal(got.astype(np.float64), want[:m]), (name, m, vec)
    if name == 'a':                                   # the default build: the 1024-row windowed layout
        well = _operator('a', True, None)
        assert well.layout()[0] == 'well' and well.bf16_ready()
        for m in cases.VECTORS:
            assert np.array_equal(_step(well, m, y, p, b, (1.0, -1.0, 1.0), n).astype(np.float64), want[:m]), m


@pytest.mark.parametrize('index', [np.int32, np.int64])
@pytest.mark.parametrize('name', ['a', 'd'])
def test_device_built(name, index):
    """3. The operator built on the device from a torch.sparse_csr tensor takes the step and gives the bits of the
    host-built interleaved handle (the two builds leave identical arrays)."""
    torch = pytest.importorskip('torch')
    assert torch.cuda.is_available()
    from raleigh_amd.algebra.hip import SparseSymmetricMatrix
    from _device_data_cases import csr_tensor
    A = cases.matrix(name)
    n = A.shape[0]
    y, p, b = cases.inputs(name)
    dev = SparseSymmetricMatrix(csr_tensor(A, 'cuda', index))
    assert dev.supports_bf16() and dev.layout()[0] == 'wide'
    with _Env(RLH_SPMM_FORMAT='wide'):
        hst = SparseSymmetricMatrix(A)
    assert hst.supports_bf16() and hst.layout()[0] == 'wide'
    if name == 'd':                                   # both builds took the pair form (see test_row_pair_form_is_taken)
        for op in (dev, hst):
            assert _device_bytes(_operator('d1')) - _device_bytes(op._SparseSymmetricMatrix__op) > 0.9 * _half_positions()
    ref, mag = cases.rounding_reference(name)
    for m in (13, 16, 33):
        got = _step(dev, m, y, p, b, cases.COEFF, n)
        assert np.array_equal(got.view(np.uint32), _step(hst, m, y, p, b, cases.COEFF, n).view(np.uint32)), (name, m)
        assert np.all(np.abs(got.astype(np.float64) - ref[:m]) <= cases.rounding_bound(A, ref[:m], mag[:m]))


def test_row_shard():
    """4. A row window of (a) as a shard: own columns from y, the others from a bfloat16 halo block.  Part 1, handed
    NaNs for the halo, writes the rows of the interior blocks only and no NaN; parts 1 + 2 are part 0 bit for bit; a
    halo block with an odd leading dimension is refused."""
    from raleigh_amd import _lib
    from raleigh_amd.algebra.hip import CsrOperator
    A = cases.matrix('a')
    n = A.shape[0]
    r0, r1 = 2000, 5200
    loc = sp.csr_matrix(A[r0:r1])
    used = np.unique(loc.indices)
    halo = used[(used < r0) | (used >= r1)]
    nown = r1 - r0
    assert nown % 8 == 0
    nh = -(-len(halo) // 8) * 8
    newcol = np.full(n, -1, dtype=np.int64)
    newcol[r0:r1] = np.arange(nown)
    newcol[halo] = nown + np.arange(len(halo))
    L = sp.csr_matrix((loc.data, newcol[loc.indices].astype(np.int32), loc.indptr), shape=(nown, nown + nh))
    L.sort_indices()
    with _Env(RLH_SPMM_FORMAT='wide'):
        op = CsrOperator(L, n_own=nown)
    assert op.layout()[0] == 'wide'
    m = 13
    yfull, pfull, bfull = cases.inputs('a')
    y, p, b = yfull[:, r0:r1], pfull[:, r0:r1], bfull[:, r0:r1]
    hval = np.zeros((m, nh), dtype=np.float32)
    hval[:, :len(halo)] = yfull[:m, halo]
    hgood, _ = _upload(hval, m)
    hbad, _ = _upload(np.full((m, nh), np.nan, dtype=np.float32), m)
    assert hgood.ld >= nh and op.bf16_ready(hgood.ld) and not op.bf16_ready(hgood.ld + 1)
    # the blocks of 256 rows that reference no halo column
    maxcol = np.array([L.indices[L.indptr[r]:L.indptr[min(r + 256, nown)]].max() for r in range(0, nown, 256)])
    interior = np.repeat(maxcol < nown, 256)[:nown]
    assert interior.any() and not interior.all()

    def run(parts):
        (yb, y0), (pb, p0), (bb, b0) = _upload(y, m), _upload(p, m), _upload(b, m)
        out = []
        for part, h in parts:
            op.cheb_step_bf16(m, yb, pb, bb, *cases.COEFF, h.ptr(), h.ld, part=part)
            p1 = _download(pb, m)
            assert np.array_equal(p1[m], p0[m]) and np.array_equal(p1[:, nown:], p0[:, nown:])
            assert not np.any(np.isnan(ops.bf16_from_bits(p1[:m, :nown])))
            out.append(p1[:m, :nown])
        assert np.array_equal(_download(yb, m), y0) and np.array_equal(_download(bb, m), b0)
        return out, p0[:m, :nown]

    (whole,), start = run([(0, hgood)])
    (first, both), _ = run([(1, hbad), (2, hgood)])
    assert np.array_equal(first[:, ~interior], start[:, ~interior])             # part 1 left the boundary rows alone
    assert np.array_equal(first[:, interior], whole[:, interior])
    assert not np.array_equal(first[:, interior], start[:, interior])
    assert np.array_equal(both, whole)
    ref, mag = cases.step_reference(L, y[:m], p[:m], b[:m], cases.COEFF, halo=hval)
    assert np.all(np.abs(ops.bf16_from_bits(whole).astype(np.float64) - ref) <= cases.rounding_bound(L, ref, mag))
    odd, _ = _upload(np.zeros((m, nh + 8), dtype=np.float32), m)
    (yb, _), (pb, _), (bb, _) = _upload(y, m), _upload(p, m), _upload(b, m)
    with pytest.raises(_lib.RlhError, match='a halo block needs n_own and ldh to be multiples of 8'):
        op.cheb_step_bf16(m, yb, pb, bb, *cases.COEFF, odd.ptr(), nh + 1, part=0)


def test_end_to_end(monkeypatch):
    """5. partial_hevp on a tensor with the preconditioner's work blocks in float32 and in bfloat16."""
    torch = pytest.importorskip('torch')
    assert torch.cuda.is_available()
    cases.end_to_end('cuda', monkeypatch)
