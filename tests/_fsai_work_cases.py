"""The approximate inverse's own application (rlh_fsapply_*, ApproximateInverse(work=...)): cases shared by the CPU tier
(tests/fake_fsai.py) and the GPU tier.  Matrices and helpers come from tests/_fsai_cases.py.

THE BOUND OF AN APPLICATION.  T: the type of X and Y; V: the stored values (G~ = G rounded once to V, which the test
does itself: the reference is G~^H (G~ X) in longdouble, so rounding G is no error); Wt: the type of W = G~ X.  A row of
G~ has at most a entries, a row of G~^H at most b.  The library forms w_i = sum_j g_ij x_j in T by fused multiply-adds:
|fl(w) - w| <= gamma_a |G~| |x| (Higham, Accuracy and Stability, (3.5)), rounds it once to Wt when Wt differs from T
(relative uW), and forms y = G~^H w the same way (gamma_b, plus one addition where a row's tail is added to its sliced
part).  To first order
    |y - exact| <= ((a + b + 1) uT + uW) |G~|^H (|G~| |X|);
the bound asserted is ((a + b + 2) uT' + 2 uW') |G~|^H (|G~| |X|), whose extra uT and doubled uW take the second-order
terms (and, for bfloat16, the rounding to float32 that precedes the one to bfloat16).  u' = u for real types and 4 u
for complex ones (Higham Lemma 3.5: a complex product carries sqrt(2) gamma_2 < 4 u).  uW = 2^-8 for bfloat16 and
2^-24 for float32; the term is present only when Wt differs from T.  Nothing in it is measured.
"""

import ctypes
import functools
import math

import numpy as np
import pytest
import scipy.sparse as sp

from _fsai_cases import N, TYPES, _L, _check, _with_profile, create, destroy, dev, fetch, get, last_error, matrix, unit

WORKS = {'native': 0, 'float32': 1, 'bf16': 2}
PAIRS = [(code, work) for code in 'sdcz' for work in WORKS if not (work == 'bf16' and code in 'cz')]
VECTORS = (1, 3, 8, 17, 33, 65)
GUARD = 2


# ---------------------------------------------------------------- the raw entry points
def plan_create(h, work):
    p = ctypes.c_void_p(12345)
    return _L().rlh_fsapply_create(ctypes.byref(p), h, work), p


def plan_destroy(p):
    _L().rlh_fsapply_destroy(p)


def plan_info(p):
    work, slots, tail, nbytes = ctypes.c_int(-1), ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
    _check(_L().rlh_fsapply_info(p, ctypes.byref(work), ctypes.byref(slots), ctypes.byref(tail), ctypes.byref(nbytes)))
    return dict(work=work.value, slots=slots.value, tail=tail.value, bytes=nbytes.value)


def run(p, m, x, ldx, y, ldy):
    return _L().rlh_fsapply_run(p, m, x, ldx, y, ldy)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---------------------------------------------------------------- the reference
def stored_type(dt, work):
    dt = np.dtype(dt)
    if work == 'native':
        return dt.type
    return np.complex64 if dt.kind == 'c' else np.float32


def work_unit(dt, work):
    """uW', or 0 where W is kept in T."""
    dt = np.dtype(dt)
    if work == 'bf16':
        return 2.0 ** -8
    if work == 'float32' and dt.itemsize // (2 if dt.kind == 'c' else 1) == 8:
        return 2.0 ** -24 * (4 if dt.kind == 'c' else 1)
    return 0.0


class Reference:
    """G~^H (G~ X) in longdouble and the bound of the module docstring, for G as fetched from the handle."""

    def __init__(self, G, dt, work):
        dt = np.dtype(dt)
        self.dt, self.wide = dt, np.clongdouble if dt.kind == 'c' else np.longdouble
        Gt = sp.csr_matrix(G.astype(stored_type(dt, work)))
        dense = Gt.toarray()
        self.Gd = dense.astype(self.wide)
        self.Ga = np.abs(dense).astype(np.float64)
        a = int(np.diff(G.indptr).max()) if G.nnz else 0
        b = int(np.diff(sp.csc_matrix(G).indptr).max()) if G.nnz else 0
        self.a, self.b = a, b
        ut = unit(dt) * (4 if dt.kind == 'c' else 1)
        self.coef = (a + b + 2) * ut + 2 * work_unit(dt, work)

    def exact(self, x):
        """x: (m, n), one vector per row."""
        return (np.conj(self.Gd.T) @ (self.Gd @ x.astype(self.wide).T)).T

    def bound(self, x):
        return self.coef * (self.Ga.T @ (self.Ga @ np.abs(x).astype(np.float64).T)).T

    def check(self, x, y, exact=None):
        exact = self.exact(x) if exact is None else exact
        err, bound = np.abs(y.astype(self.wide) - exact).astype(np.float64), self.bound(x)
        assert np.all(err <= bound), float(np.max(err / np.maximum(bound, 1e-300)))
        return float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0


def random_block(rng, m, n, dt):
    x = rng.standard_normal((m, n))
    if np.dtype(dt).kind == 'c':
        x = x + 1j * rng.standard_normal((m, n))
    return x.astype(dt)


def padded(x, ld, lead=0):
    """x (m, n) as a flat column-major block of leading dimension ld with NaN in the padding rows and in GUARD guard
    columns, behind `lead` NaN elements."""
    m, n = x.shape
    out = np.full((m + GUARD, ld), np.nan, dtype=x.dtype)
    out[:m, :n] = x
    return np.concatenate([np.full(lead, np.nan, dtype=x.dtype), out.reshape(-1)])


def checked_application(plan, ref, n, vectors, seed, alone=()):
    """The checks of one plan over blocks of `vectors` vectors (the first m of one random block); alone: (m, columns) --
    these columns of the call with m vectors are compared with the same vectors applied alone."""
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
        assert run(plan, m, X.ptr, ld, Y.ptr, ldy) == 0, last_error()
        y = fetch(Y, hy.size, dt).reshape(m + GUARD, ldy)
        assert np.array_equal(bits(fetch(X, hx.size, dt)), bits(hx))                # X is unchanged
        assert np.all(np.isnan(y[:, n:])) and np.all(np.isnan(y[m:, :]))            # guards
        worst = max(worst, ref.check(x, y[:m, :n], exact[:m]))
        Y2 = dev(hy)                                                                # again: equal bits
        assert run(plan, m, X.ptr, ld, Y2.ptr, ldy) == 0, last_error()
        assert np.array_equal(bits(fetch(Y2, hy.size, dt)), bits(y.reshape(-1)))
        # the same block one element further on (X and Y only element-aligned)
        X1, Y1 = dev(padded(x, ld, lead=1)), dev(np.full(hy.size + 1, np.nan, dtype=dt))
        assert run(plan, m, X1.ptr + es, ld, Y1.ptr + es, ldy) == 0, last_error()
        y1 = fetch(Y1, hy.size + 1, dt)
        assert np.isnan(y1[0]) and np.array_equal(bits(y1[1:]), bits(y.reshape(-1)))
        if alone and m == alone[0]:
            for j in alone[1]:
                Yj = dev(np.full(ldy + 1, np.nan, dtype=dt))
                assert run(plan, 1, X.ptr + j * ld * es, ld, Yj.ptr, ldy) == 0, last_error()
                yj = fetch(Yj, ldy + 1, dt)
                assert np.array_equal(bits(yj[:n]), bits(y[j, :n])) and np.all(np.isnan(yj[n:])), j
        assert run(plan, m, X.ptr, ld, X.ptr, ld) == 0, last_error()                # in place
        z = fetch(X, hx.size, dt).reshape(m + GUARD, ld)
        assert np.array_equal(bits(z[:m, :n]), bits(y[:m, :n]))
        assert np.all(np.isnan(z[:, n:])) and np.all(np.isnan(z[m:, :]))
    print('largest error / bound: %.3g (a = %d, b = %d, coefficient %.3g)' % (worst, ref.a, ref.b, ref.coef))


def with_plan(A, work, body):
    """body(handle, plan, G) on a level-1 build of A and a plan of this work form."""
    rc, h = create(A, bits=32)
    _check(rc)
    try:
        G = get(h, A.dtype.type)
        rc, p = plan_create(h, WORKS[work])
        _check(rc)
        try:
            assert plan_info(p)['work'] == WORKS[work]
            return body(h, p, G)
        finally:
            plan_destroy(p)
    finally:
        destroy(h)


# ---------------------------------------------------------------- 1: application, raw ABI
def application(code, work):
    A = matrix(code)
    assert N % 64 != 0

    def body(h, p, G):
        f = plan_info(p)
        sliced = 2 * G.nnz - f['tail']                       # entries of G and G^H outside the tails
        assert 0 <= f['tail'] and sliced <= f['slots'] <= 2 * sliced
        checked_application(p, Reference(G, TYPES[code], work), N, VECTORS, 31, alone=(33, (0, 7, 8, 32)))
    with_plan(A, work, body)


# ---------------------------------------------------------------- 2: small and edge sizes
def small_sizes(n, work):
    A = _with_profile(n, (1, 2, 9), np.float64, 40 + n)
    with_plan(A, work, lambda h, p, G: checked_application(p, Reference(G, np.float64, work), n, (1, 9), 32, alone=(9, (0, 8))))


def empty_sizes():
    dt = np.float64
    # m = 0 on a plan of the n = 777 matrix: nothing is touched
    def body(h, p, G):
        hy = np.full(N + 5, np.nan)
        X, Y = dev(np.ones(N + 5)), dev(hy)
        assert run(p, 0, X.ptr, N + 5, Y.ptr, N + 5) == 0
        assert np.all(np.isnan(fetch(Y, hy.size, dt)))
    with_plan(matrix('d'), 'native', body)
    # n = 0: a valid empty plan
    A = sp.csr_matrix((0, 0), dtype=dt)
    rc, h = create(A, bits=32)
    _check(rc)
    try:
        for work in WORKS.values():
            rc, p = plan_create(h, work)
            assert rc == 0 and p.value, last_error()
            f = plan_info(p)
            assert f['slots'] == 0 and f['tail'] == 0 and f['work'] == work
            Y = dev(np.full(4, np.nan))
            assert run(p, 3, Y.ptr, 0, Y.ptr, 0) == 0
            assert np.all(np.isnan(fetch(Y, 4, dt)))
            plan_destroy(p)
    finally:
        destroy(h)


# ---------------------------------------------------------------- 3: long rows of G^H and the memory condition
@functools.lru_cache(maxsize=None)
def arrowhead(n=2049):
    """Row and column 0 full with small entries, a tridiagonal part, strictly diagonally dominant: column 0 of G (lower
    triangular on the pattern of tril(A)) has n entries, so row 0 of G^H has."""
    rng = np.random.default_rng(5)
    i = np.arange(1, n)
    rows = np.concatenate([i, i[1:]])
    cols = np.concatenate([np.zeros(n - 1, dtype=np.int64), i[1:] - 1])
    vals = np.concatenate([rng.uniform(0.5, 1.0, n - 1) / n, rng.uniform(-1.0, 1.0, n - 2)])
    low = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    off = low + low.T
    diag = np.asarray(abs(off).sum(axis=1)).ravel() + 1.0 + rng.uniform(0.0, 1.0, n)
    A = sp.csr_matrix(off + sp.diags(diag)).astype(np.float64)
    A.sort_indices()
    return A


def long_rows(work):
    A = arrowhead()
    n = A.shape[0]

    def body(h, p, G):
        assert int(np.diff(sp.csc_matrix(G).indptr).max()) == n
        f = plan_info(p)                                   # (before the first product: W is not there yet)
        sv = np.dtype(stored_type(np.float64, work)).itemsize
        print('slots %d, tail entries %d, %d bytes held; nnz(G) = %d' % (f['slots'], f['tail'], f['bytes'], G.nnz))
        assert f['tail'] > 0
        assert f['bytes'] <= 2 * (G.nnz + G.nnz) * (4 + sv) + 64 * n + 4096
        ref = Reference(G, np.float64, work)
        assert ref.b == n
        checked_application(p, ref, n, (1, 17), 33, alone=(17, (0, 16)))
    with_plan(A, work, body)


# ---------------------------------------------------------------- 4: padding is never read
def nan_row(work, j=300):
    A = matrix('d')
    m, ld = 9, N + 5

    def body(h, p, G):
        x = random_block(np.random.default_rng(34), m, N, np.float64)
        xn = x.copy()
        xn[:, j] = np.nan
        out = []
        for block in (x, xn):
            X, Y = dev(padded(block, ld)), dev(np.full((m + GUARD) * ld, np.nan))
            assert run(p, m, X.ptr, ld, Y.ptr, ld) == 0, last_error()
            out.append(fetch(Y, (m + GUARD) * ld, np.float64).reshape(m + GUARD, ld)[:m, :N])
        y, yn = out
        S = sp.csr_matrix((np.ones(G.nnz), G.indices, G.indptr), shape=G.shape)        # every stored entry is multiplied
        hit = np.asarray((S.T @ S)[:, [j]].todense()).ravel() > 0
        assert hit[j] and 0 < hit.sum() < N
        assert np.all(np.isfinite(y))
        assert np.all(np.isnan(yn[:, hit])) and np.array_equal(bits(yn[:, ~hit]), bits(y[:, ~hit]))
    with_plan(A, work, body)


# ---------------------------------------------------------------- 5: refusals
def _refused(rc, p, text):
    assert rc != 0 and not p.value, text
    assert text in last_error(), (text, last_error())


def refusals_raw():
    rc, h = create(matrix('d'), bits=32)
    _check(rc)
    rc, hz = create(matrix('z'), bits=32)
    _check(rc)
    try:
        _refused(*plan_create(h, 3), 'rlh_fsapply_create: work must be 0 (native), 1 (float32) or 2 (bf16), got 3')
        _refused(*plan_create(h, -1), 'rlh_fsapply_create: work must be')
        _refused(*plan_create(hz, 2), 'rlh_fsapply_create: bfloat16 work blocks are for real types only')
        _refused(*plan_create(None, 0), 'rlh_fsapply_create: null handle')
        rc, p = plan_create(h, 0)
        _check(rc)
        try:
            X = dev(np.ones(2 * (N + 5)))
            for args, text in (((2, None, N + 5, X.ptr, N + 5), 'rlh_fsapply_run: null pointer'),
                               ((2, X.ptr, N + 5, None, N + 5), 'rlh_fsapply_run: null pointer'),
                               ((2, X.ptr, N - 1, X.ptr, N + 5), 'rlh_fsapply_run: Matrix and vectors dimensions incompatible'),
                               ((-1, X.ptr, N + 5, X.ptr, N + 5), 'rlh_fsapply_run: negative number of vectors')):
                assert run(p, *args) != 0 and text in last_error(), (text, last_error())
            assert _L().rlh_fsapply_run(None, 1, X.ptr, N, X.ptr, N) != 0 and 'rlh_fsapply_run: null plan' in last_error()
            assert np.array_equal(fetch(X, 2 * (N + 5), np.float64), np.ones(2 * (N + 5)))
        finally:
            plan_destroy(p)
    finally:
        destroy(h)
        destroy(hz)


def refusals_class(calls=None):
    """calls: the stand-in's counters on the CPU tier."""
    from raleigh_amd.algebra.hip import Vectors
    from raleigh_amd.algebra.hip.precond import ApproximateInverse
    A = matrix('d')
    with pytest.raises(ValueError, match='work must be'):
        ApproximateInverse(A, work='float16')
    with pytest.raises(ValueError, match='work must be'):
        ApproximateInverse(A, work=1)
    before = dict(calls) if calls is not None else None
    with pytest.raises(ValueError, match='real matrices only'):
        ApproximateInverse(matrix('z'), work='bf16')
    if calls is not None:
        assert dict(calls) == before                         # refused before any library call
    T = ApproximateInverse(A, work='bf16')
    plain = ApproximateInverse(A)
    assert T.device_bytes() > plain.device_bytes()
    assert T.algorithmic_bytes(4) == 2 * T.nnz * (4 + 4) + N * 4 * (2 * 8 + 2 * 2)
    assert ApproximateInverse(A, work='native').algorithmic_bytes(4) == 2 * T.nnz * (8 + 4) + N * 4 * (2 * 8 + 2 * 8)
    assert ApproximateInverse(matrix('c'), work='float32').algorithmic_bytes(4) == 2 * T.nnz * (8 + 4) + N * 4 * 4 * 8
    assert plain.algorithmic_bytes(4) == 2 * T.nnz * 12 + 4 * N * 4 * 8
    x = Vectors(np.ones((3, N)))
    with pytest.raises(ValueError, match='data types differ'):
        T.apply(Vectors(np.ones((3, N), dtype=np.float32)), x)
    with pytest.raises(ValueError, match='dimensions incompatible'):
        T.apply(Vectors(np.ones((3, N + 1))), x)
    with pytest.raises(ValueError, match='vectors differ'):
        T.apply(Vectors(np.ones((2, N))), x)

    class Sharded:
        comm = object()
    with pytest.raises(ValueError, match='row-sharded'):
        T.apply(Sharded(), x)
    G = T.csr()
    assert G.dtype == np.float64 and np.array_equal(bits(G.data), bits(plain.csr().data))      # the handle keeps G
    y, y0 = Vectors(np.zeros((3, N))), Vectors(np.zeros((3, N)))
    if calls is not None:
        before = dict(calls)
    plain.apply(x, y0)
    if calls is not None:                                     # work=None: the calls it always made, and no other
        assert calls.get('fsapply_run', 0) == before.get('fsapply_run', 0)
        assert calls.get('fsai_apply', 0) == before.get('fsai_apply', 0) + 1
        assert before.get('fsapply_create', 0) == 3           # bf16, native and float32 above; none for work=None
    T.apply(x, y)
    if calls is not None:
        assert calls.get('fsapply_run', 0) == before.get('fsapply_run', 0) + 1
        assert calls.get('fsai_apply', 0) == before.get('fsai_apply', 0) + 1
    Reference(G, np.float64, 'bf16').check(np.ones((3, N)), y.data())
    T.apply(x, x)
    assert np.array_equal(x.data(), y.data())


# ---------------------------------------------------------------- 6: device memory (GPU tier)
def device_memory():
    def live():
        nbytes, nblocks = ctypes.c_int64(-1), ctypes.c_int64(-1)
        _check(_L().rlh_device_live(ctypes.byref(nbytes), ctypes.byref(nblocks)))
        return nbytes.value, nblocks.value
    A = matrix('d')
    first = live()
    rc, h = create(A, bits=32)
    _check(rc)
    held = live()
    assert held[0] > first[0]
    rc, p = plan_create(h, 2)
    _check(rc)
    made = live()
    assert made[0] - held[0] == plan_info(p)['bytes'] > 0
    X = dev(np.ones(33 * N))
    for m in (8, 33):                                       # W grows once
        assert run(p, m, X.ptr, N, X.ptr, N) == 0, last_error()
        assert live()[0] - held[0] == plan_info(p)['bytes'] == made[0] - held[0] + ((m + 7) // 8) * N * 8 * 2
    plan_destroy(p)
    assert live() == held
    destroy(h)
    assert live() == first


# ---------------------------------------------------------------- 7: end to end
def end_to_end(device, as_tensor=True, record=None):
    """record: a list that receives (work, iterations) of every run."""
    import scipy.linalg
    from raleigh_amd.synthetic import fe_surrogate
    from raleigh_amd.interfaces import partial_hevp
    from raleigh_amd.algebra.hip.precond import ApproximateInverse
    from _device_data_cases import csr_tensor, host
    from _device_operator_cases import TOL, _residual
    from _fsai_cases import hermitian_from_upper
    A = sp.csr_matrix(fe_surrogate(grid=(7, 6, 5))).astype(np.float64)
    A.sort_indices()
    which = 6
    exact = scipy.linalg.eigvalsh(hermitian_from_upper(A).toarray())[:which]
    a = csr_tensor(A, device) if as_tensor else A
    np.random.seed(1)
    lmd_ref, x_ref, status_ref = partial_hevp(A, T=True, which=which, tol=TOL, verb=-1)
    assert status_ref == 0
    res_ref = _residual(A, None, lmd_ref[:which], x_ref[:, :which])
    its = {}
    for work in WORKS:
        T = ApproximateInverse(a, work=work)
        np.random.seed(1)
        lmd, x, status = partial_hevp(a, T=T, which=which, tol=TOL, verb=-1)
        its[work] = partial_hevp.last['iterations']
        assert status == 0
        assert np.max(np.abs(lmd[:which] - exact)) <= 1e-10
        if as_tensor:
            x = host(x)
        res = _residual(A, None, lmd[:which], x[:, :which].astype(np.float64))
        print('work=%s: %d iterations, residual %.3e (no preconditioner: %.3e)' % (work, its[work], res, res_ref))
        assert res <= 10 * res_ref
        if record is not None:
            record.append((work, its[work]))
    print('iterations: native %d, float32 %d, bf16 %d' % (its['native'], its['float32'], its['bf16']))
    for work in WORKS:
        assert its[work] <= math.ceil(1.1 * its['native']), its
