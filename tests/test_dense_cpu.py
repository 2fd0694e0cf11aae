"""CPU tier: the dense-operator cases of tests/_dense_cases.py over tests/fake_lib.py -- the harness itself (NaN poison,
guards, repeated calls, the references), the proof that NumPy in the working precision meets every bound that the GPU
tier holds the kernels to, that every exact case is exact and that the sums S stay below what the type holds exactly, the
coverage of every kernel family that route() can name under every leg, three planted kernel faults, and the child runner
of the once-per-process legs.  The stand-in takes every alignment and every switch the same way, so the legs are spread
over the types.  A machine of 4 compute units is assumed, and one of 256 for the workspace cap."""

import numpy as np
import pytest

import fake_lib
import _dense_cases as cases

KEYS = cases.KEYS
CU = 4
LEG_ENV = {
    'default': {}, 'kernel1': {'RLH_DENSE_KERNEL': '1'}, 'kernel2': {'RLH_DENSE_KERNEL': '2'},
    'kernel2_bk16': {'RLH_DENSE_KERNEL': '2', 'RLH_DENSE_BK': '16'}, 'kernel2_bk32': {'RLH_DENSE_KERNEL': '2', 'RLH_DENSE_BK': '32'},
    'd_tile22': {'RLH_DENSE_D_TILE': '22'}, 'valu': {'RLH_DENSE_VALU': '1'}}


def with_requires(fake):
    """The refusals of rlh_dense_apply_r1 (raleigh_amd/csrc/dense.hip) restated, in its order, in front of the stand-in's
    product.  The CPU test_refusals over this copy shows only that cases.refusals() is well-formed (its calls, messages and
    the untouched operands); that the LIBRARY refuses is shown by the GPU tier alone."""
    product = fake.rlh_dense_apply_r1

    def apply_r1(code, M, N, A, lda, order, transp, m, X, ldx, Y, ldy, d_u, d_c):
        addr = fake_lib._addr
        if addr(d_u) and not addr(d_c):
            return fake._fail('rlh_dense_apply_r1: a vector u without coefficients c')
        if code not in fake_lib._DT:
            return fake._fail('rlh_dense_apply: unknown dtype %d' % code)
        if M < 0 or N < 0 or m < 0:
            return fake._fail('rlh_dense_apply: negative size')
        if order not in (0, 1):
            return fake._fail('rlh_dense_apply: order must be 0 (row-major) or 1 (column-major)')
        if transp not in (0, 1):
            return fake._fail('rlh_dense_apply: transp must be 0 or 1')
        ny, nx = (N, M) if transp else (M, N)
        if m == 0 or ny == 0:
            return 0
        if not addr(Y) or (nx > 0 and not (addr(A) and addr(X))):
            return fake._fail('rlh_dense_apply: null pointer')
        if lda < (N if order == 0 else M):
            return fake._fail('rlh_dense_apply: lda too small')
        if ldx < nx or ldy < ny:
            return fake._fail('rlh_dense_apply: Matrix and vectors dimensions incompatible')
        if m > 65535 * 64:
            return fake._fail('rlh_dense_apply: too many vectors')
        return product(code, M, N, A, lda, order, transp, m, X, ldx, Y, ldy, d_u, d_c)

    return apply_r1


@pytest.fixture(autouse=True)
def fake(monkeypatch):
    for name in cases.SWITCHES:
        monkeypatch.delenv('RLH_DENSE_' + name, raising=False)
    f = fake_lib.install()
    yield f
    fake_lib.uninstall()


@pytest.mark.parametrize('key', KEYS)
def test_aligned(key):
    cases.sweep(key, 'aligned', CU)
    print(cases.ratios_text())


@pytest.mark.parametrize('key,align', [('s', 'unaligned'), ('z', 'unaligned'), ('d', 'y_unaligned'), ('c', 'tight'), ('s', 'tight'),
                                       ('s', 'window'), ('z', 'window'), ('d', 'window_rows'), ('c', 'window_odd')])
def test_alignment_and_windows(key, align):
    cases.sweep(key, align, CU)
    print(cases.ratios_text())


@pytest.mark.parametrize('key,leg', [('d', 'valu'), ('c', 'valu')])
def test_valu_shapes_on_aligned_blocks(key, leg, monkeypatch):
    for name, value in LEG_ENV[leg].items():
        monkeypatch.setenv(name, value)
    cases.sweep(key, 'aligned', CU)


@pytest.mark.parametrize('key,align', [('s', 'aligned'), ('d', 'y_unaligned'), ('c', 'aligned'), ('z', 'y_unaligned')])
def test_splits(key, align):
    cases.splits(key, CU, align)
    print(cases.ratios_text())


@pytest.mark.parametrize('key', ['s', 'd'])
def test_workspace_cap(key):
    assert cases.workspace_cap(key, 4) is not None            # (4 CUs want one split: nothing to cap, nothing is run)
    assert cases.workspace_cap(key, 256) is None
    print(cases.ratios_text())


@pytest.mark.parametrize('key', KEYS)
def test_many_row_tiles(key):
    cases.many_row_tiles(key, CU)


@pytest.mark.parametrize('key', KEYS)
def test_degenerate(key):
    cases.degenerate(key)


def test_refusals(fake, monkeypatch):
    monkeypatch.setattr(fake, 'rlh_dense_apply_r1', with_requires(fake))
    cases.refusals()


# ---------------------------------------------------------------------------------------------------- coverage
def expected_families(key, leg):
    """Every kernel family that dense_impl can reach for the type under the leg, on the direct tile store and through
    the split-K reduction."""
    if leg == 'valu':
        return {'valu'} | ({'valu conj'} if key in 'cz' else set())
    if key == 's':
        kernel = {'default': {'KC': 1, 'CM': 2}, 'kernel1': {'KC': 1, 'CM': 1}}.get(leg, {'KC': 2, 'CM': 2})
        bk = {'kernel2_bk16': {'KC': 16, 'CM': 16}, 'kernel2_bk32': {'KC': 32, 'CM': 32}}.get(leg, {'KC': 16, 'CM': 32})
        out = {('mfma1 BN%d %s' % (bn, t)) if kernel[t] == 1 else ('mfma2 BN%d BK%d %s' % (bn, bk[t], t))
               for bn in (32, 64, 128) for t in ('KC', 'CM')}
    elif key == 'd':
        out = {'mfma16 2x%d %s' % (tv, t) for tv in ((2,) if leg == 'd_tile22' else (2, 4)) for t in ('KC', 'CM')}
    else:
        out = {'mfma16 2x2 ' + t for t in ('KC', 'CM', 'KC conj', 'CM conj')}
    return out | {f + ' split' for f in out}


GPU_LEGS = [('s', 'default'), ('s', 'kernel1'), ('s', 'kernel2'), ('s', 'kernel2_bk16'), ('s', 'kernel2_bk32'),
            ('d', 'default'), ('d', 'd_tile22'), ('d', 'valu'), ('c', 'default'), ('c', 'valu'), ('z', 'default'), ('z', 'valu')]


@pytest.mark.parametrize('cu', [4, 256, 304])
@pytest.mark.parametrize('key,leg', GPU_LEGS)
def test_every_family_is_reached_under_every_leg(key, leg, cu, monkeypatch):
    """The sweep and the split cases of a leg reach every family of the type, directly stored and split, with every row
    count, every vector count and every K chosen for the kernel -- and every K with every (order, transp) form."""
    for name, value in LEG_ENV[leg].items():
        monkeypatch.setenv(name, value)
    sweep = cases.pairings(key, 'aligned', cu)
    reached = {}
    for ny, nx, m, order, transp, epi in sweep + [(ny, nx, m, o, t, e) for ny, m, o, t, e, nx in cases.split_cases(key)]:
        reached.setdefault(cases.table_family(cases.route(key, ny, nx, m, order, transp, 'aligned', cu)), set()).add(epi)
    want = expected_families(key, leg)
    assert want <= set(reached), (key, leg, sorted(want - set(reached)))
    assert set(reached) <= want | {'valu', 'valu conj'}, sorted(set(reached) - want)       # (nx = 0 takes the VALU kernel)
    for family in want:
        assert reached[family] == set(cases.EPILOGUES), (key, leg, family, reached[family])
    nys, nxs, ms = cases.lists(key, 'aligned', cu)
    assert {c[0] for c in sweep} == set(nys) and {c[2] for c in sweep} == set(ms)
    assert {(c[1], c[3], c[4]) for c in sweep} == {(nx, o, t) for nx in nxs for o, t in cases.FORMS}
    # the tight and the window legs stay on the matrix cores, the unaligned ones leave them
    if leg != 'valu':
        for align in ('tight', 'window', 'window_rows', 'y_unaligned'):
            got = {cases.table_family(cases.route(key, c[0], c[1], c[2], c[3], c[4], align, cu)) for c in cases.pairings(key, align, cu)}
            assert {f for f in want if not f.endswith('split')} <= got, (key, leg, align)
    names = {cases.route(key, c[0], c[1], c[2], c[3], c[4], 'unaligned', cu) for c in cases.pairings(key, 'unaligned', cu)}
    assert names <= {'valu', 'valu conj'}
    if key != 'z':
        names = {cases.route(key, c[0], c[1], c[2], c[3], c[4], 'window_odd', cu) for c in cases.pairings(key, 'window_odd', cu)}
        assert names <= {'valu', 'valu conj'}


def test_route_names_the_kernel_and_the_split_count(monkeypatch):
    """The dispatch model at its limits: BN 32 | 64 | 128 and 2x2 | 2x4 by the vector count, one, two, three, 15 and 16
    splits, a last split of one element, the workspace cap that lowers two splits to one, the unaligned legs, MR = 64."""
    r = cases.route
    assert r('s', 129, 1025, 33, 0, 0, 'aligned', 256) == 'mfma1 BN64 KC x3'
    assert r('s', 129, 7681, 129, 0, 1, 'aligned', 256) == 'mfma2 BN128 BK32 CM x16'
    assert r('s', 129, 7680, 129, 0, 1, 'aligned', 256) == 'mfma2 BN128 BK32 CM x15'
    assert r('s', 129, 513, 5, 1, 1, 'aligned', 256) == 'mfma1 BN32 KC x2'
    assert r('s', 129, 512, 5, 1, 1, 'aligned', 256) == 'mfma1 BN32 KC x1'
    assert r('s', 129, 512, 5, 1, 1, 'unaligned', 256) == 'valu'
    assert r('s', 129, 0, 5, 1, 1, 'aligned', 256) == 'valu'
    assert r('s', 129, 64, 5, 0, 0, 'y_unaligned', 256) == 'mfma1 BN32 KC x1'
    assert r('d', 129, 64, 65, 0, 0, 'aligned', 256) == 'mfma16 2x4 KC x1'
    assert r('d', 129, 64, 64, 0, 1, 'aligned', 256) == 'mfma16 2x2 CM x1'
    assert r('z', 129, 7681, 64, 1, 1, 'aligned', 256) == 'mfma16 2x2 KC conj x16'
    assert r('c', 129, 64, 64, 0, 1, 'aligned', 256) == 'mfma16 2x2 CM conj x1'
    assert r('z', 129, 64, 64, 0, 1, 'unaligned', 256) == 'valu conj'
    assert r('z', 129, 64, 64, 0, 0, 'window_odd', 256) == 'mfma16 2x2 KC x1'
    assert r('d', 129, 64, 64, 0, 0, 'window_odd', 256) == 'valu'
    # 7681 = 15 * 512 + 1: the last float split holds one element; the double kernel's chunks of 16 k end the same way
    assert cases.split_plan(129, 7681, 129, 128, 128, 4, 32, 256) == (16, 16)
    # the workspace lowers two splits to one
    assert cases.plan('s', 1024, 600, 12352, 0, 0, 'aligned', 256) == ('mfma1 BN128 KC', 2, 1)
    assert cases.plan('d', 1024, 600, 6208, 0, 1, 'aligned', 256) == ('mfma16 2x4 CM', 2, 1)
    assert cases.plan('d', 1024, 600, 6144, 0, 1, 'aligned', 256) == ('mfma16 2x4 CM', 2, 2)
    monkeypatch.setenv('RLH_DENSE_KERNEL', '1')
    monkeypatch.setenv('RLH_DENSE_MR', '64')
    assert r('s', 129, 64, 65, 0, 1, 'aligned', 256) == 'mfma1 MR64 BN128 CM x1'
    assert r('s', 129, 64, 64, 0, 1, 'aligned', 256) == 'mfma1 BN64 CM x1'
    monkeypatch.setenv('RLH_DENSE_WG_PER_CU', '1')
    ny, m = cases.wg1_shape('s', 256)
    assert r('s', ny, 1025, m, 0, 1, 'aligned', 256) == 'mfma1 MR64 BN128 CM x1' and ny == 8187


# ---------------------------------------------------------------------------------------------------- planted faults
def _views(code, M, N, A, lda, order, transp, m, X, ldx, Y, ldy):
    ny, nx = (N, M) if transp else (M, N)
    return ny, nx, fake_lib._block(X, code, nx, m, ldx), fake_lib._block(Y, code, ny, m, ldy)


def test_harness_sees_a_planted_fault(fake, monkeypatch):
    """A skipped row, a written guard element, a written column after the window, Y accumulated into, a modified source:
    each is reported."""
    real = fake.rlh_dense_apply_r1
    state = {}

    def broken(code, M, N, A, lda, order, transp, m, X, ldx, Y, ldy, d_u, d_c):
        es = np.dtype(fake_lib._DT[code]).itemsize
        ny, nx, x, y = _views(code, M, N, A, lda, order, transp, m, X, ldx, Y, ldy)
        before = y.copy()
        rc = real(code, M, N, A, lda, order, transp, m, X, ldx, Y, ldy, d_u, d_c)
        if 'row' in state:                         # the last row is never stored
            y[:, ny - 1] = before[:, ny - 1]
        if 'accumulate' in state:
            y += np.where(np.isnan(before), 0, before)
        if 'guard' in state:                       # row ny of the last vector
            fake_lib._flat(fake_lib._addr(Y) + ((m - 1) * ldy + ny) * es, 'u1', 1)[0] ^= 1
        if 'nan' in state:                         # a NaN (a row of a ragged tile that read A's padding) stored at row ny
            fake_lib._block(Y, code, ny + 1, m, ldy)[m - 1, ny] = np.nan
        if 'column' in state:                      # the column after the window
            fake_lib._flat(fake_lib._addr(Y) + m * ldy * es, 'u1', 1)[0] ^= 1
        if 'source' in state:                      # the NaN after the first row of A (the call is made twice: no change that cancels)
            fake_lib._flat(fake_lib._addr(A) + N * es, 'u1', 1)[0] += 1
        if 'repeat' in state:                      # other bits on the second call
            state['repeat'] += 1
            y[0, 0] += state['repeat'] - 1
        return rc

    monkeypatch.setattr(fake, 'rlh_dense_apply_r1', broken)
    state['row'] = 1
    with pytest.raises(AssertionError, match='differ from the exact result'):
        cases.apply('d', 33, 5, 4, 0, 1, 'uc')
    with pytest.raises(AssertionError, match='above the bound'):
        cases.apply('c', 33, 5, 4, 1, 1, 'c', kind='gauss')
    for fault, message in (('guard', 'guard columns or padding rows of the result modified'),
                           ('nan', 'guard columns or padding rows of the result modified'),
                           ('column', 'guard columns or padding rows of the result modified'),
                           ('source', 'read-only operand modified'), ('repeat', 'a repeated call gives other bits')):
        state.clear()
        state[fault] = 1
        with pytest.raises(AssertionError, match=message):
            cases.apply('c', 33, 5, 4, 0, 0, 'uc')
    state.clear()
    cases.apply('c', 33, 5, 4, 0, 0, 'uc')


def test_harness_sees_an_accumulated_result(fake, monkeypatch):
    """Y must be overwritten: the NaN that it holds before the call comes back if the kernel adds to it."""
    real = fake.rlh_dense_apply_r1

    def broken(code, M, N, A, lda, order, transp, m, X, ldx, Y, ldy, d_u, d_c):
        ny, nx, x, y = _views(code, M, N, A, lda, order, transp, m, X, ldx, Y, ldy)
        before = y.copy()
        rc = real(code, M, N, A, lda, order, transp, m, X, ldx, Y, ldy, d_u, d_c)
        y += before
        return rc

    monkeypatch.setattr(fake, 'rlh_dense_apply_r1', broken)
    with pytest.raises(AssertionError, match='differ from the exact result'):
        cases.apply('s', 33, 5, 4)
    with pytest.raises(AssertionError, match='above the bound'):
        cases.apply('z', 33, 5, 4, kind='scaled')


def test_harness_sees_a_value_read_past_the_extent(fake, monkeypatch):
    """An operand read one element past its extent (A's line, X's column) brings a NaN into the result."""
    real = fake.rlh_dense_apply_r1

    def broken(code, M, N, A, lda, order, transp, m, X, ldx, Y, ldy, d_u, d_c):
        rc = real(code, M, N, A, lda, order, transp, m, X, ldx, Y, ldy, d_u, d_c)
        ny, nx, x, y = _views(code, M, N, A, lda, order, transp, m, X, ldx, Y, ldy)
        y[m - 1, :] += fake_lib._block(X, code, nx + 1, m, ldx)[m - 1, nx] * 0
        return rc

    monkeypatch.setattr(fake, 'rlh_dense_apply_r1', broken)
    with pytest.raises(AssertionError, match='differ from the exact result'):
        cases.apply('d', 33, 5, 4)


def test_harness_sees_an_element_outside_the_bound(fake, monkeypatch):
    """One element off by 2.5 (L + 5) u S -- beyond (L + 4) u S whatever the stand-in's own error is -- is reported."""
    real = fake.rlh_dense_apply_r1

    def broken(code, M, N, A, lda, order, transp, m, X, ldx, Y, ldy, d_u, d_c):
        rc = real(code, M, N, A, lda, order, transp, m, X, ldx, Y, ldy, d_u, d_c)
        ny, nx, x, y = _views(code, M, N, A, lda, order, transp, m, X, ldx, Y, ldy)
        a = fake_lib._block(A, code, N, M, lda)
        s = float(np.abs(a[ny - 1]) @ np.abs(x[m - 1]))
        y[m - 1, ny - 1] += (nx + 5) * 2.0 ** -53 * s * 2.5
        return rc

    monkeypatch.setattr(fake, 'rlh_dense_apply_r1', broken)
    with pytest.raises(AssertionError, match=r'\(vector 3, row 32\): error .* above the bound'):
        cases.apply('d', 33, 5, 4, kind='gauss')


def _mutated(fake, monkeypatch, mutate):
    real = fake.rlh_dense_apply_r1

    def broken(code, M, N, A, lda, order, transp, m, X, ldx, Y, ldy, d_u, d_c):
        rc = real(code, M, N, A, lda, order, transp, m, X, ldx, Y, ldy, d_u, d_c)
        ny, nx, x, y = _views(code, M, N, A, lda, order, transp, m, X, ldx, Y, ldy)
        a = fake_lib._block(A, code, N, M, lda) if order == 0 else fake_lib._block(A, code, M, N, lda).T
        op = np.conj(a).T if transp else a                                   # (ny, nx)
        c = fake_lib._flat(d_c, fake_lib._DT[code], m) if fake_lib._addr(d_c) else None
        u = (fake_lib._flat(d_u, fake_lib._DT[code], ny) if fake_lib._addr(d_u) else np.ones(ny, dtype=y.dtype)) if c is not None else None
        mutate(op, x, y, u, c)
        return rc

    monkeypatch.setattr(fake, 'rlh_dense_apply_r1', broken)


@pytest.mark.parametrize('key', KEYS)
def test_a_dropped_k_step_is_seen(fake, monkeypatch, key):
    """One 32-wide K step (the second of three) lost by the elements of one 32 x 32 tile corner: exact data differs, and
    bound data exceeds the bound -- at a shape where the norm of the whole block moves by less than 2e-4."""
    def mutate(op, x, y, u, c):
        if x.shape[1] > 64:
            y[-3:, -5:] -= x[-3:, 32:64] @ op[-5:, 32:64].T

    _mutated(fake, monkeypatch, mutate)
    with pytest.raises(AssertionError, match='differ from the exact result'):
        cases.apply(key, 129, 97, 65, 0, 0, 'uc')
    with pytest.raises(AssertionError, match='above the bound'):
        cases.apply(key, 129, 97, 65, 0, 1, 'none', kind='gauss')


@pytest.mark.parametrize('key', KEYS)
def test_swapped_vectors_of_one_tile_are_seen(fake, monkeypatch, key):
    """Vector v and v ^ 4 swapped in the last row tile (a wrong lane-to-vector map of the accumulator registers)."""
    def mutate(op, x, y, u, c):
        rows = slice(y.shape[1] // 32 * 32, None)
        if y.shape[0] >= 8:
            y[[1, 5], rows] = y[[5, 1], rows]

    _mutated(fake, monkeypatch, mutate)
    with pytest.raises(AssertionError, match='differ from the exact result'):
        cases.apply(key, 33, 17, 9, 1, 0, 'c')
    with pytest.raises(AssertionError, match='above the bound'):
        cases.apply(key, 33, 17, 9, 1, 1, 'none', kind='scaled')


@pytest.mark.parametrize('key', KEYS)
def test_a_rank_one_term_applied_once_per_split_is_seen(fake, monkeypatch, key):
    """The rank-one term subtracted by every split's tile store instead of once by the reduction."""
    def mutate(op, x, y, u, c):
        if c is not None and x.shape[1] > 512:
            y -= np.outer(c, u) * ((x.shape[1] + 511) // 512 - 1)

    _mutated(fake, monkeypatch, mutate)
    for epi in ('c', 'uc'):
        with pytest.raises(AssertionError, match='differ from the exact result'):
            cases.apply(key, 17, 1025, 8, 0, 0, epi)
        with pytest.raises(AssertionError, match='above the bound'):
            cases.apply(key, 5, 1025, 3, 0, 1, epi, kind='gauss')
    cases.apply(key, 17, 1025, 8, 0, 0, 'none')
    cases.apply(key, 17, 512, 8, 0, 0, 'uc')


def test_child_runner():
    done = cases.run_child('wg1', CU, fake=True)
    print(done.stdout[-4000:])
    assert done.returncode == 0 and 'DENSE_CHILD_OK leg wg1' in done.stdout
    done = cases.run_child('mr64', CU, fake=True)
    print(done.stdout[-4000:])
    assert done.returncode == 0 and 'DENSE_CHILD_OK leg mr64' in done.stdout
    done = cases.run_child('mr64', CU, fake=True, env_override={'RLH_DENSE_MR': '128'})
    print(done.stdout)
    assert done.returncode == 2 and 'needs RLH_DENSE_MR=64' in done.stdout
