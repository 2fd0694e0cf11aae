"""CPU tier: the sparse-product cases of tests/_spmm_cases.py over tests/fake_lib.py -- the harness itself (NaN poison,
guards, repeated calls, parts, the references), the proof that NumPy / SciPy in the working precision meets every bound
that the GPU tier holds the kernels to and that every exact case is exact, and that every family of the case table is the
target of bound and exact cases.  A machine of 4 compute units is assumed for the second-trip cases."""

import numpy as np
import pytest

import fake_lib
import _spmm_cases as cases
from oracle import ops

KEYS = cases.KEYS
CU = 4


@pytest.fixture(autouse=True)
def fake(monkeypatch):
    cases.clear(monkeypatch.delenv)
    f = fake_lib.install()
    yield f
    fake_lib.uninstall()


def test_stand_in_answers_fake():
    assert cases.last_launch() == 'fake'
    assert not cases.native()


def test_bfloat16_unit_roundoff_is_2_to_minus_8():
    """A correctly rounded bfloat16 result misses 2^-9 |r|: the bound of the bfloat16 step uses 2^-8."""
    r = np.float32(1.0 + 2.0 ** -8)                   # exactly between the neighbours 1 and 1 + 2^-7
    got = ops.bf16_round(np.array([r]))[0]
    assert abs(float(got) - float(r)) == 2.0 ** -8
    assert abs(float(got) - float(r)) > 2.0 ** -9 * float(r)
    assert abs(float(got) - float(r)) <= cases.U_BF16 * float(r)


@pytest.mark.parametrize('key', KEYS)
def test_sliced(key, monkeypatch):
    cases.sell(key, monkeypatch.setenv, monkeypatch.delenv)
    print(cases.ratios_text())


@pytest.mark.parametrize('key', ['s', 'd'])
def test_windowed(key, monkeypatch):
    cases.well(key, monkeypatch.setenv, monkeypatch.delenv)
    cases.well_halo(key, monkeypatch.setenv, monkeypatch.delenv)
    print(cases.ratios_text())


@pytest.mark.parametrize('key', ['s', 'd'])
def test_windowed_group_counts(key, monkeypatch):
    cases.well_windows(key, monkeypatch.setenv, monkeypatch.delenv)


@pytest.mark.parametrize('key', KEYS)
def test_interleaved(key, monkeypatch):
    cases.wide(key, monkeypatch.setenv, monkeypatch.delenv)
    cases.wide_halo(key, monkeypatch.setenv, monkeypatch.delenv)
    cases.wide_windows(key, monkeypatch.setenv, monkeypatch.delenv)
    if key in 'sd':
        cases.wide_pairs(key, monkeypatch.setenv, monkeypatch.delenv)
    print(cases.ratios_text())


@pytest.mark.parametrize('key', KEYS)
def test_stacks(key, monkeypatch):
    cases.stacks(key, monkeypatch.setenv, monkeypatch.delenv, grids=((16, 16, 12),))
    if key != 'z':
        cases.stacks_dictionaries(key, monkeypatch.setenv, monkeypatch.delenv)
    cases.stacks_halo(key, monkeypatch.setenv, monkeypatch.delenv)
    cases.stacks_overhang(key, monkeypatch.setenv, monkeypatch.delenv)
    if key != 's':
        cases.stacks_recut(key, monkeypatch.setenv, monkeypatch.delenv)
    print(cases.ratios_text())


def test_bfloat16_step(monkeypatch):
    cases.bf16_step(monkeypatch.setenv, monkeypatch.delenv)
    print(cases.ratios_text())


@pytest.mark.parametrize('family', ['sell', 'well', 'wide', 'stack'])
def test_second_trip(family, monkeypatch):
    cases.second_trip('d', family, CU, monkeypatch.setenv, monkeypatch.delenv)


@pytest.mark.parametrize('key', KEYS)
def test_gather_rows(key):
    cases.gather(key)
    if key == 's':
        cases.gather(key, bf16=True)


@pytest.mark.parametrize('key', KEYS)
def test_constructors(key, monkeypatch):
    cases.constructors(key, monkeypatch.setenv, monkeypatch.delenv, 'wide')


@pytest.mark.parametrize('key,fmt', [('s', 'sell'), ('d', 'well'), ('c', 'wide'), ('z', 'sell')])
def test_foreign_columns_and_empty_rows(key, fmt, monkeypatch):
    cases.foreign_columns(key, fmt, monkeypatch.setenv, monkeypatch.delenv)
    cases.empty_rows_pinned(key, fmt, monkeypatch.setenv, monkeypatch.delenv)
    if key in 'dz':
        cases.foreign_columns_stacks(key, monkeypatch.setenv, monkeypatch.delenv)
    if key == 's':
        cases.foreign_columns_bf16(monkeypatch.setenv, monkeypatch.delenv)


def test_harness_sees_a_wrong_element_and_a_touched_guard(fake, monkeypatch):
    """The harness fails when the library is wrong: an element written into a guard row, a dropped entry on exact data,
    and one element of a float32 product off by a relative 1e-3, which 2e-6 of the Frobenius norm lets through."""
    key = 'd'
    a = cases.ragged(key, 130, [3, 5, 1], 'exact')
    real = fake.rlh_spmm_part

    def one_element(h, part, m, X, ldx, n_own, H, ldh, Y, ldy):
        rc = real(h, part, m, X, ldx, n_own, H, ldh, Y, ldy)
        y = fake_lib._block(Y, 0, 4099, m, ldy)
        y[1, 77] *= np.float32(1.001)
        return rc
    with cases.Handle('s', cases.ragged('s', 4099, [3, 5, 1], 'graded'), 'bound') as h:
        x = cases.draw('s', 'gauss', (3, 4099), 100)
        y = (h.a.astype(np.float64) @ x.astype(np.float64).T).T
        wrong = y.copy()
        wrong[1, 77] *= 1.001
        assert np.linalg.norm(wrong - y) < 2e-6 * np.linalg.norm(y)              # (the norm check passes it)
        cases.run(h, 3, 'sell cheb=0')
        monkeypatch.setattr(fake, 'rlh_spmm_part', one_element)
        with pytest.raises(AssertionError, match='row 77.*above the bound'):
            cases.run(h, 3, 'sell cheb=0')
        monkeypatch.setattr(fake, 'rlh_spmm_part', real)

    def guard(h, part, m, X, ldx, n_own, H, ldh, Y, ldy):
        rc = real(h, part, m, X, ldx, n_own, H, ldh, Y, ldy)
        fake_lib._block(Y, 1, ldy, m, ldy)[0, 130] = 1.0          # row n_rows of the first vector
        return rc

    def dropped(h, part, m, X, ldx, n_own, H, ldh, Y, ldy):
        c = fake._csr[fake_lib._addr(h)]
        keep = c.mat.copy()
        c.mat = c.mat.tolil()
        c.mat[7, c.mat.rows[7][-1]] = 0
        c.mat = c.mat.tocsr()
        rc = real(h, part, m, X, ldx, n_own, H, ldh, Y, ldy)
        c.mat = keep
        return rc
    with cases.Handle(key, a, 'exact') as h:
        cases.run(h, 3, 'sell cheb=0')
        for broken, text in ((guard, 'guard'), (dropped, 'differ')):
            monkeypatch.setattr(fake, 'rlh_spmm_part', broken)
            with pytest.raises(AssertionError, match=text):
                cases.run(h, 3, 'sell cheb=0')
            monkeypatch.setattr(fake, 'rlh_spmm_part', real)


def test_every_family_is_the_target_of_bound_and_exact_cases(monkeypatch):
    """The table covers the whole family list (one small sweep per family here, so that the test stands alone; after the
    tests above it sees their cases as well) and no stand-in result exceeds its bound."""
    env = (monkeypatch.setenv, monkeypatch.delenv)
    cases.sell('d', *env, ns=[65])
    cases.well('s', *env, ns=[1024])
    cases.wide('c', *env, ns=[257])
    for key in 'sdz':
        cases.stacks(key, *env, grids=((16, 16, 12),))
    cases.bf16_step(*env)
    seen = {}
    for (key, family), (bound, ratio, exact) in cases.RATIOS.items():
        s = seen.setdefault(family, [0, 0, 0.0])
        s[0] += bound
        s[1] += exact
        s[2] = max(s[2], ratio)
    print(cases.ratios_text())
    for family in cases.FAMILIES:
        assert family in seen, family
        assert seen[family][0] > 0 and seen[family][1] > 0, (family, seen[family])
        assert seen[family][2] <= 1.0
