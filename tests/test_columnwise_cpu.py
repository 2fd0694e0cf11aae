"""CPU tier: the column-wise cases of tests/_columnwise_cases.py over tests/fake_lib.py -- the harness itself, the host
logic of the classes on blocks of many short vectors, and the proof that NumPy in the working precision meets
every bound that the GPU tier holds the kernels to."""

import pytest

import fake_lib
import _columnwise_cases as cases
import _backend_cases

KEYS = cases.KEYS
ALIGNED = [True, False]


@pytest.fixture(autouse=True)
def fake():
    f = fake_lib.install()
    yield f
    fake_lib.uninstall()


@pytest.mark.parametrize('aligned', ALIGNED)
@pytest.mark.parametrize('key', KEYS)
def test_axpy_and_axpy_cols(key, aligned):
    for n, m in cases.SHAPES:
        cases.axpy(key, n, m, aligned)
        cases.axpy_cols(key, n, m, aligned)


@pytest.mark.parametrize('alias', [None, 'a', 'b'])
@pytest.mark.parametrize('aligned', ALIGNED)
@pytest.mark.parametrize('key', KEYS)
def test_lincomb(key, aligned, alias):
    for n, m in cases.SHAPES:
        cases.lincomb(key, n, m, aligned, alias)


@pytest.mark.parametrize('multiply', [True, False])
@pytest.mark.parametrize('aligned', ALIGNED)
@pytest.mark.parametrize('key', KEYS)
def test_scale(key, aligned, multiply):
    for n, m in cases.SHAPES:
        cases.scale(key, n, m, aligned, multiply)


@pytest.mark.parametrize('aligned', ALIGNED)
@pytest.mark.parametrize('key', KEYS)
def test_copy_and_copy_cols(key, aligned):
    for n, m in cases.COPY_SHAPES:
        cases.copy(key, n, m, aligned)
        cases.copy_cols(key, n, m, aligned)


@pytest.mark.parametrize('aligned', ALIGNED)
@pytest.mark.parametrize('key', ['c', 'z'])
def test_conj(key, aligned):
    for n, m in cases.SHAPES:
        cases.conj(key, n, m, aligned)


@pytest.mark.parametrize('aligned', ALIGNED)
@pytest.mark.parametrize('src,dst', cases.CONVERSIONS)
def test_convert(src, dst, aligned):
    for n, m in cases.SHAPES:
        cases.convert(src, dst, n, m, aligned)


@pytest.mark.parametrize('aligned', ALIGNED)
@pytest.mark.parametrize('key', ['s', 'd'])
def test_bf16_pack_unpack(key, aligned):
    for n, m in cases.SHAPES:
        cases.bf16(key, n, m, aligned)


@pytest.mark.parametrize('aligned', ALIGNED)
@pytest.mark.parametrize('key', KEYS)
def test_dots(key, aligned):
    for n, m in cases.SHAPES:
        cases.dots(key, n, m, aligned)
        cases.dots(key, n, m, aligned, same=True)


@pytest.mark.parametrize('aligned', ALIGNED)
@pytest.mark.parametrize('key', KEYS)
def test_dots_transp(key, aligned):
    for n in cases.ROWS:
        for m in (0, 1, 7):
            cases.dots_transp(key, n, m, aligned)


def test_dots_transp_capped_grid():
    cases.dots_transp('s', 600001, 3, True)


@pytest.mark.parametrize('aligned', ALIGNED)
@pytest.mark.parametrize('key', KEYS)
def test_absmax(key, aligned):
    for n, m in cases.SHAPES:
        cases.absmax(key, n, m, aligned)


@pytest.mark.parametrize('aligned', ALIGNED)
@pytest.mark.parametrize('key', KEYS + ['h'])
def test_gather_rows(key, aligned):
    for nidx in cases.GATHER_COUNTS:
        for m in cases.COLS:
            cases.gather_rows(key, nidx, m, aligned)


@pytest.mark.parametrize('n,m', cases.MANY_SHAPES)
@pytest.mark.parametrize('key', cases.MANY_KEYS)
def test_many_short_vectors(key, n, m):
    cases.many_vectors(key, n, m)


@pytest.mark.parametrize('key', cases.MANY_KEYS)
def test_many_rows_through_the_classes(key):
    cases.many_rows_through_the_classes(key)


def test_gram_keeps_its_limit(fake):
    cases.gram_keeps_its_limit()
    assert fake.calls.get('gram') == 3           # (refused by the stand-in's own check, as the library's)
