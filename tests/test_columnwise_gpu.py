"""GPU tier: the column-wise kernels of librlhip.so element by element against float64 / complex128 NumPy, whole
arrays compared (guard columns, padding rows, read-only operands) -- the cases and bounds of
tests/_columnwise_cases.py -- past one workgroup per column, on every alignment path, with and without the
non-temporal hint, under a capped grid that sweeps each column several times, and on blocks of more vectors than
one launch can index."""

import pytest

import _columnwise_cases as cases

pytestmark = pytest.mark.gpu

KEYS = cases.KEYS
ALIGNED = [True, False]
# The switches are read by every call: 'nt' forces the non-temporal loads and stores that otherwise start at 192 MB
# (the ALIGNED instantiations with the hint), 'plain' forbids them.
PATHS = [(aligned, leg) for leg in ('default', 'nt', 'plain') for aligned in ALIGNED]


@pytest.fixture(scope='module', autouse=True)
def real_library():
    from raleigh_amd import _lib
    _lib.set_library(None)
    L = _lib.lib()                    # raises if the .so or the GPU is missing
    import ctypes
    assert isinstance(L, ctypes.CDLL), 'native library not loaded'
    yield L


def set_leg(monkeypatch, leg):
    for name in ('RLH_STREAM_NT', 'RLH_GRAM_NT', 'RLH_ROW_BLOCKS_PER_CU'):
        monkeypatch.delenv(name, raising=False)
    if leg in ('nt', 'plain'):
        monkeypatch.setenv('RLH_STREAM_NT', '1' if leg == 'nt' else '0')
        monkeypatch.setenv('RLH_GRAM_NT', '1' if leg == 'nt' else '0')      # (the same hint in rlh_dots)
    elif leg == 'sweep':
        monkeypatch.setenv('RLH_ROW_BLOCKS_PER_CU', '1')


@pytest.mark.parametrize('aligned,leg', PATHS)
@pytest.mark.parametrize('key', KEYS)
def test_axpy_and_axpy_cols(monkeypatch, key, aligned, leg):
    set_leg(monkeypatch, leg)
    for n, m in cases.SHAPES:
        cases.axpy(key, n, m, aligned)
        cases.axpy_cols(key, n, m, aligned)


@pytest.mark.parametrize('alias', [None, 'a', 'b'])
@pytest.mark.parametrize('aligned,leg', PATHS)
@pytest.mark.parametrize('key', KEYS)
def test_lincomb(monkeypatch, key, aligned, leg, alias):
    set_leg(monkeypatch, leg)
    for n, m in cases.SHAPES:
        cases.lincomb(key, n, m, aligned, alias)


@pytest.mark.parametrize('multiply', [True, False])
@pytest.mark.parametrize('aligned,leg', PATHS)
@pytest.mark.parametrize('key', KEYS)
def test_scale(monkeypatch, key, aligned, leg, multiply):
    set_leg(monkeypatch, leg)
    for n, m in cases.SHAPES:
        cases.scale(key, n, m, aligned, multiply)


@pytest.mark.parametrize('aligned,leg', PATHS)
@pytest.mark.parametrize('key', KEYS)
def test_copy_and_copy_cols(monkeypatch, key, aligned, leg):
    set_leg(monkeypatch, leg)
    for n, m in cases.COPY_SHAPES:
        cases.copy(key, n, m, aligned)
        cases.copy_cols(key, n, m, aligned)


@pytest.mark.parametrize('aligned,leg', PATHS)
@pytest.mark.parametrize('key', KEYS)
def test_dots(monkeypatch, key, aligned, leg):
    set_leg(monkeypatch, leg)
    for n, m in cases.SHAPES:
        cases.dots(key, n, m, aligned)
        cases.dots(key, n, m, aligned, same=True)


@pytest.mark.parametrize('aligned', ALIGNED)
@pytest.mark.parametrize('key', KEYS)
def test_capped_grid_sweeps_every_column_several_times(monkeypatch, key, aligned):
    """RLH_ROW_BLOCKS_PER_CU=1 at 66001 x 17: the strided loops run several sweeps, the last one ragged."""
    set_leg(monkeypatch, 'sweep')
    n, m = cases.SWEEP_SHAPE
    cases.axpy(key, n, m, aligned)
    cases.axpy_cols(key, n, m, aligned)
    for alias in (None, 'a', 'b'):
        cases.lincomb(key, n, m, aligned, alias)
    cases.scale(key, n, m, aligned, True)
    cases.scale(key, n, m, aligned, False)
    cases.copy(key, n, m, aligned)
    cases.copy_cols(key, n, m, aligned)
    if key in 'cz':
        cases.conj(key, n, m, aligned)
    for src, dst in cases.CONVERSIONS:
        if src == key:
            cases.convert(src, dst, n, m, aligned)
    if key in 'sd':
        cases.bf16(key, n, m, aligned)


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
def test_dots_transp(key, aligned):
    for n in cases.ROWS:
        for m in (0, 1, 7):
            cases.dots_transp(key, n, m, aligned)


def test_dots_transp_capped_grid():
    """More rows than the capped grid of rlh_dots_transp has lanes: its loop runs more than once."""
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


def test_gram_keeps_its_limit():
    cases.gram_keeps_its_limit()
