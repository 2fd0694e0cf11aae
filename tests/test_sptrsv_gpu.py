"""GPU tier: rlh_sptrsv_create / rlh_sptrsv_solve_chain / rlh_bdiag_solve of librlhip.so element by element -- the
cases and bounds of tests/_sptrsv_cases.py: every number of lanes per row, the sum through the LDS, second batches,
second trips over a row's pieces, the block transform against its off switch, chains against single calls, plan
eviction, raw storage forms, leading dimensions with guards, non-finite right-hand sides."""

import pytest

import _sptrsv_cases as cases

pytestmark = pytest.mark.gpu

KEYS = cases.KEYS


@pytest.fixture(scope='module', autouse=True)
def real_library():
    from raleigh_amd import _lib
    _lib.set_library(None)
    L = _lib.lib()                    # raises if the .so or the GPU is missing
    import ctypes
    assert isinstance(L, ctypes.CDLL), 'native library not loaded'
    yield L


FAMILIES = ['staircase', 'random', 'blocks', 'bidiagonal', 'ilut']


def report():
    print(cases.ratios_text())


@pytest.mark.parametrize('n', [1, 7, 8, 9, 1000])
@pytest.mark.parametrize('block', [None, '1'])
@pytest.mark.parametrize('key', KEYS)
def test_diagonal_and_empty_unit_factor(monkeypatch, key, block, n):
    cases.calls('diagonal', key, block, monkeypatch, n=n)
    report()


@pytest.mark.parametrize('block', [None, '1'])
@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('key', KEYS)
def test_every_call(monkeypatch, key, family, block):
    """Every m, chains against single calls, leading dimensions, in place, the call-time switches, the refusals."""
    cases.calls(family, key, block, monkeypatch)
    report()


@pytest.mark.parametrize('family', ['blocks', 'bidiagonal'])
@pytest.mark.parametrize('key', KEYS)
def test_every_call_with_blocks_of_sixteen(monkeypatch, key, family):
    cases.calls(family, key, '16', monkeypatch)
    report()


@pytest.mark.parametrize('block', cases.BLOCKS)
@pytest.mark.parametrize('family,n', [('bidiagonal', None), ('staircase', 200)])
@pytest.mark.parametrize('key', KEYS)
def test_more_than_512_pieces_per_row(monkeypatch, key, family, n, block):
    cases.large_m(family, key, block, monkeypatch, n=n)
    report()


@pytest.mark.parametrize('block', [None, '1'])
@pytest.mark.parametrize('key', KEYS)
def test_plan_cache_eviction(monkeypatch, key, block):
    cases.plan_cache(key, block, monkeypatch)
    report()


@pytest.mark.parametrize('block', [None, '1'])
@pytest.mark.parametrize('key', KEYS)
def test_storage_forms(monkeypatch, key, block):
    cases.storage_forms(key, block, monkeypatch)
    report()


@pytest.mark.parametrize('key', KEYS)
def test_levels(monkeypatch, key):
    cases.levels(key, monkeypatch)


@pytest.mark.parametrize('key', KEYS)
def test_empty_calls(key):
    cases.empty_operator(key)
    cases.m_zero_writes_nothing(key)


@pytest.mark.parametrize('padded', [False, True])
@pytest.mark.parametrize('key', KEYS)
def test_bdiag_solve(key, padded):
    for n in cases.BDIAG_N:
        for m in cases.BDIAG_M:
            cases.bdiag(key, n, m, padded)
    report()


def test_bdiag_refusals():
    cases.bdiag_refusals()


@pytest.mark.parametrize('key', ['s', 'd'])
def test_nonfinite_right_hand_side(monkeypatch, key):
    """(the last test of the file)"""
    cases.nonfinite(key, monkeypatch)
