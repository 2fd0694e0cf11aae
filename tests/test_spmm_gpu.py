"""GPU tier: rlh_spmm(_part), rlh_spmm_cheb(_part), rlh_spmm_cheb_bf16(_part) and rlh_gather_rows(_bf16) of librlhip.so
element by element -- the cases and bounds of tests/_spmm_cases.py on every kernel family the dispatch of
raleigh_amd/csrc/spmm.hip reaches, each case asserting the family that rlh_spmm_last_launch reports.  One handle per matrix
and kind of data, its cases run on it; every test prints the accumulated family table."""

import pytest

import _spmm_cases as cases

pytestmark = pytest.mark.gpu

KEYS = cases.KEYS
REAL_KEYS = ['s', 'd']


@pytest.fixture(scope='module', autouse=True)
def real_library():
    from raleigh_amd import _lib
    _lib.set_library(None)
    L = _lib.lib()                    # raises if the .so or the GPU is missing
    import ctypes
    assert isinstance(L, ctypes.CDLL), 'native library not loaded'
    yield L


@pytest.fixture(autouse=True)
def switches(monkeypatch):
    cases.clear(monkeypatch.delenv)
    yield


@pytest.fixture(scope='module')
def cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def report():
    print(cases.ratios_text())


def test_the_library_says_what_it_launched(monkeypatch):
    """`none` for a call with nothing to launch, the kernel and its parameters, the grid and the schedule length else."""
    assert cases.native()
    monkeypatch.setenv('RLH_SPMM_FORMAT', 'sell')
    with cases.Handle('d', cases.ragged('d', 130, [3, 1, 2], 'exact'), 'exact') as h:
        _, rep = cases.run(h, 0, cases.sell_family('d', 0, False))
        assert rep == ['none']
        _, rep = cases.run(h, 5, cases.sell_family('d', 5, False))
        assert rep[0].startswith('sell jt=8 tt=1 tpb=1 cheb=0 grid=8 len=3'), rep


@pytest.mark.parametrize('key', KEYS)
def test_sliced(key, monkeypatch):
    cases.sell(key, monkeypatch.setenv, monkeypatch.delenv)
    report()


@pytest.mark.parametrize('key', REAL_KEYS)
def test_windowed(key, monkeypatch):
    cases.well(key, monkeypatch.setenv, monkeypatch.delenv)
    report()


@pytest.mark.parametrize('key', REAL_KEYS)
def test_windowed_halo_and_parts(key, monkeypatch):
    cases.well_halo(key, monkeypatch.setenv, monkeypatch.delenv)
    report()


@pytest.mark.parametrize('key', REAL_KEYS)
def test_windowed_group_counts(key, monkeypatch):
    cases.well_windows(key, monkeypatch.setenv, monkeypatch.delenv)
    report()


@pytest.mark.parametrize('key', KEYS)
def test_interleaved(key, monkeypatch):
    cases.wide(key, monkeypatch.setenv, monkeypatch.delenv)
    report()


@pytest.mark.parametrize('key', KEYS)
def test_interleaved_many_staged_columns(key, monkeypatch):
    cases.wide_windows(key, monkeypatch.setenv, monkeypatch.delenv)
    report()


@pytest.mark.parametrize('key', KEYS)
def test_interleaved_halo_and_parts(key, monkeypatch):
    cases.wide_halo(key, monkeypatch.setenv, monkeypatch.delenv)
    report()


@pytest.mark.parametrize('key', REAL_KEYS)
def test_interleaved_row_pairs(key, monkeypatch):
    cases.wide_pairs(key, monkeypatch.setenv, monkeypatch.delenv)
    report()


@pytest.mark.parametrize('key', KEYS)
def test_stacks(key, monkeypatch):
    cases.stacks(key, monkeypatch.setenv, monkeypatch.delenv)
    report()


@pytest.mark.parametrize('key', ['s', 'd', 'c'])
def test_stacks_dictionaries(key, monkeypatch):
    cases.stacks_dictionaries(key, monkeypatch.setenv, monkeypatch.delenv)
    report()


@pytest.mark.parametrize('key', KEYS)
def test_stacks_halo_and_parts(key, monkeypatch):
    cases.stacks_halo(key, monkeypatch.setenv, monkeypatch.delenv)
    report()


@pytest.mark.parametrize('key', KEYS)
def test_stacks_overhang_and_tight(key, monkeypatch):
    cases.stacks_overhang(key, monkeypatch.setenv, monkeypatch.delenv)
    print(cases.legs_text())
    report()


@pytest.mark.parametrize('key', ['d', 'c', 'z'])
def test_stacks_cut_plane_by_plane(key, monkeypatch):
    cases.stacks_recut(key, monkeypatch.setenv, monkeypatch.delenv)
    print(cases.legs_text())
    report()


def test_bfloat16_step(monkeypatch):
    cases.bf16_step(monkeypatch.setenv, monkeypatch.delenv)
    report()


@pytest.mark.parametrize('key,family', [('d', 'sell'), ('s', 'well'), ('z', 'wide'), ('d', 'stack'), ('s', 'stack')])
def test_second_trip_of_the_grid(key, family, cu, monkeypatch):
    cases.second_trip(key, family, cu, monkeypatch.setenv, monkeypatch.delenv)
    report()


@pytest.mark.parametrize('key', KEYS)
def test_gather_rows(key):
    cases.gather(key)
    if key == 's':
        cases.gather(key, bf16=True)


@pytest.mark.parametrize('key', KEYS)
@pytest.mark.parametrize('fmt', ['sell', 'wide'])
def test_constructors_give_the_same_bits(key, fmt, monkeypatch):
    cases.constructors(key, monkeypatch.setenv, monkeypatch.delenv, fmt)


@pytest.mark.parametrize('key,fmt', [('s', 'sell'), ('z', 'sell'), ('s', 'well'), ('d', 'well'), ('d', 'wide'), ('c', 'wide')])
def test_foreign_columns(key, fmt, monkeypatch):
    cases.foreign_columns(key, fmt, monkeypatch.setenv, monkeypatch.delenv)


@pytest.mark.parametrize('key', KEYS)
def test_foreign_columns_stacks(key, monkeypatch):
    cases.foreign_columns_stacks(key, monkeypatch.setenv, monkeypatch.delenv)


def test_foreign_columns_bfloat16_step(monkeypatch):
    cases.foreign_columns_bf16(monkeypatch.setenv, monkeypatch.delenv)


@pytest.mark.parametrize('fmt', ['sell', 'well', 'wide'])
def test_empty_rows_under_a_nonfinite_position_0_are_nan_or_zero(fmt, monkeypatch):
    """Pins today's behaviour (see "Empty rows" in _spmm_cases.py): the kernels are not changed for it."""
    cases.empty_rows_pinned('s', fmt, monkeypatch.setenv, monkeypatch.delenv)
    cases.empty_rows_pinned('d', fmt, monkeypatch.setenv, monkeypatch.delenv)
