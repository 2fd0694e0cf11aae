"""GPU tier: new matrix values on a row shard's kept pattern (rlh_shardvalues_*) on the real library, one process playing
all the shards; cases in tests/_shard_values_cases.py.  The class with forced collectives and its device memory are
tests/test_shard_values_forced_gpu.py."""

import pytest

import _shard_values_cases as cases

pytestmark = pytest.mark.gpu


def _cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def test_library_is_native():
    import ctypes
    from raleigh_amd import _lib
    assert isinstance(_lib.lib(), ctypes.CDLL)
    names = [name for name in _lib.SIGNATURES if name.startswith('rlh_shardvalues_')]
    assert len(names) == 3 and all(hasattr(_lib.lib(), name) for name in names)


@pytest.mark.parametrize('code,work', cases.PAIRS)
def test_three_shards(code, work):
    cases.three_shards(code, work)


@pytest.mark.parametrize('n_own', [1, 63, 64, 65])
def test_small_shards_with_a_one_row_halo(n_own):
    for work in sorted(cases.WORKS):
        cases.small_shards(n_own, work)


@pytest.mark.parametrize('work', sorted(cases.WORKS))
def test_long_rows_refill_the_tails(work):
    cases.long_rows(work)


def test_no_own_rows():
    cases.no_rows()


def test_loops_past_their_first_trip():
    cases.loops(_cu() * cases.BLOCKS_PER_CU * cases.ROWS_PER_BLOCK + 1)


def test_refusals_leave_the_plan_as_it_was():
    cases.refusals()


def test_pack_delivers_zero_for_a_position_out_of_range():
    cases.pack_contract()
