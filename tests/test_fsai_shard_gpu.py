"""GPU tier: the approximate inverse's application on row shards (rlh_fsshard_*) on the real library, one process
playing all the shards; cases and the bound in tests/_fsai_shard_cases.py."""

import pytest

import _fsai_shard_cases as cases

pytestmark = pytest.mark.gpu


def test_library_is_native():
    import ctypes
    from raleigh_amd import _lib
    assert isinstance(_lib.lib(), ctypes.CDLL)
    assert all(hasattr(_lib.lib(), name) for name in _lib.SIGNATURES if name.startswith('rlh_fsshard_'))


@pytest.mark.parametrize('code,work', cases.PAIRS)
def test_one_shard_is_the_existing_plan(code, work):
    cases.one_shard(code, work)


@pytest.mark.parametrize('code,work', cases.PAIRS)
def test_three_shards(code, work):
    cases.three_shards(code, work)


@pytest.mark.parametrize('work', sorted(cases.WORKS))
def test_halo_rows_from_two_owners(work):
    cases.two_owners(work)


@pytest.mark.parametrize('work', sorted(cases.WORKS))
def test_unreferenced_halo_rows_are_never_read(work):
    cases.unreferenced_rows(work)


@pytest.mark.parametrize('work', sorted(cases.WORKS))
def test_long_rows_with_halo_columns(work):
    cases.long_rows(work)


def test_empty_sizes():
    cases.edges_empty()


@pytest.mark.parametrize('work', sorted(cases.WORKS))
@pytest.mark.parametrize('n_own', [1, 63, 64, 65])
def test_small_shards_with_a_one_row_halo(n_own, work):
    cases.edges_small(n_own, work)


def test_refusals_of_the_library():
    cases.refusals(host_indices=False)


def test_device_memory():
    cases.device_memory()
