"""CPU tier: the approximate inverse on row shards over tests/fake_fsai.py (a NumPy stand-in for the
rlh_fsshard_* entry points with the library's rounding model, checks and messages): the cases of
tests/_fsai_shard_cases.py, which the GPU tier asks of the real library, and the host logic of
ShardedApproximateInverse on a one-rank gloo group (no halos: gloo has no send to self, so the two virtual ranks of a
forced run are the GPU tier's; real ranks are tests/test_fsai_shard_dist.py)."""

import numpy as np
import pytest

import fake_fsai
import fake_lib
import _fsai_shard_cases as cases

torch = pytest.importorskip('torch')


@pytest.fixture(autouse=True)
def fake():
    f = fake_fsai.install()
    yield f
    fake_lib.uninstall()


def test_stand_in_has_every_entry_point(fake):
    from raleigh_amd import _lib
    names = [name for name in _lib.SIGNATURES if name.startswith('rlh_fsshard_')]
    assert len(names) == 7 and all(callable(getattr(fake, name, None)) for name in names), names


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
    cases.refusals(host_indices=True)


@pytest.fixture
def comm():
    """One rank on gloo."""
    import torch.distributed as dist
    from raleigh_amd.algebra.hip.dist import Comm
    store = dist.HashStore()
    dist.init_process_group('gloo', store=store, rank=0, world_size=1)
    try:
        yield Comm(force_collectives=False)
    finally:
        dist.destroy_process_group()


def test_class_on_one_rank(comm, fake):
    from raleigh_amd.algebra.hip.dist import partition
    A = cases.global_matrix(np.float64, 500)
    off = partition(500, 1)
    cases.class_refusals(A, comm, off)
    cases.class_level1(A, comm, off)
    before = dict(fake.calls)
    cases.class_application(A, comm, off, ('native', 'bf16'))
    made = {k: fake.calls.get(k, 0) - before.get(k, 0) for k in ('fsshard_first', 'fsshard_pack', 'fsshard_halo', 'fsshard_second')}
    assert made['fsshard_first'] == made['fsshard_second'] == 8 and made['fsshard_pack'] == made['fsshard_halo'] == 0, made
