"""CPU tier: new matrix values on a row shard's kept pattern over tests/fake_shard_values.py (a NumPy stand-in for
rlh_shardvalues_* with the library's rounding, checks and messages): the cases of tests/_shard_values_cases.py, which
the GPU tier asks of the real library, and ShardedApproximateInverse(updatable=True) on a one-rank gloo group (no halos:
gloo has no send to self; real ranks are tests/test_shard_values_dist.py, the forced run the GPU tier's)."""

import numpy as np
import pytest

import fake_lib
import fake_shard_values
import _shard_values_cases as cases

torch = pytest.importorskip('torch')


@pytest.fixture(autouse=True)
def fake():
    f = fake_shard_values.install()
    yield f
    fake_lib.uninstall()


def test_stand_in_has_every_entry_point(fake):
    from raleigh_amd import _lib
    names = sorted(name for name in _lib.SIGNATURES if name.startswith('rlh_shardvalues_'))
    assert names == ['rlh_shardvalues_info', 'rlh_shardvalues_pack', 'rlh_shardvalues_refill']
    assert all(callable(getattr(fake, name, None)) for name in names)
    assert not any(name.startswith('rlh_fs') for name in names)


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


def test_loops():
    cases.loops(300)


def test_refusals_leave_the_plan_as_it_was():
    cases.refusals()


def test_pack_delivers_zero_for_a_position_out_of_range():
    cases.pack_contract()


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
    A = cases.sc.global_matrix(np.float64, cases.N_CLASS)
    off = partition(cases.N_CLASS, 1)
    before = dict(fake.calls)
    cases.class_levels(A, comm, off, works=('native', 'bf16'))
    made = {k: fake.calls.get(k, 0) - before.get(k, 0) for k in ('shardvalues_pack', 'shardvalues_refill', 'fsvalues_update')}
    # per (levels, work): two updates of T and one of U; one rank sends nothing
    assert made == dict(shardvalues_pack=0, shardvalues_refill=12, fsvalues_update=12), made
    cases.class_by_value(A, comm, off)
    cases.class_refused(A, comm, off)


def test_update_needs_the_keyword(comm):
    from raleigh_amd.algebra.hip.dist import partition
    A = cases.sc.global_matrix(np.float64, cases.N_CLASS)
    cases.class_not_updatable(A, comm, partition(cases.N_CLASS, 1))


def test_not_updatable_makes_the_calls_it_made_before(comm, fake):
    """updatable=False: the library calls of a set-up and an application are those of the object without the keyword,
    name by name and count by count; with the keyword only the builder's destruction is missing from the set-up."""
    from raleigh_amd.algebra.hip.dist import ShardedApproximateInverse, ShardedVectors, partition
    A = cases.sc.global_matrix(np.float64, cases.N_CLASS)
    off = partition(cases.N_CLASS, 1)
    x = cases.random_block(np.random.default_rng(5), 3, cases.N_CLASS, A.dtype)

    def calls_of(**kw):
        before = dict(fake.calls)
        T = ShardedApproximateInverse(A, comm, offsets=off, levels=2, drop=0.05, **kw)
        X = ShardedVectors(x, comm=comm, offsets=off)
        T.apply(X, X)
        made = {k: v - before.get(k, 0) for k, v in fake.calls.items() if v != before.get(k, 0)}
        return made, T.device_bytes()
    plain, plain_bytes = calls_of()
    explicit, explicit_bytes = calls_of(updatable=False)
    assert plain == explicit and plain_bytes == explicit_bytes
    assert not any(name.startswith('shardvalues') or name.startswith('fsvalues') for name in plain)
    kept, kept_bytes = calls_of(updatable=True)
    assert kept == plain and kept_bytes > plain_bytes
