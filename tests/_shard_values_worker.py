"""Worker of tests/test_shard_values_dist.py: launched by torch.distributed.run with the gloo backend (CPU); installs
tests/fake_shard_values.py as the C-ABI library and checks the updates of ShardedApproximateInverse on real ranks, the
same global data on every rank (tests/_shard_values_cases.py: the class, on a process group)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    import torch.distributed as dist
    dist.init_process_group('gloo')
    import fake_shard_values
    fake = fake_shard_values.install()
    import _shard_values_cases as cases
    from raleigh_amd.algebra.hip.dist import Comm, partition
    comm = Comm()
    assert comm.size == int(os.environ['WORLD_SIZE'])
    off = partition(cases.N_CLASS, comm.size)
    for dt in cases.CLASS_TYPES:
        A = cases.sc.global_matrix(dt, cases.N_CLASS)
        before = dict(fake.calls)
        cases.class_levels(A, comm, off)                                        # (a), (d)
        packs = fake.calls.get('shardvalues_pack', 0) - before.get('shardvalues_pack', 0)
        assert (packs > 0) == (comm.rank > 0), packs                            # every rank but the first sends its lower columns
        cases.class_by_value(A, comm, off)                                      # (b)
        cases.class_refused(A, comm, off)                                       # (c)
    cases.class_not_updatable(cases.sc.global_matrix(cases.CLASS_TYPES[0], cases.N_CLASS), comm, off)
    dist.barrier()
    if comm.rank == 0:
        print('SHARD_VALUES_OK world=%d' % comm.size)
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
