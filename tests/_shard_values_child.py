"""Child of tests/test_shard_values_forced_gpu.py: ONE rank on nccl with forced collectives, so that the shard is cut
into two virtual ranks and the entries across the cut go rlh_shardvalues_pack -> send to self -> receive -> the
received branch of rlh_shardvalues_refill on the real library (tests/_shard_values_cases.py: the class, on a process
group).  Nothing is started after an error: the first failed assertion ends the process."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    import ctypes
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT='29591', RANK='0', WORLD_SIZE='1')
    from raleigh_amd import _lib
    L = _lib.lib()
    assert isinstance(L, ctypes.CDLL), 'native library not loaded'
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', device_id=torch.device('cuda', 0))
    import _shard_values_cases as cases
    from raleigh_amd.algebra.hip.dist import Comm, ShardedApproximateInverse, partition
    comm = Comm(force_collectives=True)
    off = partition(cases.N_CLASS, 1)
    for dt in cases.CLASS_TYPES:
        A = cases.sc.global_matrix(dt, cases.N_CLASS)
        T = ShardedApproximateInverse(A, comm, offsets=off, updatable=True)
        assert T._value_sends and T._value_sends[0][2] > 0 and T._value_recvs == [(0, T._value_sends[0][2])]   # the route across the cut
        del T
        cases.class_levels(A, comm, off, single_work='native', works=('native', 'float32'))     # (a), (d)
        cases.class_by_value(A, comm, off)                                                      # (b)
        cases.class_refused(A, comm, off)                                                       # (c)
    cases.class_not_updatable(cases.sc.global_matrix(cases.CLASS_TYPES[0], cases.N_CLASS), comm, off)
    cases.device_memory_class(comm)
    _lib.check(L.rlh_sync())
    torch.cuda.synchronize()
    dist.destroy_process_group()
    print('SHARD_VALUES_FORCED_OK')


if __name__ == '__main__':
    main()
