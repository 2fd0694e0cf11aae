"""Worker of tests/test_fsai_threshold_dist.py: launched by torch.distributed.run with the gloo backend (CPU); installs
tests/fake_fsai.py as the C-ABI library and checks ShardedApproximateInverse(prefilter=...) on real ranks, the
same global data on every rank (tests/_fsai_threshold_cases.py: row shards)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    import torch.distributed as dist
    dist.init_process_group('gloo')
    import fake_fsai
    fake = fake_fsai.install()
    import _fsai_shard_cases as shard_cases
    import _fsai_threshold_cases as cases
    from raleigh_amd.algebra.hip.dist import Comm, partition
    comm = Comm()
    assert comm.size == int(os.environ['WORLD_SIZE'])
    off = partition(1000, comm.size)
    for dt in (np.float64, np.complex64):
        cases.sharded(shard_cases.global_matrix(dt), comm, off)
    assert fake.calls.get('fsthreshold_create', 0) > 0
    dist.barrier()
    if comm.rank == 0:
        print('FSAI_THRESHOLD_SHARD_OK world=%d' % comm.size)
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
