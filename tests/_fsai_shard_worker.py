"""Worker of tests/test_fsai_shard_dist.py: launched by torch.distributed.run with the gloo backend (CPU); installs
tests/fake_fsai.py as the C-ABI library and checks ShardedApproximateInverse on real ranks, the same global data on
every rank (tests/_fsai_shard_cases.py: the class, on a process group)."""
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
    fake_fsai.install()
    import _fsai_shard_cases as cases
    from raleigh_amd.algebra.hip.dist import Comm, partition
    comm = Comm()
    assert comm.size == int(os.environ['WORLD_SIZE'])
    off = partition(1000, comm.size)
    for dt in (np.float64, np.float32, np.complex128):
        A = cases.global_matrix(dt)
        works = ('native', 'float32') + (() if np.dtype(dt).kind == 'c' else ('bf16',))
        cases.class_level1(A, comm, off)                                        # (a)
        cases.class_rows_defined(A, comm, off, levels=2)                        # (b)
        cases.class_rows_defined(A, comm, off, steps=2, step_size=2)
        cases.class_application(A, comm, off, works)                            # (c), (d)
    cases.class_refusals(cases.global_matrix(np.float64), comm, off)
    cases.class_end_to_end(comm)                                                # (e)
    dist.barrier()
    if comm.rank == 0:
        print('FSAI_SHARD_OK world=%d' % comm.size)
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
