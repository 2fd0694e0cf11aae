"""Child of tests/test_fsai_shard_forced_gpu.py: ONE rank on nccl with forced collectives, so that the shard is cut
into two virtual ranks and both exchanges of ShardedApproximateInverse.apply run as sends to self on the real library
(tests/_fsai_shard_cases.py: the class, on a process group).  Nothing is started after an error: the first failed
assertion ends the process."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    import ctypes
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT='29571', RANK='0', WORLD_SIZE='1')
    from raleigh_amd import _lib
    L = _lib.lib()
    assert isinstance(L, ctypes.CDLL), 'native library not loaded'
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', device_id=torch.device('cuda', 0))
    import _fsai_shard_cases as cases
    from raleigh_amd.algebra.hip.dist import Comm, partition
    comm = Comm(force_collectives=True)
    off = partition(1000, 1)
    for dt in (np.float64, np.float32, np.complex128):
        A = cases.global_matrix(dt)
        works = ('native', 'float32') + (() if np.dtype(dt).kind == 'c' else ('bf16',))
        cases.class_level1(A, comm, off, single_work='native')                  # (a)
        cases.class_application(A, comm, off, works)                            # (c), (d): both halo counts non-zero
    cases.class_refusals(cases.global_matrix(np.float64), comm, off)
    its = cases.class_end_to_end(comm)                                          # (e)
    _lib.check(L.rlh_sync())
    torch.cuda.synchronize()
    dist.destroy_process_group()
    print('FSAI_SHARD_FORCED_OK iterations=%d' % its)


if __name__ == '__main__':
    main()
