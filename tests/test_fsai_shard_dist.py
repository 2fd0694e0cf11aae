"""Multi-process CPU tier: ShardedApproximateInverse on real ranks (gloo, world sizes 2 and 3) over
tests/fake_fsai.py: the set-up exchanges, both halo exchanges of an application and the driver."""

import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize('world', [2, 3])
def test_sharded_approximate_inverse(world):
    env = dict(os.environ)
    env.pop('RANK', None)
    # (the ports of tests/test_dist_gloo.py are 29502 .. 29703, that of the GPU tier's child 29571)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(world),
           '--master-addr', '127.0.0.1', '--master-port', str(29500 + 400 + world + (os.getpid() % 200)),
           os.path.join(HERE, '_fsai_shard_worker.py')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'FSAI_SHARD_OK world=%d' % world in r.stdout
