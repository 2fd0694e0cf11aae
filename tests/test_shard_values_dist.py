"""Multi-process CPU tier: the updates of ShardedApproximateInverse(updatable=True) on real ranks (gloo, world sizes 2
and 3) over tests/fake_shard_values.py: the fetch of the lower rows, the two agreements, the point-to-point messages of
the packed values and the refill."""

import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize('world', [2, 3])
def test_sharded_updates(world):
    env = dict(os.environ)
    env.pop('RANK', None)
    # (the ports of the other multi-process tests lie in 29502 .. 30400, that of this tier's GPU child is 29591)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(world),
           '--master-addr', '127.0.0.1', '--master-port', str(30500 + world + (os.getpid() % 200)),
           os.path.join(HERE, '_shard_values_worker.py')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'SHARD_VALUES_OK world=%d' % world in r.stdout
