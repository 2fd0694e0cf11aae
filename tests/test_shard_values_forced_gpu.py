"""GPU tier: the updates of ShardedApproximateInverse(updatable=True) on ONE GPU with the collectives forced (two virtual
ranks: the entries across the cut are packed, sent to self through RCCL and received), and the device memory of an
update, in a fresh child process: this process may already have created and destroyed a process group
(tests/test_dist_gpu.py)."""

import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def test_forced_collectives_on_one_gpu():
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK') and not k.startswith('MASTER_')}
    r = subprocess.run([sys.executable, os.path.join(HERE, '_shard_values_child.py')], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'SHARD_VALUES_FORCED_OK' in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
