"""CPU tier: ShardedApproximateInverse(prefilter=...) over tests/fake_fsai.py, on two real ranks (gloo; the
worker is tests/_fsai_threshold_worker.py) and on one rank in this process."""

import os
import subprocess
import sys

import numpy as np
import pytest

import fake_fsai
import fake_lib
import _fsai_shard_cases as shard_cases
import _fsai_threshold_cases as cases

torch = pytest.importorskip('torch')

HERE = os.path.dirname(os.path.abspath(__file__))


def test_sharded_prefilter_on_two_ranks():
    env = dict(os.environ)
    env.pop('RANK', None)
    # (the ports of tests/test_dist_gloo.py are 29502 .. 29703, those of tests/test_fsai_shard_dist.py 29902 .. 30102)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
           '--master-addr', '127.0.0.1', '--master-port', str(30200 + (os.getpid() % 200)),
           os.path.join(HERE, '_fsai_threshold_worker.py')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'FSAI_THRESHOLD_SHARD_OK world=2' in r.stdout


@pytest.fixture
def fake():
    f = fake_fsai.install()
    yield f
    fake_lib.uninstall()


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
    A = shard_cases.global_matrix(np.float64, 500)
    cases.sharded(A, comm, partition(500, 1))
    assert fake.calls.get('fsthreshold_create', 0) >= 6 and fake.calls.get('fsfilter_create', 0) == 0
