"""CPU tier: sparse eigenproblems on torch.sparse_csr tensors (host logic of SparseSymmetricMatrix and partial_hevp
over tests/fake_device_operator.py, where CPU tensors stand for device tensors), cases of
tests/_device_operator_cases.py."""

import numpy as np
import pytest

import fake_device_operator
import fake_lib
import _device_operator_cases as cases

torch = pytest.importorskip('torch')


@pytest.fixture(autouse=True)
def fake():
    f = fake_device_operator.install()
    yield f
    fake_lib.uninstall()


@pytest.fixture
def device(monkeypatch):
    fake_device_operator.as_device(monkeypatch)
    return 'cpu'


def test_apply_matches(device, monkeypatch):
    cases.apply_matches(device, monkeypatch)


def test_odd_storage(device):
    cases.odd_storage(device)


def test_tensor_on_another_gpu(monkeypatch):
    cases.other_gpu(monkeypatch)


def test_hevp_plain(device):
    cases.hevp_plain(device)


def test_hevp_chebyshev(device):
    cases.hevp_chebyshev(device)


def test_hevp_generalized(device):
    cases.hevp_generalized(device)


def test_hevp_iterative(device):
    cases.hevp_iterative(device)


def test_direct_mode(device):
    cases.direct_mode(device)


def test_rejections(device):
    cases.rejections(device)


def test_structure_must_be_symmetric(device):
    cases.structure_must_be_symmetric(device)


def test_cpu_tensor_takes_host_path(fake):
    cases.cpu_tensor()
    assert fake.calls.get('csr_create_device', 0) == 0 and fake.calls.get('csr_create_upper', 0) > 0


def test_operators_are_built_on_the_device(device, fake):
    """A and B given as "device" tensors: both operators come from rlh_csr_create_device, no host creation call is
    made, and no block crosses the host / device boundary on the way to the eigenvectors (the host path downloads
    them)."""
    import scipy.sparse as sp
    from raleigh_amd.interfaces import partial_hevp
    from raleigh_amd.algebra.hip.shift_invert import IterativeSymmetricSolver
    A = cases.lap()
    B = sp.csr_matrix(sp.identity(cases.N, dtype=np.float64, format='csr') * 2.0)
    ta, tb = cases.csr_tensor(A, device), cases.csr_tensor(B, device)
    np.random.seed(1)
    lmd, x, status = partial_hevp(ta, B=tb, T=True, which=2, tol=1e-5, verb=-1)
    assert status == 0
    assert fake.calls.get('csr_create_device', 0) == 2
    assert fake.calls.get('csr_create', 0) == 0 and fake.calls.get('csr_create_upper', 0) == 0
    moved = fake.calls.get('block_transfer', 0)
    fake.calls.clear()
    np.random.seed(1)
    partial_hevp(A, B=B, T=True, which=2, tol=1e-5, verb=-1)
    assert fake.calls.get('csr_create_device', 0) == 0 and fake.calls.get('csr_create_upper', 0) == 2
    assert fake.calls.get('block_transfer', 0) >= moved + 1
    fake.calls.clear()
    ev = cases.lap_eigenvalues(2)
    partial_hevp(ta, sigma=0.5 * (ev[0] + ev[1]), which=2, tol=1e-5, verb=-1,
                 solver=IterativeSymmetricSolver(dtype=np.float64, tol=1e-10))
    assert fake.calls.get('csr_create_device', 0) >= 1
    assert fake.calls.get('csr_create', 0) == 0 and fake.calls.get('csr_create_upper', 0) == 0
