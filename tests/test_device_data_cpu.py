"""CPU tier: PCA and truncated SVD of torch tensors (host logic of the interfaces and of the operators' device-tensor
constructors over tests/fake_device_data.py, where CPU tensors stand for device tensors), cases of
tests/_device_data_cases.py."""

import os
import subprocess
import sys

import numpy as np
import pytest

import fake_device_data
import fake_lib
import _device_data_cases as cases

torch = pytest.importorskip('torch')


@pytest.fixture(autouse=True)
def fake():
    f = fake_device_data.install()
    yield f
    fake_lib.uninstall()


@pytest.fixture
def device(monkeypatch):
    fake_device_data.as_device(monkeypatch)
    return 'cpu'


@pytest.mark.parametrize('name', cases.NAMES)
def test_interfaces_match(name, device):
    cases.interfaces_match(name, device)


def test_pca_have(device):
    cases.pca_have(device)


def test_rejections(device):
    cases.rejections(device)


def test_grad_and_conj(device):
    cases.grad_and_conj(device)


def test_cpu_tensor_takes_host_path(fake):
    cases.cpu_tensor_takes_host_path()
    assert fake.calls.get('spd_create_device', 0) == 0 and fake.calls.get('bytes_create_device', 0) == 0


@pytest.mark.parametrize('name', cases.NAMES)
def test_nothing_crosses_the_host_boundary(name, device, fake):
    """Creating an operator from a "device" tensor and returning the results move no block between host and device:
    the count of such transfers over a whole call is the count of the solve alone, the same as between the
    creation and the results of the host path."""
    from raleigh_amd.interfaces.lra import _as_matrix_like
    from raleigh_amd.interfaces import truncated_svd
    from raleigh_amd.algebra.hip import device_data, Vectors
    (_, T, H, dt, _), = [c for c in cases._inputs(device) if c[0] == name]
    n0 = fake.calls.get('block_transfer', 0)
    matrix, like = _as_matrix_like(T, 'hip')
    assert like is not None
    assert fake.calls.get('block_transfer', 0) == n0            # creation
    v = Vectors(np.ones((6, 5000), dtype=dt))                   # (an upload: counted)
    n1 = fake.calls.get('block_transfer', 0)
    assert n1 > n0
    out = device_data.export(v, like), device_data.export(v, like, transpose=True)
    device_data.finish()
    assert fake.calls.get('block_transfer', 0) == n1            # results
    assert np.array_equal(out[0].numpy(), np.ones((6, 5000), dtype=dt)) and out[1].shape == (5000, 6)
    kind = {'dense': 'dense_apply', 'bytes': 'bytes_apply'}.get(name, 'spd_apply')
    fake.calls.clear()
    np.random.seed(1)
    truncated_svd(T, nsv=3)
    moved = fake.calls.get('block_transfer', 0)
    assert fake.calls.get(kind, 0) > 0
    fake.calls.clear()
    np.random.seed(1)
    truncated_svd(H, nsv=3)
    # the host path uploads the data (dense: one block transfer; bytes and sparse go through their create calls) and
    # downloads u and vt: at least two transfers more
    assert fake.calls.get('block_transfer', 0) >= moved + 2


def test_operator_layouts(device):
    """hip.Matrix over a tensor: what is borrowed and what is copied, and that both read the same values."""
    from raleigh_amd.algebra.hip import Matrix
    from raleigh_amd.algebra.hip.memory import DeviceBuffer
    rng = np.random.default_rng(3)
    base = torch.from_numpy(rng.standard_normal((37, 80)).astype(np.float32))
    tall = torch.from_numpy(rng.standard_normal((64, 48)).astype(np.float32))
    for t, borrowed, order in ((base[:, :64].contiguous(), True, 'C_CONTIGUOUS'), (base[:, :64], True, 'C_CONTIGUOUS'),
                               (base[:, :61].contiguous(), False, 'C_CONTIGUOUS'), (base[:, 1:65], False, 'C_CONTIGUOUS'),
                               (tall[:, :37].T, True, 'F_CONTIGUOUS'),              # leading dimension 48: 192 bytes
                               (tall[:, :37].contiguous().T, False, 'F_CONTIGUOUS')):   # 37: 148 bytes
        if t.data_ptr() % 16:
            borrowed = False            # (the host allocator decides the alignment of a CPU tensor)
        m = Matrix(t)
        assert m.borrowed() == borrowed and m.order() == order and m.shape() == tuple(t.shape)
        assert isinstance(m.matrix_data(), DeviceBuffer) != borrowed
        ref = Matrix(np.ascontiguousarray(t.numpy()) if order[0] == 'C' else np.asfortranarray(t.numpy()))
        assert np.array_equal(m.dots(), ref.dots()) and m.absmax() == ref.absmax()
    with pytest.raises(ValueError, match='contiguous'):
        Matrix(base[:, ::2])


def test_package_imports_without_torch():
    """The package and its interfaces import, and take an ndarray's type for what it is, with torch hidden."""
    code = ("import sys; sys.modules['torch'] = None\n"
            "import numpy\n"
            "import raleigh_amd, raleigh_amd.interfaces, raleigh_amd.algebra.hip\n"
            "from raleigh_amd.algebra.hip import device_data\n"
            "assert not device_data.is_tensor(numpy.zeros((2, 2))) and not device_data.is_tensor(None)\n"
            "assert sys.modules['torch'] is None\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd=root)
    assert r.returncode == 0, r.stderr
