"""CPU tier: the approximate-inverse preconditioner over tests/fake_fsai.py (a NumPy stand-in for the rlh_fsai_*
entry points; CPU tensors stand for device tensors): the host logic of ApproximateInverse, the checks and their
messages, and the mathematics of the cases in tests/_fsai_cases.py, which the GPU tier runs on the real library."""

import pytest

import fake_fsai
import fake_lib
import _fsai_cases as cases

torch = pytest.importorskip('torch')


@pytest.fixture(autouse=True)
def fake():
    f = fake_fsai.install()
    yield f
    fake_lib.uninstall()


@pytest.fixture
def device(monkeypatch):
    fake_fsai.as_device(monkeypatch)
    return 'cpu'


def test_stand_in_has_every_entry_point(fake):
    from raleigh_amd import _lib
    names = [name for name in _lib.SIGNATURES if name.startswith('rlh_fs')]
    assert names and all(callable(getattr(fake, name, None)) for name in names), names


@pytest.mark.parametrize('bits', [32, 64])
@pytest.mark.parametrize('code', sorted(cases.TYPES))
def test_defining_property(code, bits):
    cases.defining_property(code, bits)


@pytest.mark.parametrize('code', ['s', 'z'])
def test_truncation(code):
    cases.truncation(code)


@pytest.mark.parametrize('code', ['d', 'c'])
def test_upper_triangle_defines_the_operator(code):
    cases.upper_defines(code)


def test_bit_identity():
    cases.bit_identity('d')


def test_loops_past_their_first_trip():
    cases.loops_long(4)


@pytest.mark.parametrize('code', sorted(cases.TYPES))
def test_application(code):
    cases.application(code)


def test_rejections_of_the_build():
    cases.rejections_raw()


def test_rejections_of_the_class(device, fake):
    cases.rejections_class(device)
    # the tensor went down the device path, the SciPy matrix down the host path
    assert fake.calls.get('fsai_create_device', 0) >= 1 and fake.calls.get('fsai_create', 0) == 1


def test_cpu_tensor_takes_the_host_path(fake):
    from raleigh_amd.algebra.hip.precond import ApproximateInverse
    A = cases.matrix('d')
    G = ApproximateInverse(cases.csr_tensor(A, 'cpu')).csr()
    assert fake.calls.get('fsai_create_device', 0) == 0 and fake.calls.get('fsai_create', 0) == 1
    assert cases.same_bits(G, ApproximateInverse(A).csr())


def test_quality():
    cases.quality()


def test_end_to_end(device):
    cases.end_to_end(device, as_tensor=False)


def test_end_to_end_on_a_tensor(device, fake):
    cases.end_to_end(device)
    assert fake.calls.get('fsai_create_device', 0) == 1 and fake.calls.get('fsai_create', 0) == 0
    assert fake.calls.get('fsai_apply', 0) > 0
