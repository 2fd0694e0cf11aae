"""GPU tier: the approximate-inverse preconditioner built and applied by the library (rlh_fsai_*; cases and the
derivation of every bound in tests/_fsai_cases.py).  The short / long boundary of the set-up paths is 8 | 9 kept
entries; the loop tests size their matrices from the CU count and the launch geometry stated there."""

import pytest

import _fsai_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture
def device():
    torch = pytest.importorskip('torch')
    assert torch.cuda.is_available()
    return 'cuda'


def _cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def test_library_is_native():
    import ctypes
    from raleigh_amd import _lib
    assert isinstance(_lib.lib(), ctypes.CDLL)


@pytest.mark.parametrize('bits', [32, 64])
@pytest.mark.parametrize('code', sorted(cases.TYPES))
def test_defining_property(code, bits):
    cases.defining_property(code, bits)


@pytest.mark.parametrize('code', sorted(cases.TYPES))
def test_truncation(code):
    cases.truncation(code)


@pytest.mark.parametrize('code', sorted(cases.TYPES))
def test_upper_triangle_defines_the_operator(code):
    cases.upper_defines(code)


@pytest.mark.parametrize('code', sorted(cases.TYPES))
def test_bit_identity(code):
    cases.bit_identity(code)


def test_short_path_past_one_grid_pass():
    cases.loops_short(_cu())


def test_wave_path_past_one_grid_pass():
    cases.loops_long(_cu())


@pytest.mark.parametrize('code', sorted(cases.TYPES))
def test_application(code):
    cases.application(code)


def test_rejections_of_the_build():
    cases.rejections_raw()


def test_rejections_of_the_class(device):
    cases.rejections_class(device)


def test_cpu_tensor_takes_the_host_path():
    pytest.importorskip('torch')
    from raleigh_amd.algebra.hip.precond import ApproximateInverse
    A = cases.matrix('d')
    assert cases.same_bits(ApproximateInverse(cases.csr_tensor(A, 'cpu')).csr(), ApproximateInverse(A).csr())


def test_quality():
    cases.quality()


def test_end_to_end(device):
    cases.end_to_end(device)
