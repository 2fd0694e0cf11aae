"""GPU tier: the approximate inverse's own two-kernel application (rlh_fsapply_*, ApproximateInverse(work=...)) on
the real library; cases and the derivation of every bound in tests/_fsai_work_cases.py."""

import pytest

import _fsai_work_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture
def device():
    torch = pytest.importorskip('torch')
    assert torch.cuda.is_available()
    return 'cuda'


def test_library_is_native():
    import ctypes
    from raleigh_amd import _lib
    assert isinstance(_lib.lib(), ctypes.CDLL)


@pytest.mark.parametrize('code,work', cases.PAIRS)
def test_application(code, work):
    cases.application(code, work)


@pytest.mark.parametrize('work', sorted(cases.WORKS))
@pytest.mark.parametrize('n', [1, 63, 64, 65, 129])
def test_small_sizes(n, work):
    cases.small_sizes(n, work)


def test_empty_sizes():
    cases.empty_sizes()


@pytest.mark.parametrize('work', sorted(cases.WORKS))
def test_long_rows_and_memory_condition(work):
    cases.long_rows(work)


@pytest.mark.parametrize('work', sorted(cases.WORKS))
def test_padding_is_never_read(work):
    cases.nan_row(work)


def test_refusals_of_the_library():
    cases.refusals_raw()


def test_refusals_of_the_class():
    cases.refusals_class()


def test_device_memory():
    cases.device_memory()


def test_end_to_end(device):
    cases.end_to_end(device)
