"""CPU tier: the approximate inverse's own application over tests/fake_fsai.py (a NumPy stand-in for the
rlh_fsapply_* entry points with the library's rounding model): the host logic of ApproximateInverse(work=...), the
refusals and their messages, and the bounds of tests/_fsai_work_cases.py, which the GPU tier asks of the real library."""

import pytest

import fake_fsai
import fake_lib
import _fsai_work_cases as cases

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
    names = [name for name in _lib.SIGNATURES if name.startswith('rlh_fsapply_')]
    assert len(names) == 4 and all(callable(getattr(fake, name, None)) for name in names), names


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


def test_refusals_of_the_class(fake):
    cases.refusals_class(fake.calls)


def test_end_to_end(device):
    cases.end_to_end(device, as_tensor=False)


def test_end_to_end_on_a_tensor(device, fake):
    cases.end_to_end(device)
    assert fake.calls.get('fsapply_create', 0) == 3 and fake.calls.get('fsapply_run', 0) > 0
    assert fake.calls.get('fsai_apply', 0) == 0
