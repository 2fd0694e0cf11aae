"""CPU tier: level-of-fill patterns of the approximate inverse over tests/fake_fsai.py (a NumPy stand-in for the
rlh_fsai_* entry points; CPU tensors stand for device tensors): the host logic of ApproximateInverse(levels=...), the
checks and their messages, and the mathematics of the cases in tests/_fsai_levels_cases.py, which the GPU tier runs on
the real library."""

import pytest

import fake_fsai
import fake_lib
import _fsai_levels_cases as cases

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


def test_banded_matrix_has_every_class():
    cases.banded_classes()


@pytest.mark.parametrize('levels', [1, 2, 3, 4])
@pytest.mark.parametrize('which', ['lap3d', 'profile', 'banded'])
def test_pattern(which, levels):
    cases.pattern(which, levels)


@pytest.mark.parametrize('code', sorted(cases.TYPES))
def test_padding_equivalence(code):
    cases.padding(code)


@pytest.mark.parametrize('levels', [2, 3])
@pytest.mark.parametrize('code', sorted(cases.TYPES))
def test_defining_property(code, levels):
    cases.defining_property(code, levels)


@pytest.mark.parametrize('code', ['d', 'c'])
def test_level_one_is_unchanged(code):
    cases.unchanged_level_one(code)


def test_bins(monkeypatch):
    cases.bins('d', monkeypatch)


@pytest.mark.parametrize('lanes', [16, 32])
def test_loops_past_their_first_trip(lanes):
    cases.loops(4, lanes)


def test_monotone_quality():
    cases.monotone_quality()


def test_rejections_of_the_build():
    cases.rejections_raw()


def test_rejections_of_the_class(fake):
    cases.rejections_class(fake)


def test_class_takes_three_kinds_of_input(device, fake):
    cases.class_inputs(device)
    assert fake.calls.get('fsai_create_levels_device', 0) >= 2 and fake.calls.get('fsai_create_levels', 0) >= 1
    assert fake.calls.get('fsai_create_device', 0) == 0 and fake.calls.get('fsai_create', 0) == 0


def test_level_one_takes_the_old_entry_points(device, fake):
    from raleigh_amd.algebra.hip.precond import ApproximateInverse
    A = cases.banded('d')
    ApproximateInverse(A)
    ApproximateInverse(cases.csr_tensor(A, device), levels=1)
    assert fake.calls.get('fsai_create', 0) == 1 and fake.calls.get('fsai_create_device', 0) == 1
    assert fake.calls.get('fsai_create_levels', 0) == 0 and fake.calls.get('fsai_create_levels_device', 0) == 0


def test_end_to_end(device, fake):
    its = cases.end_to_end(device)
    assert its[1] - its[2] >= 8
    assert fake.calls.get('fsai_create_levels_device', 0) == 1 and fake.calls.get('fsai_create_device', 0) == 1
