"""CPU tier: adaptive patterns of the approximate inverse over tests/fake_fsai.py (a NumPy stand-in for the
rlh_fsai_* entry points; CPU tensors stand for device tensors): the host logic of ApproximateInverse(steps=...,
step_size=...), the checks and their messages, and the mathematics of the cases in tests/_fsai_adaptive_cases.py, which
the GPU tier runs on the real library."""

import pytest

import fake_fsai
import fake_lib
import _fsai_adaptive_cases as cases

torch = pytest.importorskip('torch')

NEW = ('fsai_create_adaptive', 'fsai_create_adaptive_device')
OLD = ('fsai_create', 'fsai_create_device', 'fsai_create_levels', 'fsai_create_levels_device')


@pytest.fixture(autouse=True)
def fake():
    f = fake_fsai.install()
    yield f
    fake_lib.uninstall()


@pytest.fixture
def device(monkeypatch):
    fake_fsai.as_device(monkeypatch)
    return 'cpu'


@pytest.mark.parametrize('config', cases.CONFIGS, ids=lambda c: '-'.join(map(str, c)))
@pytest.mark.parametrize('which', cases.MATRICES)
def test_pattern(which, config):
    cases.pattern(which, config)


@pytest.mark.parametrize('code', sorted(cases.TYPES))
def test_padding_equivalence(code):
    cases.padding(code)


@pytest.mark.parametrize('config', [(1, 4, 2), (2, 2, 4)], ids=lambda c: '-'.join(map(str, c)))
@pytest.mark.parametrize('code', sorted(cases.TYPES))
def test_defining_property(code, config):
    cases.defining_property(code, config)


def test_nesting():
    cases.nesting()


def test_quality():
    cases.quality()


@pytest.mark.parametrize('code', ['d', 'c'])
def test_no_steps_is_unchanged(code, device, fake):
    cases.unchanged_without_steps(code, device)
    assert all(fake.calls.get(name, 0) == 0 for name in NEW)
    assert fake.calls.get('fsai_create', 0) == 2 and fake.calls.get('fsai_create_device', 0) == 2
    assert fake.calls.get('fsai_create_levels', 0) == 1 and fake.calls.get('fsai_create_levels_device', 0) == 1


def test_bins(monkeypatch):
    cases.bins('d', monkeypatch)


def test_rejections_of_the_build():
    cases.rejections_raw()


def test_rejections_of_the_class(fake):
    cases.rejections_class(fake)


def test_class_takes_three_kinds_of_input(device, fake):
    cases.class_inputs(device)
    assert fake.calls.get('fsai_create_adaptive_device', 0) >= 2 and fake.calls.get('fsai_create_adaptive', 0) >= 1
    assert all(fake.calls.get(name, 0) == 0 for name in OLD)


def test_end_to_end(device, fake):
    cases.end_to_end(device)
    assert fake.calls.get('fsai_create_adaptive_device', 0) == 1 and fake.calls.get('fsai_create_device', 0) == 1
