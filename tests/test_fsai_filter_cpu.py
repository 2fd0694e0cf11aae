"""CPU tier: post-filtration of the approximate inverse over tests/fake_fsai.py (a NumPy stand-in for the
rlh_fsfilter_create* and rlh_fsfilter_info entry points; CPU tensors stand for device tensors): the host logic of
ApproximateInverse(drop=...), the checks and their messages, and the mathematics of the cases in
tests/_fsai_filter_cases.py, which the GPU tier runs on the real library."""

import pytest

import fake_fsai
import fake_lib
import _fsai_filter_cases as cases

torch = pytest.importorskip('torch')

NEW = ('fsfilter_create', 'fsfilter_create_device')


@pytest.fixture(autouse=True)
def fake():
    f = fake_fsai.install()
    yield f
    fake_lib.uninstall()


@pytest.fixture
def device(monkeypatch):
    fake_fsai.as_device(monkeypatch)
    return 'cpu'


def _id(v):
    return '-'.join(map(str, v)) if isinstance(v, tuple) else str(v)


def test_stand_in_has_every_entry_point(fake):
    from raleigh_amd import _lib
    names = [name for name in _lib.SIGNATURES if name.startswith(('rlh_fsai_', 'rlh_fsapply_', 'rlh_fsfilter_'))]
    assert len(names) == 19 and all(callable(getattr(fake, name, None)) for name in names), names


@pytest.mark.parametrize('drop', cases.DROPS)
@pytest.mark.parametrize('which,config', cases.PATTERN_CASES, ids=_id)
def test_pattern_and_values(which, config, drop):
    cases.pattern(which, config, drop)


@pytest.mark.parametrize('drop', cases.DROPS)
@pytest.mark.parametrize('which,config', [('profile-d', cases.LEVEL_1), ('profile-c', cases.LEVEL_1), ('banded-d', cases.LEVEL_2),
                                          ('banded-d', cases.ADAPTIVE)], ids=_id)
def test_rule_against_the_unfiltered_build(which, config, drop):
    cases.rule(which, config, drop)


def test_nothing_to_remove():
    cases.nothing_to_remove()


def test_everything_removed():
    cases.everything_removed()


@pytest.mark.parametrize('which,config', [('profile-s', cases.LEVEL_1), ('banded-d', cases.LEVEL_2), ('banded-d', cases.ADAPTIVE),
                                          ('profile-z', cases.LEVEL_1)], ids=_id)
def test_scaling_by_powers_of_two(which, config):
    cases.scaling(which, config, 0.03, exact=False)


def test_kaporin_order():
    cases.kaporin_order()


def test_bins(monkeypatch):
    cases.bins('d', monkeypatch)


@pytest.mark.parametrize('work', sorted(cases.wk.WORKS))
def test_with_a_plan(work):
    cases.with_plan(work)


def test_class_takes_every_kind_of_input(device, fake):
    cases.class_inputs(device)
    assert fake.calls.get('fsfilter_create_device', 0) >= 4 and fake.calls.get('fsfilter_create', 0) >= 2


@pytest.mark.parametrize('code', ['d', 'c'])
def test_no_drop_is_unchanged(code, device, fake):
    cases.unchanged_without_drop(code, device)
    assert all(fake.calls.get(name, 0) == 0 for name in NEW)          # drop = 0 never reaches rlh_fsfilter_create*


def test_device_memory():
    cases.device_memory()


def test_rejections_of_the_build():
    cases.rejections_raw()


def test_rejections_of_the_class(fake):
    cases.rejections_class(fake)


def test_end_to_end(device, fake):
    cases.end_to_end(device)
    assert fake.calls.get('fsfilter_create_device', 0) == 1 and fake.calls.get('fsai_create_levels_device', 0) == 1
