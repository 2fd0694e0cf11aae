"""CPU tier: prefiltration of the approximate inverse's pattern over tests/fake_fsai.py (a NumPy stand-in for
the rlh_fsthreshold_create* and rlh_fsthreshold_info entry points; CPU tensors stand for device tensors): the host logic
of ApproximateInverse(prefilter=...), the checks and their messages, and the mathematics of the cases in
tests/_fsai_threshold_cases.py, which the GPU tier runs on the real library."""

import pytest

import fake_fsai
import fake_lib
import _fsai_threshold_cases as cases

torch = pytest.importorskip('torch')

NEW = ('fsthreshold_create', 'fsthreshold_create_device')


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
    names = [name for name in _lib.SIGNATURES if name.startswith('rlh_fsthreshold_')]
    assert len(names) == 3 and all(callable(getattr(fake, name, None)) for name in names), names
    others = [name for name in _lib.SIGNATURES
              if name.startswith(('rlh_fsai_', 'rlh_fsapply_', 'rlh_fsfilter_', 'rlh_fsshard_', 'rlh_fsvalues_'))]
    assert len(others) == 30 and all(callable(getattr(fake, name, None)) for name in others), others


def test_thresholds_stay_clear_of_the_ratios():
    cases.gaps()


def test_shapes_the_cases_rely_on():
    cases.cut_is_exercised()


@pytest.mark.parametrize('levels', cases.LEVELS)
@pytest.mark.parametrize('which,tau', cases.PATTERN_CASES)
def test_pattern(which, tau, levels):
    cases.pattern(which, tau, levels)


@pytest.mark.parametrize('code', sorted(cases.TYPES))
def test_values_on_the_full_block(code):
    cases.values(code)


def test_nothing_weak():
    cases.nothing_weak()


def test_everything_weak():
    cases.everything_weak()


@pytest.mark.parametrize('code', ['d', 'c'])
def test_lower_triangle_is_never_read(code):
    cases.lower_never_read(code)


def test_nan_above_the_diagonal_is_weak():
    cases.nan_above_is_weak()


@pytest.mark.parametrize('which,tau,levels', [('profile-s', 0.02, 1), ('banded-d', 0.02, 2), ('profile-z', 0.05, 3)])
def test_scaling_by_powers_of_two(which, tau, levels):
    cases.scaling(which, tau, levels, exact=False)


def test_nested_patterns():
    cases.nested()


def test_with_enrichment_steps():
    cases.with_steps()


def test_with_post_filtration():
    cases.with_drop()


def test_with_a_plan():
    cases.with_plan()


def test_bins(monkeypatch):
    cases.bins('d', monkeypatch)


def test_update_values_keeps_the_pattern():
    cases.update_values()


def test_class_takes_every_kind_of_input(device, fake):
    cases.class_inputs(device)
    assert fake.calls.get('fsthreshold_create_device', 0) >= 4 and fake.calls.get('fsthreshold_create', 0) >= 2


@pytest.mark.parametrize('code', ['d', 'c'])
def test_no_prefilter_is_unchanged(code, device, fake):
    cases.unchanged_without_prefilter(code, device)
    assert all(fake.calls.get(name, 0) == 0 for name in NEW)          # prefilter = 0 never reaches rlh_fsthreshold_create*


def test_rejections_of_the_build():
    cases.rejections_raw()


def test_rejections_of_the_class(fake):
    cases.rejections_class(fake)


def test_device_memory():
    cases.device_memory()


def test_end_to_end(device, fake):
    cases.end_to_end(device)
    assert fake.calls.get('fsthreshold_create_device', 0) == 1 and fake.calls.get('fsai_create_levels_device', 0) == 1
