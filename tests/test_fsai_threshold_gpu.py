"""GPU tier: prefiltration of the approximate inverse's pattern built by the library (rlh_fsthreshold_create*; cases, the
oracle, the gap of the exact comparison and the launch geometry the loop test relies on in tests/_fsai_threshold_cases.py,
the bound of the defining property in tests/_fsai_cases.py)."""

import pytest

import _fsai_threshold_cases as cases

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


@pytest.mark.parametrize('code', sorted(cases.TYPES))
def test_lower_triangle_is_never_read(code):
    cases.lower_never_read(code)


def test_nan_above_the_diagonal_is_weak():
    cases.nan_above_is_weak()


@pytest.mark.parametrize('which,tau,levels', [('profile-s', 0.02, 1), ('banded-d', 0.02, 2), ('profile-z', 0.05, 3)])
def test_scaling_by_powers_of_two(which, tau, levels):
    cases.scaling(which, tau, levels)


def test_nested_patterns():
    cases.nested()


def test_with_enrichment_steps():
    cases.with_steps()


def test_with_post_filtration():
    cases.with_drop()


def test_with_a_plan():
    cases.with_plan()


@pytest.mark.parametrize('code', sorted(cases.TYPES))
def test_bins(code, monkeypatch):
    cases.bins(code, monkeypatch)


def test_every_loop_past_its_first_trip():
    cases.loops(_cu())


def test_update_values_keeps_the_pattern():
    cases.update_values()


def test_class_takes_every_kind_of_input(device):
    cases.class_inputs(device)


@pytest.mark.parametrize('code', ['d', 'c'])
def test_no_prefilter_is_unchanged(code, device):
    cases.unchanged_without_prefilter(code, device)


def test_rejections_of_the_build():
    cases.rejections_raw()


def test_rejections_of_the_class():
    cases.rejections_class()


def test_device_memory():
    cases.device_memory()


def test_end_to_end(device):
    cases.end_to_end(device)
