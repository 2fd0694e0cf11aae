"""GPU tier: post-filtration of the approximate inverse built by the library (rlh_fsfilter_create*; cases, the
oracle, the gap of the exact comparison and the launch geometry the loop test relies on in tests/_fsai_filter_cases.py,
the bound of the defining property in tests/_fsai_cases.py)."""

import pytest

import _fsai_filter_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture
def device():
    torch = pytest.importorskip('torch')
    assert torch.cuda.is_available()
    return 'cuda'


def _cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _id(v):
    return '-'.join(map(str, v)) if isinstance(v, tuple) else str(v)


def test_library_is_native():
    import ctypes
    from raleigh_amd import _lib
    assert isinstance(_lib.lib(), ctypes.CDLL)


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
    cases.scaling(which, config, 0.03)


def test_kaporin_order():
    cases.kaporin_order()


@pytest.mark.parametrize('code', sorted(cases.TYPES))
def test_bins(code, monkeypatch):
    cases.bins(code, monkeypatch)


def test_filter_past_one_grid_pass():
    cases.loops(_cu())


@pytest.mark.parametrize('work', sorted(cases.wk.WORKS))
def test_with_a_plan(work):
    cases.with_plan(work)


def test_class_takes_every_kind_of_input(device):
    cases.class_inputs(device)


@pytest.mark.parametrize('code', sorted(cases.TYPES))
def test_no_drop_is_unchanged(code, device):
    cases.unchanged_without_drop(code, device)


def test_device_memory():
    cases.device_memory()


def test_rejections_of_the_build():
    cases.rejections_raw()


def test_rejections_of_the_class():
    cases.rejections_class()


def test_end_to_end(device):
    cases.end_to_end(device)
