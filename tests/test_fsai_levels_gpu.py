"""GPU tier: level-of-fill patterns of the approximate inverse built by the library (rlh_fsai_create_levels*; cases, the
oracle and the launch geometry the loop tests rely on in tests/_fsai_levels_cases.py, the bound of the defining
property in tests/_fsai_cases.py)."""

import pytest

import _fsai_levels_cases as cases

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


@pytest.mark.parametrize('code', sorted(cases.TYPES))
def test_level_one_is_unchanged(code):
    cases.unchanged_level_one(code)


@pytest.mark.parametrize('code', sorted(cases.TYPES))
def test_bins(code, monkeypatch):
    cases.bins(code, monkeypatch)


@pytest.mark.parametrize('lanes', [16, 32])
def test_pattern_and_bin_past_one_grid_pass(lanes):
    cases.loops(_cu(), lanes)


def test_monotone_quality():
    cases.monotone_quality()


def test_rejections_of_the_build():
    cases.rejections_raw()


def test_rejections_of_the_class():
    cases.rejections_class()


def test_class_takes_three_kinds_of_input(device):
    cases.class_inputs(device)


def test_end_to_end(device):
    cases.end_to_end(device)
