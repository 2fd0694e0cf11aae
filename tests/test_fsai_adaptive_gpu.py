"""GPU tier: adaptive patterns of the approximate inverse built by the library (rlh_fsai_create_adaptive*; cases, the
oracle and the launch geometry the loop test relies on in tests/_fsai_adaptive_cases.py, the bound of the defining
property in tests/_fsai_cases.py)."""

import pytest

import _fsai_adaptive_cases as cases

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


@pytest.mark.parametrize('code', sorted(cases.TYPES))
def test_no_steps_is_unchanged(code, device):
    cases.unchanged_without_steps(code, device)


@pytest.mark.parametrize('code', sorted(cases.TYPES))
def test_bins(code, monkeypatch):
    cases.bins(code, monkeypatch)


def test_enrichment_past_one_grid_pass():
    cases.loops(_cu())


def test_rejections_of_the_build():
    cases.rejections_raw()


def test_rejections_of_the_class():
    cases.rejections_class()


def test_class_takes_three_kinds_of_input(device):
    cases.class_inputs(device)


def test_end_to_end(device):
    cases.end_to_end(device)
