"""GPU tier: new matrix values on the kept pattern of an approximate inverse, by the library (rlh_fsvalues_*; cases,
what is compared exactly and the launch geometry the loop tests rely on in tests/_fsai_values_cases.py, the bound of the
defining property in tests/_fsai_cases.py)."""

import pytest

import _fsai_values_cases as cases

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
    assert all(hasattr(_lib.lib(), name) for name in _lib.SIGNATURES if name.startswith('rlh_fsvalues_'))


@pytest.mark.parametrize('drop', cases.DROPS)
@pytest.mark.parametrize('config', cases.CONFIGS, ids=_id)
def test_same_matrix(config, drop):
    cases.same_matrix('profile-d', config, drop)


@pytest.mark.parametrize('host,bits', [(False, 32), (False, 64), (True, 64)])
@pytest.mark.parametrize('code', sorted(cases.TYPES))
def test_same_matrix_types_and_entry_points(code, host, bits):
    cases.same_matrix('profile-' + code, cases.LEVEL_1, 0, host=host, bits=bits)


@pytest.mark.parametrize('which,config', cases.LEVELS_ONLY, ids=_id)
def test_new_values_on_a_level_pattern(which, config):
    cases.levels_only(which, config)


def test_new_values_from_host_arrays():
    cases.levels_only('profile-d', cases.LEVEL_1, host=True)


@pytest.mark.parametrize('which,config,drop', cases.BY_VALUE, ids=_id)
def test_new_values_on_a_pattern_chosen_by_value(which, config, drop):
    cases.by_value(which, config, drop)


@pytest.mark.parametrize('drop', cases.DROPS)
@pytest.mark.parametrize('config', cases.CONFIGS, ids=_id)
@pytest.mark.parametrize('which', ['profile-d', 'banded-d'])
def test_scaling_by_powers_of_two(which, config, drop):
    cases.scaling(which, config, drop)


@pytest.mark.parametrize('which', ['profile-s', 'profile-z'])
def test_scaling_by_powers_of_two_types(which):
    cases.scaling(which, cases.LEVEL_1, 0.1)


@pytest.mark.parametrize('code', sorted(cases.TYPES))
def test_explicit_zeros_change_nothing(code):
    cases.padded(code)


def test_an_entry_the_new_matrix_does_not_store_is_zero():
    cases.entry_removed()


@pytest.mark.parametrize('work', sorted(cases.wk.WORKS))
def test_plans(work):
    cases.plans(work)


@pytest.mark.parametrize('host', [False, True], ids=['device', 'host'])
def test_refusals_leave_the_handle_as_it_was(host):
    cases.refusals(host)


def test_update_past_one_grid_pass_short_rows():
    cases.loops_short(_cu() * cases.BLOCKS_PER_CU * cases.ROWS_PER_BLOCK + 1, work='native')


def test_update_past_one_grid_pass_long_rows():
    cases.loops_long(_cu() * cases.BLOCKS_PER_CU + 1)


@pytest.mark.parametrize('code', sorted(cases.TYPES))
def test_bins(code, monkeypatch):
    cases.bins(code, monkeypatch)


def test_device_memory():
    def handle_bytes(n, nnz, es):                           # G and G^H: row pointers, entries, one start row per 256 merge items
        return 2 * (8 * (n + 1) + nnz * (4 + es) + 4 * ((n + nnz + 255) // 256 + 1))
    cases.device_memory(handle_bytes)


def test_class_takes_every_kind_of_input(device):
    cases.class_inputs(device)


def test_rejections_of_the_class(device):
    cases.class_rejections(device)


def test_end_to_end(device):
    cases.end_to_end(device)
