"""CPU tier: new matrix values on the kept pattern of an approximate inverse over tests/fake_fsai.py (a NumPy
stand-in for the rlh_fsvalues_* entry points; CPU tensors stand for device tensors): the host logic of
ApproximateInverse.update_values, the checks, their order and messages, and the mathematics of the cases in
tests/_fsai_values_cases.py, which the GPU tier runs on the real library."""

import pytest

import fake_fsai
import fake_lib
import _fsai_values_cases as cases

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


def _id(v):
    return '-'.join(map(str, v)) if isinstance(v, tuple) else str(v)


def test_stand_in_has_every_entry_point(fake):
    from raleigh_amd import _lib
    names = [name for name in _lib.SIGNATURES if name.startswith('rlh_fsvalues_')]
    assert len(names) == 4 and all(callable(getattr(fake, name, None)) for name in names), names
    others = [name for name in _lib.SIGNATURES if name.startswith(('rlh_fsai_', 'rlh_fsapply_', 'rlh_fsfilter_', 'rlh_fsshard_'))]
    assert len(others) == 26 and all(callable(getattr(fake, name, None)) for name in others), others


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
@pytest.mark.parametrize('which,config', [('profile-s', cases.LEVEL_1), ('banded-d', cases.LEVEL_2), ('banded-d', cases.ADAPTIVE),
                                          ('profile-z', cases.SHORT_ROWS)], ids=_id)
def test_scaling_by_powers_of_two(which, config, drop):
    cases.scaling(which, config, drop, exact=False)


@pytest.mark.parametrize('code', ['d', 'c'])
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


def test_loops():
    cases.loops_short(300, work='native')
    cases.loops_long(120)


def test_bins(monkeypatch):
    cases.bins('d', monkeypatch)


def test_device_memory():
    cases.device_memory(lambda n, nnz, es: 2 * nnz * (es + 4) + 16 * (n + 1))


def test_class_takes_every_kind_of_input(device, fake):
    cases.class_inputs(device, fake)


def test_cpu_tensor_takes_the_host_path(fake):
    cases.cpu_tensor_takes_host_path(fake)


def test_rejections_of_the_class(device, fake):
    cases.class_rejections(device, fake)


def test_end_to_end(device, fake):
    cases.end_to_end(device)
    assert fake.calls.get('fsvalues_update_device', 0) == 2
