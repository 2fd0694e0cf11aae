"""GPU tier: rlh_dense_apply / rlh_dense_apply_r1 of librlhip.so element by element -- the cases and bounds of
tests/_dense_cases.py on every kernel family that dense_impl of raleigh_amd/csrc/dense.hip reaches: the switches that
every call reads by monkeypatch, RLH_DENSE_MR=64 and RLH_DENSE_WG_PER_CU=1 (read once per process) in one child process
each (tests/_dense_child.py), shapes on the tile, wave and K-step boundaries of the five kernels, K splits pinned from one
to 16 with the workspace cap, and A as a window of a wider parent."""

import pytest

import _dense_cases as cases

pytestmark = pytest.mark.gpu

KEYS = cases.KEYS
# read by every call
PER_CALL = {
    'default': {},
    'kernel1': {'RLH_DENSE_KERNEL': '1'},
    'kernel2': {'RLH_DENSE_KERNEL': '2'},
    'kernel2_bk16': {'RLH_DENSE_KERNEL': '2', 'RLH_DENSE_BK': '16'},
    'kernel2_bk32': {'RLH_DENSE_KERNEL': '2', 'RLH_DENSE_BK': '32'},
    'd_tile22': {'RLH_DENSE_D_TILE': '22'},
    'valu': {'RLH_DENSE_VALU': '1'},
}
LEGS = [('s', 'default'), ('s', 'kernel1'), ('s', 'kernel2'), ('s', 'kernel2_bk16'), ('s', 'kernel2_bk32'),
        ('d', 'default'), ('d', 'd_tile22'), ('d', 'valu'), ('c', 'default'), ('c', 'valu'), ('z', 'default'), ('z', 'valu')]
MATRIX_CORE_LEGS = [(key, leg) for key, leg in LEGS if leg != 'valu']


@pytest.fixture(scope='module', autouse=True)
def real_library():
    from raleigh_amd import _lib
    _lib.set_library(None)
    L = _lib.lib()                    # raises if the .so or the GPU is missing
    import ctypes
    assert isinstance(L, ctypes.CDLL), 'native library not loaded'
    yield L


@pytest.fixture(scope='module')
def cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def set_leg(monkeypatch, leg):
    for name in cases.SWITCHES:
        monkeypatch.delenv('RLH_DENSE_' + name, raising=False)
    for name, value in PER_CALL[leg].items():
        monkeypatch.setenv(name, value)


def report():
    print(cases.ratios_text())


@pytest.mark.parametrize('key,leg', LEGS)
def test_aligned(monkeypatch, cu, key, leg):
    set_leg(monkeypatch, leg)
    cases.sweep(key, 'aligned', cu)
    report()


@pytest.mark.parametrize('key', KEYS)
def test_unaligned(monkeypatch, cu, key):
    """No operand 16-byte aligned: dense_valu_kernel against the reference, for float32 the only way to it."""
    set_leg(monkeypatch, 'default')
    assert cases.route(key, 65, 33, 5, 0, 0, 'unaligned', cu) == 'valu'
    cases.sweep(key, 'unaligned', cu)
    report()


@pytest.mark.parametrize('align', ['y_unaligned', 'tight'])
@pytest.mark.parametrize('key,leg', MATRIX_CORE_LEGS)
def test_alignment(monkeypatch, cu, key, leg, align):
    """Only Y unaligned (ldy odd), and lda == length with ldx == nx: both stay on the matrix cores."""
    set_leg(monkeypatch, leg)
    cases.sweep(key, align, cu)
    report()


@pytest.mark.parametrize('align', ['window', 'window_rows'])
@pytest.mark.parametrize('key,leg', MATRIX_CORE_LEGS)
def test_window_of_a_wider_parent(monkeypatch, cu, key, leg, align):
    """A is a window of lines that are wider than its rounded extent (transp = 1 on a row-major parent is the call of the
    distributed operator), and a window further down its parent."""
    set_leg(monkeypatch, leg)
    cases.sweep(key, align, cu)
    report()


@pytest.mark.parametrize('key', KEYS)
def test_window_at_an_offset_that_breaks_the_alignment(monkeypatch, cu, key):
    """j0 = 17: dense_valu_kernel for every type but complex128 (no switch of the matrix-core kernels changes that path, so
    once per type)."""
    set_leg(monkeypatch, 'default')
    assert (cases.route(key, 65, 33, 5, 0, 0, 'window_odd', cu) == 'valu') == (key != 'z')
    cases.sweep(key, 'window_odd', cu)
    report()


@pytest.mark.parametrize('key,leg', LEGS)
def test_splits(monkeypatch, cu, key, leg):
    set_leg(monkeypatch, leg)
    cases.splits(key, cu)
    report()


@pytest.mark.parametrize('key,leg', MATRIX_CORE_LEGS)
def test_splits_into_an_unaligned_result(monkeypatch, cu, key, leg):
    set_leg(monkeypatch, leg)
    cases.splits(key, cu, 'y_unaligned')
    report()


@pytest.mark.parametrize('key', ['s', 'd'])
def test_workspace_cap(monkeypatch, cu, key):
    set_leg(monkeypatch, 'default')
    why = cases.workspace_cap(key, cu)
    if why:
        pytest.skip('the workspace does not cap two splits to one here: ' + why)
    report()


@pytest.mark.parametrize('key,leg', LEGS)
def test_many_row_tiles(monkeypatch, cu, key, leg):
    set_leg(monkeypatch, leg)
    cases.many_row_tiles(key, cu)
    report()


@pytest.mark.parametrize('key', KEYS)
def test_degenerate(monkeypatch, key):
    set_leg(monkeypatch, 'default')
    cases.degenerate(key)


def test_refusals(monkeypatch):
    set_leg(monkeypatch, 'default')
    cases.refusals()


@pytest.mark.parametrize('leg', sorted(cases.LEGS))
def test_once_per_process_switch(cu, leg):
    """RLH_DENSE_MR=64 and RLH_DENSE_WG_PER_CU=1 in one fresh child each, under its own time limit; its output is shown, its
    exit status asserted, and a child that failed or died is not started again."""
    done = cases.run_child(leg, cu, timeout=300)
    print(done.stdout[-6000:])
    assert done.returncode == 0, 'leg %s: exit status %d' % (leg, done.returncode)
    assert 'DENSE_CHILD_OK leg %s' % leg in done.stdout
