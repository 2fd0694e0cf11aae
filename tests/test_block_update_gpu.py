"""GPU tier: rlh_block_update / rlh_block_update2 / rlh_block_update2x2 of librlhip.so element by element -- the cases and
bounds of tests/_block_update_cases.py on every kernel family that launch_update of raleigh_amd/csrc/update.hip reaches:
the switches that every call reads by monkeypatch, RLH_UPDATE_RV=0 (read once per process) in one child process
(tests/_block_update_child.py), row counts on the tile, wave and workgroup boundaries of the three kernels, rows computed
from the CU count that take the complex kernel's grid-stride loop into a third sweep, and the non-temporal instantiation
as production sizes reach it."""

import pytest

import _block_update_cases as cases

pytestmark = pytest.mark.gpu

KEYS = cases.KEYS
SWITCHES = ('NT', 'STREAM', 'MFMA', 'MFMA_WG', 'RV')
# read by every call
PER_CALL = {
    'default': {},
    'nt1': {'RLH_UPDATE_NT': '1'},
    'stream0': {'RLH_UPDATE_STREAM': '0'},                                  # real types on the VALU kernel
    'mfma0': {'RLH_UPDATE_MFMA': '0'},                                      # complex types on the VALU kernel
    'stream0_nt1': {'RLH_UPDATE_STREAM': '0', 'RLH_UPDATE_NT': '1'},
    'mfma_wg1': {'RLH_UPDATE_MFMA_WG': '1'},                                # one resident workgroup per CU
}
# the legs that change the path of a type (the complex matrix-core kernel and one row per lane take no hint)
LEGS = [('s', 'default'), ('s', 'nt1'), ('s', 'stream0'), ('s', 'stream0_nt1'),
        ('d', 'default'), ('d', 'nt1'), ('d', 'stream0'), ('d', 'stream0_nt1'),
        ('c', 'default'), ('c', 'nt1'), ('c', 'mfma0'), ('z', 'default'), ('z', 'mfma0')]
VALU_LEGS = ('stream0', 'mfma0', 'stream0_nt1')


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
    for name in SWITCHES:
        monkeypatch.delenv('RLH_UPDATE_' + name, raising=False)
    for name, value in PER_CALL[leg].items():
        monkeypatch.setenv(name, value)


def report():
    print(cases.ratios_text())


@pytest.mark.parametrize('key,leg', LEGS)
def test_single_source(monkeypatch, key, leg):
    set_leg(monkeypatch, leg)
    cases.single(key, 'aligned', valu=leg in VALU_LEGS)
    report()


@pytest.mark.parametrize('align', ['unaligned', 'mixed'])
@pytest.mark.parametrize('key', KEYS)
def test_single_source_alignment(monkeypatch, key, align):
    """No 16-byte aligned operand: one row per lane.  Only the results unaligned: the same for the real types, the
    matrix-core kernel with unaligned stores for the complex ones."""
    set_leg(monkeypatch, 'default')
    cases.single(key, align, valu=(key in 'sd'))
    report()


@pytest.mark.parametrize('key,leg', LEGS)
def test_two_sources(monkeypatch, key, leg):
    set_leg(monkeypatch, leg)
    cases.two_sources(key, 'aligned', valu=leg in VALU_LEGS)
    report()


@pytest.mark.parametrize('align', ['unaligned', 'mixed', 'mixed_x2'])
@pytest.mark.parametrize('key', KEYS)
def test_two_sources_alignment(monkeypatch, key, align):
    set_leg(monkeypatch, 'default')
    cases.two_sources(key, align, valu=True)
    report()


@pytest.mark.parametrize('key,leg', LEGS)
def test_two_results(monkeypatch, key, leg):
    set_leg(monkeypatch, leg)
    cases.two_results(key, 'aligned', valu=leg in VALU_LEGS)
    report()


@pytest.mark.parametrize('align', ['unaligned', 'mixed'])
@pytest.mark.parametrize('key', KEYS)
def test_two_results_alignment(monkeypatch, key, align):
    set_leg(monkeypatch, 'default')
    cases.two_results(key, align, valu=True)
    report()


def test_two_results_beyond_the_lds(monkeypatch):
    set_leg(monkeypatch, 'default')
    cases.two_results_beyond_the_lds()
    report()


@pytest.mark.parametrize('align', ['aligned', 'unaligned', 'mixed'])
@pytest.mark.parametrize('key', KEYS)
def test_layouts_and_windows(monkeypatch, key, align):
    set_leg(monkeypatch, 'default')
    cases.layouts_and_windows(key, align)
    report()


@pytest.mark.parametrize('key', KEYS)
def test_layouts_and_windows_on_the_valu_kernel(monkeypatch, key):
    set_leg(monkeypatch, 'stream0' if key in 'sd' else 'mfma0')
    cases.layouts_and_windows(key, 'aligned')
    report()


@pytest.mark.parametrize('key', KEYS)
def test_chunked(monkeypatch, key):
    set_leg(monkeypatch, 'default')
    cases.chunked(key)
    report()


@pytest.mark.parametrize('leg,cap', [('default', 2), ('mfma_wg1', 1)])
@pytest.mark.parametrize('key', ['c', 'z'])
def test_deep_complex_rows(monkeypatch, cu, key, leg, cap):
    set_leg(monkeypatch, leg)
    cases.deep_complex(key, cu, cap)
    report()


@pytest.mark.parametrize('key', ['s', 'd'])
def test_non_temporal_threshold(monkeypatch, key):
    set_leg(monkeypatch, 'default')
    cases.nt_threshold(key)
    report()


@pytest.mark.parametrize('key,leg', [('s', 'default'), ('s', 'stream0'), ('d', 'default'), ('d', 'stream0'), ('c', 'mfma0')])
def test_non_temporal_hint_keeps_the_bits(monkeypatch, key, leg):
    set_leg(monkeypatch, leg)
    cases.nt_equals_default(key, monkeypatch.setenv, monkeypatch.delenv)
    report()


@pytest.mark.parametrize('key', KEYS)
def test_every_kernel_family(monkeypatch, key):
    cases.every_family(key, monkeypatch.setenv, monkeypatch.delenv, SWITCHES)
    report()


@pytest.mark.parametrize('key', KEYS)
def test_degenerate(monkeypatch, key):
    set_leg(monkeypatch, 'default')
    cases.degenerate(key)


def test_refusals(monkeypatch):
    set_leg(monkeypatch, 'default')
    cases.refusals()


def test_one_row_per_lane_on_aligned_blocks(cu):
    """RLH_UPDATE_RV=0 in one fresh child, under its own time limit; its output is shown, its exit status asserted, and a
    child that failed or died is not started again."""
    done = cases.run_child('rv0', cu, timeout=300)
    print(done.stdout[-6000:])
    assert done.returncode == 0, 'leg rv0: exit status %d' % done.returncode
    assert 'UPDATE_CHILD_OK leg rv0' in done.stdout
