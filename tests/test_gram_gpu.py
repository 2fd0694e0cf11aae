"""GPU tier: rlh_gram / rlh_gram_multi of librlhip.so entry by entry -- the cases and bounds of tests/_gram_cases.py on
every dispatch path of gram_impl / gram_multi_impl: the switches that every call reads by monkeypatch, the ones read
once per process in one child process each (tests/_gram_child.py), row counts computed from the CU count that take
every pipelined and grid-stride loop past its prologue, stacked windows, wide windows and the workspace limit."""

import pytest

import _gram_cases as cases

pytestmark = pytest.mark.gpu

KEYS = cases.KEYS
# read by every call: the workgroup kernel for windows of 9 - 64 real columns, no quadrant panels, the non-temporal hint
PER_CALL = {
    'default': {},
    'stream0': {'RLH_GRAM_STREAM': '0'},
    'quad0': {'RLH_GRAM_QUAD': '0'},
    'stream0_quad0': {'RLH_GRAM_STREAM': '0', 'RLH_GRAM_QUAD': '0'},
    'nt1': {'RLH_GRAM_NT': '1'},
    'nt0': {'RLH_GRAM_NT': '0'},
}


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
    for name in ('STREAM', 'QUAD', 'NT', 'PIPE', 'ROWS', 'ZDMA', 'WG_PER_CU'):
        monkeypatch.delenv('RLH_GRAM_' + name, raising=False)
    for name, value in PER_CALL[leg].items():
        monkeypatch.setenv(name, value)


def report():
    print(cases.ratios_text())


@pytest.mark.parametrize('leg', list(PER_CALL))
@pytest.mark.parametrize('key', KEYS)
def test_short_rows(monkeypatch, cu, key, leg):
    set_leg(monkeypatch, leg)
    cases.short(key, True, cu)
    report()


@pytest.mark.parametrize('key', KEYS)
def test_short_rows_unaligned(monkeypatch, cu, key):
    """(no switch changes the path of an unaligned request: the general loop of the workgroup kernel)"""
    set_leg(monkeypatch, 'default')
    cases.short(key, False, cu)
    report()


@pytest.mark.parametrize('leg', ['default', 'nt1', 'nt0'])
@pytest.mark.parametrize('key', KEYS)
def test_deep_streaming(monkeypatch, cu, key, leg):
    set_leg(monkeypatch, leg)
    cases.deep_stream(key, cu)


@pytest.mark.parametrize('key', KEYS)
def test_deep_self_gram_of_eight_columns(monkeypatch, cu, key):
    """MODE 2 as production reaches it: the two-register-set loop at the residency cap of 8 workgroups per CU."""
    set_leg(monkeypatch, 'default')
    cases.deep_pipelined(key, cu, 8, cases.mode2_widths(key))


@pytest.mark.parametrize('m', [16, 32])
def test_deep_self_gram_on_the_workgroup_kernel(monkeypatch, cu, m):
    set_leg(monkeypatch, 'stream0')
    cases.deep_pipelined('d', cu, 8, [(m, m, 'self')])


# (leg, chunk rows, mx, my, form, aligned): float64, one case per kernel
STRIDED = {
    'mode 4': ('default', 256, 3, 2, 'two', True),
    'mode 0, four tiles on a side': ('default', 64, 65, 1, 'two', True),
    'mode 0 unaligned': ('default', 64, 1, 1, 'two', False),
    'quadrant 128': ('default', 32, 65, 33, 'two', True),
    'quadrant 128 symmetric': ('default', 32, 65, 65, 'self', True),
    'mode 3': ('stream0', 128, 17, 1, 'two', True),
    'mode 0 on 9 - 64 columns': ('stream0', 64, 33, 1, 'two', True),
    'quadrant 64': ('stream0', 64, 33, 33, 'two', True),
    'quadrant 64 symmetric': ('stream0', 64, 33, 33, 'self', True),
    'mode 0 in place of the quadrants': ('stream0_quad0', 64, 33, 33, 'two', True),
}


@pytest.mark.parametrize('name', list(STRIDED))
def test_deep_grid_stride(monkeypatch, cu, name):
    leg, chunk, mx, my, form, aligned = STRIDED[name]
    set_leg(monkeypatch, leg)
    cases.deep_strided('d', cu, chunk, mx, my, form, aligned)


@pytest.mark.parametrize('aligned,leg', [(True, 'default'), (True, 'stream0'), (True, 'quad0'), (False, 'default')])
@pytest.mark.parametrize('key', KEYS)
def test_stacked_windows(monkeypatch, key, aligned, leg):
    set_leg(monkeypatch, leg)
    cases.multi_all(key, aligned)
    report()


@pytest.mark.parametrize('leg', ['default', 'stream0', 'nt1'])
@pytest.mark.parametrize('key', ['s', 'd'])
def test_shared_block(monkeypatch, cu, key, leg):
    set_leg(monkeypatch, leg)
    t = cases.TILE[key]
    for n in (3, t + 1, 8 * t + 1, 4099, t * (3 * 8 * cu + 4 * cu) + 5):
        cases.shared_block(key, n)
    cases.shared_block(key, t + 1, 'gauss')
    cases.shared_block(key, 3, 'positive')
    report()


@pytest.mark.parametrize('key', KEYS)
def test_reduction_batch(monkeypatch, key):
    set_leg(monkeypatch, 'default')
    cases.reduction_batch(key)


@pytest.mark.parametrize('leg', ['default', 'quad0'])
@pytest.mark.parametrize('mx,my,form', [(32768, 130, 'two'), (130, 32768, 'two'), (cases.SELF_FITS, cases.SELF_FITS, 'self')])
def test_wide_windows(monkeypatch, mx, my, form, leg):
    set_leg(monkeypatch, leg)
    cases.wide('d' if form == 'self' else 's', mx, my, form)


def test_workspace_refusal(monkeypatch):
    set_leg(monkeypatch, 'default')
    cases.workspace_refusal()


@pytest.mark.parametrize('key', KEYS)
def test_degenerate(monkeypatch, key):
    set_leg(monkeypatch, 'default')
    cases.degenerate(key)


def test_refusals(monkeypatch):
    set_leg(monkeypatch, 'default')
    cases.refusals()


@pytest.mark.parametrize('leg', list(cases.LEGS))
def test_once_per_process_switch(cu, leg):
    """One fresh child per leg, under its own time limit; its output is shown, its exit status asserted, and a child that
    failed or died is not started again."""
    done = cases.run_child(leg, cu, timeout=300)
    print(done.stdout[-6000:])
    assert done.returncode == 0, 'leg %s: exit status %d' % (leg, done.returncode)
    assert 'GRAM_CHILD_OK leg %s' % leg in done.stdout
