"""CPU tier: the block-update cases of tests/_block_update_cases.py over tests/fake_lib.py -- the harness itself (NaN
poison, guards, repeated calls, the references), the proof that NumPy in the working precision meets every bound that
the GPU tier holds the kernels to, that every exact case is exact and that the sums S stay below what the type holds
exactly, and the child runner of the once-per-process leg.  A machine of 4 compute units is assumed for the deep rows."""

import numpy as np
import pytest

import fake_lib
import _block_update_cases as cases

KEYS = cases.KEYS
CU = 4
SWITCHES = ('NT', 'STREAM', 'MFMA', 'MFMA_WG', 'RV')


@pytest.fixture(autouse=True)
def fake(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv('RLH_UPDATE_' + name, raising=False)
    f = fake_lib.install()
    yield f
    fake_lib.uninstall()


# (the stand-in takes every alignment and every switch the same way: each case function runs on all four types, the
# alignment legs and the VALU rows on two types each)
@pytest.mark.parametrize('key', KEYS)
def test_single_source(key):
    cases.single(key, 'aligned')
    print(cases.ratios_text())


@pytest.mark.parametrize('key,align', [('s', 'unaligned'), ('d', 'mixed')])
def test_single_source_valu_rows(key, align, monkeypatch):
    monkeypatch.setenv('RLH_UPDATE_STREAM', '0')
    monkeypatch.setenv('RLH_UPDATE_MFMA', '0')
    cases.single(key, align, valu=True)
    print(cases.ratios_text())


@pytest.mark.parametrize('key,align', [('s', 'mixed_x2'), ('d', 'aligned'), ('c', 'aligned'), ('z', 'mixed_x2')])
def test_two_sources(key, align):
    cases.two_sources(key, align)
    print(cases.ratios_text())


@pytest.mark.parametrize('key,align', [('s', 'aligned'), ('d', 'mixed'), ('c', 'mixed'), ('z', 'aligned')])
def test_two_results(key, align):
    cases.two_results(key, align)
    if key == 'z':
        cases.two_results_beyond_the_lds()
    print(cases.ratios_text())


@pytest.mark.parametrize('key,align', [('s', 'aligned'), ('d', 'unaligned'), ('c', 'aligned'), ('z', 'unaligned')])
def test_layouts_and_windows(key, align):
    cases.layouts_and_windows(key, align)


@pytest.mark.parametrize('key', KEYS)
def test_chunked_and_deep(key):
    cases.chunked(key, rows=(4099, 65) if key == 'd' else (65,))       # (S, asserted per case, does not grow with n)
    if key in 'cz':
        cases.deep_complex(key, CU, 2)
        cases.deep_complex(key, CU, 1)
    elif key == 'd':                       # (a million rows: once is enough for the stand-in)
        cases.nt_threshold(key)


@pytest.mark.parametrize('key', ['d', 'c'])
def test_nt_equals_default(key, monkeypatch):
    cases.nt_equals_default(key, monkeypatch.setenv, monkeypatch.delenv)


@pytest.mark.parametrize('key', KEYS)
def test_every_kernel_family(key, monkeypatch):
    cases.every_family(key, monkeypatch.setenv, monkeypatch.delenv, SWITCHES)
    print(cases.ratios_text())


@pytest.mark.parametrize('key', KEYS)
def test_degenerate(key):
    cases.degenerate(key)


def test_refusals():
    cases.refusals()


STREAM_FAMILIES = ['stream KS8', 'stream KS16', 'stream KS32']
MFMA_FAMILIES = ['mfma KS8', 'mfma KS16', 'mfma KS32']
LEG_ENV = {'default': {}, 'nt1': {'RLH_UPDATE_NT': '1'}, 'stream0': {'RLH_UPDATE_STREAM': '0'}, 'mfma0': {'RLH_UPDATE_MFMA': '0'}}


def _rows_by_family(key, requests, form, align='aligned'):
    """family named by route() -> the row counts that the leg's requests bring to it"""
    reached = {}
    for n, (ks, m) in requests:
        k1, k2 = (ks, 0) if form == 'one' else ks
        reached.setdefault(cases.route(key, n, k1, k2, m, align, form), set()).add(n)
    return reached


def _two(key, form, valu=False, align='aligned'):
    w = cases.TWO_SOURCE_WIDTHS
    if form == 'two':
        requests = [(ks, m) for i, ks in enumerate(cases.TWO_SOURCES) for m in (w[i % len(w)], w[(i + 4) % len(w)])]
    else:
        requests = [(ks, ms) for i, ms in enumerate(cases.TWO_RESULTS)
                    for ks in (cases.TWO_RESULT_SOURCES[i % 6], cases.TWO_RESULT_SOURCES[(i + 2) % 6])]
    return cases.pairings(key, requests, cases.shape_rows(key, valu), align, form)


@pytest.mark.parametrize('leg', ['default', 'nt1'])
@pytest.mark.parametrize('key', KEYS)
def test_every_row_reaches_every_matrix_core_family(key, leg, monkeypatch):
    """Every row count chosen for the streaming kernel reaches each of its KS instantiations (with the hint under
    RLH_UPDATE_NT=1), the complex rows each of the complex kernel's, through one, two sources and two results; the
    mixed leg brings the complex rows to the matrix-core kernel with unaligned results."""
    for name, value in LEG_ENV[leg].items():
        monkeypatch.setenv(name, value)
    real = key in 'sd'
    want = set(cases.COMMON_ROWS + cases.stream_rows(key)) if real else set(cases.MFMA_ROWS)
    for t in (1, 4, 5, 8, 9, 12, 13, 31, 32):
        assert not real or {t * cases.TR[key] + d for d in (-1, 0, 1)} <= want
    suffix = ' NT' if real and leg == 'nt1' else ''
    for form, requests in (('one', cases.single_cases(key)), ('two', _two(key, 'two')), ('2x2', _two(key, '2x2'))):
        reached = _rows_by_family(key, requests, form)
        for family in (STREAM_FAMILIES if real else MFMA_FAMILIES):
            assert want <= reached.get(family + suffix, set()), (key, form, family, sorted(want - reached.get(family + suffix, set())))
    if not real:
        reached = _rows_by_family(key, cases.single_cases(key, 'mixed'), 'one', 'mixed')
        for family in MFMA_FAMILIES:
            assert want <= reached[family + ' unaligned results'], (key, family)


@pytest.mark.parametrize('key,leg', [('s', 'stream0'), ('d', 'stream0'), ('c', 'mfma0'), ('z', 'mfma0'), ('c', 'default')])
def test_every_row_reaches_every_valu_family(key, leg, monkeypatch):
    """On the VALU legs every row count of VALU_ROWS -- one short of, equal to and one past 64 RV and 256 RV for
    RV = 1, 2 and 4 -- reaches every JT that the type has, at its RV; complex64 meets them on the default leg, too."""
    for name, value in LEG_ENV[leg].items():
        monkeypatch.setenv(name, value)
    for rv in (1, 2, 4):
        assert {b * rv + d for b in (64, 256) for d in (-1, 0, 1)} <= set(cases.VALU_ROWS)
    jts = {'s': [(8, 4), (16, 4), (32, 4)], 'd': [(8, 2), (16, 2), (32, 2), (64, 1)], 'c': [(8, 2), (16, 2)], 'z': [(8, 1), (16, 1)]}[key]
    reached = _rows_by_family(key, cases.single_cases(key, 'aligned', valu=leg != 'default'), 'one')
    for jt, rv in jts:
        family = 'valu JT%d RV%d' % (jt, rv)
        assert set(cases.VALU_ROWS) <= reached.get(family, set()), (key, family, sorted(set(cases.VALU_ROWS) - reached.get(family, set())))
    reached = _rows_by_family(key, cases.single_cases(key, 'unaligned', valu=True), 'one', 'unaligned')
    for jt in sorted({jt for jt, _ in jts}):
        assert set(cases.VALU_ROWS) <= reached.get('valu JT%d RV1' % jt, set()), (key, jt)


def test_route_names_every_family(monkeypatch):
    """The dispatch model at the limits that the issue of this suite names."""
    r = cases.route
    assert r('d', 100, 128, 0, 64, 'aligned', 'one') == 'stream KS32'
    assert r('d', 100, 128, 0, 65, 'aligned', 'one') == 'valu JT64 RV1'
    assert r('s', 100, 128, 0, 128, 'aligned', 'one') == 'stream KS32'
    assert r('s', 100, 128, 0, 129, 'aligned', 'one') == 'valu JT32 RV4'
    assert r('z', 100, 128, 0, 80, 'aligned', 'one') == 'mfma KS32'
    assert r('z', 100, 128, 0, 81, 'aligned', 'one') == 'valu JT16 RV1'
    assert r('c', 100, 128, 0, 160, 'aligned', 'one') == 'mfma KS32'
    assert r('c', 100, 128, 0, 161, 'aligned', 'one') == 'valu JT16 RV2'
    assert r('d', 100, 7, 1, 8, 'aligned', 'two') == 'stream KS8'
    assert r('d', 100, 3, 4, 8, 'aligned', 'two') == 'valu JT8 RV2'
    assert r('d', 100, 124, 5, 8, 'aligned', 'two') == 'valu JT8 RV2'
    assert r('d', 100, 100, 28, 8, 'aligned', 'two') == 'stream KS32'
    assert r('d', 100, 33, 0, 9, 'mixed', 'one') == 'valu JT16 RV1'
    assert r('z', 100, 33, 0, 17, 'mixed', 'one') == 'mfma KS16 unaligned results'
    assert r('z', 100, 64, 64, (64, 64), 'aligned', '2x2') == 'mfma KS32 two passes'
    assert r('z', 100, 64, 64, (96, 32), 'aligned', '2x2') == 'valu JT16 RV1'
    assert r('d', 100, 1025, 0, 9, 'aligned', 'one') == 'valu JT16 RV2 k-chunked'
    assert r('s', 1 << 21, 16, 0, 16, 'aligned', 'one', 1) == 'stream KS8 NT'
    monkeypatch.setenv('RLH_UPDATE_STREAM', '0')
    monkeypatch.setenv('RLH_UPDATE_NT', '1')
    assert r('s', 100, 16, 0, 16, 'aligned', 'one') == 'valu JT16 RV4 NT'
    assert r('s', 100, 16, 0, 16, 'unaligned', 'one') == 'valu JT16 RV1'


def test_harness_sees_a_planted_fault(fake, monkeypatch):
    """A skipped row, a written guard element, Out read under beta = 0, a modified source: each is reported."""
    real = fake.rlh_block_update
    state = {}

    def broken(code, n, k, X, ldx, m, Out, ldo, q, q_rs, q_cs, alpha, beta):
        es = np.dtype(fake_lib._DT[code]).itemsize
        if 'row' in state:                         # the last row is never computed
            rc = real(code, n - 1, k, X, ldx, m, Out, ldo, q, q_rs, q_cs, alpha, beta)
        elif 'beta' in state:                      # the accumulators start from Out whatever beta is
            rc = real(code, n, k, X, ldx, m, Out, ldo, q, q_rs, q_cs, alpha, 1)
        else:
            rc = real(code, n, k, X, ldx, m, Out, ldo, q, q_rs, q_cs, alpha, beta)
        if 'guard' in state:                       # row n of the last column
            fake_lib._flat(fake_lib._addr(Out) + ((m - 1) * ldo + n) * es, 'u1', 1)[0] ^= 1
        if 'column' in state:                      # the column after the window
            fake_lib._flat(fake_lib._addr(Out) + m * ldo * es, 'u1', 1)[0] ^= 1
        if 'source' in state:                      # (the call is made twice: a change that does not cancel)
            fake_lib._flat(fake_lib._addr(X), 'u1', 1)[0] += 1
        return rc

    monkeypatch.setattr(fake, 'rlh_block_update', broken)
    state['row'] = 1
    with pytest.raises(AssertionError, match='differ from the exact result'):
        cases.update('d', 33, (5,), (4,), 1)
    with pytest.raises(AssertionError, match='differ from the exact result'):
        cases.update('s', 33, (5,), (4,), 0, 'unaligned')
    with pytest.raises(AssertionError, match='above the bound'):
        cases.update('c', 33, (5,), (4,), 1, kind='gauss')
    state.clear()
    state['beta'] = 1
    with pytest.raises(AssertionError, match='differ from the exact result'):
        cases.update('z', 33, (5,), (4,), 0)
    with pytest.raises(AssertionError, match='above the bound'):
        cases.update('d', 33, (5,), (4,), 0, kind='scaled')
    for fault, message in (('guard', 'guard columns or padding rows of the result modified'),
                           ('column', 'guard columns or padding rows of the result modified'),
                           ('source', 'read-only operand modified')):
        state.clear()
        state[fault] = 1
        with pytest.raises(AssertionError, match=message):
            cases.update('c', 33, (5,), (4,), 1, col=3 if fault == 'column' else 1)
    state.clear()
    cases.update('c', 33, (5,), (4,), 1)


def test_harness_sees_an_element_outside_the_bound(fake, monkeypatch):
    """One element off by 2.5 (L + 5) u S -- beyond (L + 4) u S whatever the stand-in's own error is -- is reported."""
    real = fake.rlh_block_update

    def broken(code, n, k, X, ldx, m, Out, ldo, q, q_rs, q_cs, alpha, beta):
        rc = real(code, n, k, X, ldx, m, Out, ldo, q, q_rs, q_cs, alpha, beta)
        out = fake_lib._block(Out, code, n, m, ldo)
        x, qm = fake_lib._block(X, code, n, k, ldx), fake.__class__._qmat(q, np.dtype(np.float64), k, m, q_rs, q_cs)
        s = 0.3 * float(np.abs(qm[:, m - 1]) @ np.abs(x[:, n - 1]))
        out[m - 1, n - 1] += (k + 5) * 2.0 ** -53 * s * 2.5
        return rc

    monkeypatch.setattr(fake, 'rlh_block_update', broken)
    with pytest.raises(AssertionError, match=r'\(column 3, row 32\): error .* above the bound'):
        cases.update('d', 33, (5,), (4,), 0, kind='gauss')


def test_child_runner():
    done = cases.run_child('rv0', CU, fake=True, rows=[65, 129, 514, 4099])
    print(done.stdout[-4000:])
    assert done.returncode == 0 and 'UPDATE_CHILD_OK leg rv0' in done.stdout
    done = cases.run_child('rv0', CU, fake=True, env_override={'RLH_UPDATE_RV': '1'})
    print(done.stdout)
    assert done.returncode == 2 and 'needs RLH_UPDATE_RV=0' in done.stdout
