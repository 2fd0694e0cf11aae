"""CPU tier: the Gram cases of tests/_gram_cases.py over tests/fake_lib.py -- the harness itself (NaN poison, guards,
the three deliveries of a result, the references), the proof that NumPy in the working precision meets every bound
that the GPU tier holds the kernels to and that every exact case is exact, and the child runner of the once-per-process
legs.  A machine of 4 compute units is assumed for the deep row counts."""

import pytest

import fake_lib
import _gram_cases as cases

KEYS = cases.KEYS
CU = 4


@pytest.fixture(autouse=True)
def fake(monkeypatch):
    for name in ('STREAM', 'QUAD', 'NT', 'PIPE', 'ROWS', 'ZDMA', 'WG_PER_CU'):
        monkeypatch.delenv('RLH_GRAM_' + name, raising=False)
    f = fake_lib.install()
    yield f
    fake_lib.uninstall()


@pytest.mark.parametrize('aligned', [True, False])
@pytest.mark.parametrize('key', KEYS)
def test_short_rows(key, aligned):
    cases.short(key, aligned, CU)
    print(cases.ratios_text())


@pytest.mark.parametrize('key', KEYS)
def test_deep_rows(key):
    cases.deep_stream(key, CU)
    cases.deep_pipelined(key, CU, 8, cases.mode2_widths(key))
    cases.deep_strided(key, CU, 4 * cases.CHUNK[key], 3, 2, 'two')
    cases.deep_strided(key, CU, cases.CHUNK[key], 1, 1, 'two', aligned=False)


@pytest.mark.parametrize('aligned', [True, False])
@pytest.mark.parametrize('key', KEYS)
def test_stacked_windows(key, aligned):
    cases.multi_all(key, aligned)


@pytest.mark.parametrize('key', ['s', 'd'])
def test_shared_block(key):
    for n in (3, cases.TILE[key] + 1, 4099):
        cases.shared_block(key, n)
    cases.shared_block(key, cases.TILE[key] + 1, 'gauss')


@pytest.mark.parametrize('key', KEYS)
def test_reduction_batch(key):
    cases.reduction_batch(key)


def test_wide_windows():
    cases.wide('s', 32768, 130)
    cases.wide('s', 130, 32768)
    cases.wide('d', cases.SELF_FITS, cases.SELF_FITS, 'self')


@pytest.mark.parametrize('key', KEYS)
def test_degenerate(key):
    cases.degenerate(key)


def test_refusals():
    cases.refusals()


def test_harness_sees_a_wrong_entry(fake, monkeypatch):
    """One entry off by eight units of roundoff, a read past n, a write in front of the result: each is reported."""
    real = fake.rlh_gram
    state = {}

    def broken(code, n, mx, X, ldx, my, Y, ldy, d_out, h_out):
        rc = real(code, n + state.get('rows', 0), mx, X, ldx, my, Y, ldy, d_out, h_out)
        for out in (d_out, h_out):
            if fake_lib._addr(out):
                g = fake_lib._flat(out, fake_lib._DT[code], my * mx)
                if 'ulp' in state:
                    g[-1] = g[-1] * (1 + 2.0 ** -50)          # 8 u of float64
                if 'guard' in state and out is d_out:
                    fake_lib._flat(fake_lib._addr(out) - 8, 'u1', 1)[0] = 0
        return rc

    monkeypatch.setattr(fake, 'rlh_gram', broken)
    state['ulp'] = 1
    with pytest.raises(AssertionError, match='differ from the exact result'):
        cases.gram('d', 33, 5, 4, True, 'exact')
    with pytest.raises(AssertionError, match='above the bound'):
        cases.gram('d', 1, 5, 4, True, 'positive')
    state.clear()
    state['rows'] = 1
    with pytest.raises(AssertionError, match='differ from the exact result|above the bound'):
        cases.gram('s', 33, 5, 4, False, 'exact')
    state.clear()
    state['guard'] = 1
    with pytest.raises(AssertionError, match='in front of the result modified'):
        cases.gram('c', 33, 5, 4, True, 'exact')


def test_child_runner():
    done = cases.run_child('zdma0', CU, fake=True)
    print(done.stdout)
    assert done.returncode == 0 and 'GRAM_CHILD_OK leg zdma0' in done.stdout
    done = cases.run_child('zdma0', CU, fake=True, env_override={'RLH_GRAM_ZDMA': '1'})
    print(done.stdout)
    assert done.returncode == 2 and 'needs RLH_GRAM_ZDMA=0' in done.stdout
