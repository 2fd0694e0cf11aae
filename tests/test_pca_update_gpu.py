"""GPU tier: PCA update and incremental PCA through librlhip.so (fused dense products of the deflated operator,
block algebra with several hundred components) -- the cases of tests/_pca_update_cases.py, and the update /
incremental doctests of the reference (raleigh/interfaces/pca.py:108-133) at their own size."""

import numpy as np
import pytest

import _pca_update_cases as cases

pytestmark = pytest.mark.gpu


def test_update_with_tolerance(golden_dir):
    cases.update_with_tolerance(golden_dir)


def test_update_keeps_the_number_of_components(golden_dir):
    cases.update_keeps_the_number_of_components(golden_dir)


def test_incremental(golden_dir):
    cases.incremental(golden_dir)


def test_tall_batches():
    cases.tall_batches()


def test_refusals():
    cases.refusals()


def test_fewer_samples_than_features():
    cases.fewer_samples_than_features()


def test_other_norms():
    cases.other_norms()


def test_update_with_other_norms(golden_dir):
    cases.update_with_other_norms(golden_dir)


def test_more_rows_than_a_launch_indexes():
    cases.more_rows_than_a_launch_indexes()


@pytest.mark.parametrize('mode', ['1', '0'])
def test_update_eigensolver_on_the_device_and_on_the_host(monkeypatch, mode):
    """The k x k eigenproblems of an update at k ~ 900 through the vendor's eigensolver on the GPU (RLH_DEVICE_EIGH=1,
    an explicit choice) and through LAPACK on the host (the default): the same components to the tolerance of the data."""
    from raleigh_amd.interfaces import pca, pca_error
    from oracle.pca_data import generate
    monkeypatch.setenv('RLH_DEVICE_EIGH', mode)
    np.random.seed(1)
    A, sigma, u, v = generate(3000, 2000, 1000, pca=True)
    m0 = pca(np.ascontiguousarray(A[:2400]), tol=0.05)
    mean, trans, comps = pca(np.ascontiguousarray(A[2400:]), have=m0)
    assert comps.shape[0] >= 768
    cases.check_shape_of_result(A, mean, trans, comps)
    em, ef = pca_error(A, mean, trans, comps)
    assert ef < 0.055 and em < 0.03


def test_reference_doctests_incremental_and_update():
    """generate(3000, 2000, 1000): pca(A, batch_size=1000, tol=0.05) -> 'max 2-norm 2e-02, Frobenius norm 4e-02';
    pca(A[:2400], tol=0.05) then pca(A[2400:], have=...) -> '2e-02, 5e-02' for all rows (pca.py:108-133).
    The printed digits are asserted (the reference run in the build container gives 0.0223 / 0.0517 for the
    update, this path on the CPU stand-in 0.0226 / 0.0514)."""
    from raleigh_amd.interfaces import pca, pca_error
    from oracle.pca_data import generate
    np.random.seed(1)
    A, sigma, u, v = generate(3000, 2000, 1000, pca=True)
    mean, trans, comps = pca(A, batch_size=1000, tol=0.05)
    cases.check_shape_of_result(A, mean, trans, comps)
    em, ef = pca_error(A, mean, trans, comps)
    print('incremental: %d components, PCA error: max 2-norm %.0e, Frobenius norm %.0e' % (comps.shape[0], em, ef))
    assert ef <= 0.05 and '%.0e' % em == '2e-02'      # (0.044-0.046 from run to run: '4e-02' or '5e-02')
    A0, A1 = A[:2400], A[2400:]
    mean, trans, comps = pca(A0, tol=0.05)
    em, ef = pca_error(A0, mean, trans, comps)
    assert '%.0e' % ef == '5e-02' and '%.0e' % em == '2e-02'
    mean, trans, comps = pca(A1, have=(mean, trans, comps))
    cases.check_shape_of_result(A, mean, trans, comps)
    em, ef = pca_error(A, mean, trans, comps)
    print('update: %d components, PCA error: max 2-norm %.0e, Frobenius norm %.0e' % (comps.shape[0], em, ef))
    assert '%.0e' % ef == '5e-02' and '%.0e' % em == '2e-02'
