"""CPU tier: PCA and truncated SVD of uint8 / int8 input (host logic of ByteAMatrix / the interfaces over
tests/fake_byte_data.py), cases of tests/_byte_data_cases.py."""

import numpy as np
import pytest

import fake_byte_data
import fake_lib
import _byte_data_cases as cases


@pytest.fixture(autouse=True)
def fake():
    f = fake_byte_data.install()
    yield f
    fake_lib.uninstall()


@pytest.mark.parametrize('name', sorted(cases.IMAGES))
def test_pca_matches(name):
    cases.pca_matches(name)


@pytest.mark.parametrize('bytes_first', [False, True])
def test_pca_have(bytes_first):
    cases.pca_have(bytes_first)


def test_pca_batches():
    cases.pca_batches()


@pytest.mark.parametrize('name', sorted(cases.IMAGES))
def test_truncated_svd_matches(name):
    cases.truncated_svd_matches(name)


@pytest.mark.parametrize('shape', [None, (700, 600)])
def test_truncated_svd_norms(shape):
    cases.truncated_svd_norms(shape)


@pytest.mark.parametrize('signed', [False, True])
def test_known_values(signed):
    cases.known_values(signed)


def test_operator_surface():
    cases.operator_surface()


def test_refusals():
    cases.refusals()


def test_byte_images_generator():
    from raleigh_amd.synthetic import byte_images
    for name, (m, n, signed) in cases.IMAGES.items():
        A = cases.images(name)
        assert A.shape == (m, n) and A.dtype == (np.int8 if signed else np.uint8) and A.flags['C_CONTIGUOUS']
        assert np.array_equal(A, cases.images(name))                      # a pure function of its arguments
        lo, hi = (-128, 127) if signed else (0, 255)
        assert np.mean((A == lo) | (A == hi)) <= 1e-4                     # hardly anything is clipped
    a, b = byte_images(5000, 64, 4, seed=1), byte_images(5000, 64, 4, seed=2)
    assert not np.array_equal(a, b)


def test_byte_products_run_on_the_byte_operator(fake):
    """8-bit input reaches the byte operator: no float32 dense product is issued for it."""
    from raleigh_amd.interfaces import pca, truncated_svd
    A8 = cases.images('tall')
    truncated_svd(A8, nsv=3)
    pca(A8, npc=3)
    pca(A8, npc=3, batch_size=200)
    assert fake.calls.get('bytes_apply', 0) > 0
    assert fake.calls.get('dense_apply', 0) == 0
