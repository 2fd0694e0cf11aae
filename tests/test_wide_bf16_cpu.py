"""CPU tier of the bfloat16 Chebyshev step on operators built from tensors: the Python plumbing of the end-to-end
solve of tests/_wide_bf16_cases.py over tests/fake_device_operator.py, where CPU tensors stand for device tensors
(SparseSymmetricMatrix from a tensor -> supports_bf16 -> ChebyshevPreconditioner(storage='bf16') -> cheb_step_bf16).

The stand-in library does not model device layouts -- it takes the bfloat16 step for every float32 operator --, so
this file passes with and without the interleaved layout's kernel; the tests that need the kernel are in
tests/test_wide_bf16_gpu.py."""

import pytest

import fake_device_operator
import fake_lib
import _wide_bf16_cases as cases

torch = pytest.importorskip('torch')


@pytest.fixture(autouse=True)
def fake():
    f = fake_device_operator.install()
    yield f
    fake_lib.uninstall()


@pytest.fixture
def device(monkeypatch):
    fake_device_operator.as_device(monkeypatch)
    return 'cpu'


def test_end_to_end(device, fake, monkeypatch):
    cases.end_to_end(device, monkeypatch)
    # both float32 operators came from the tensor, and the bfloat16 steps reached the library
    assert fake.calls.get('csr_create', 0) == 0 and fake.calls.get('csr_create_upper', 0) == 0
    assert fake.calls.get('csr_create_device', 0) >= 3
    assert fake.calls.get('spmm_cheb_bf16', 0) > 10


def test_cases_are_what_the_gpu_tier_says():
    """The shapes the GPU tier relies on: (a) ends in a partial block, (b) has empty rows and one to four chunks, (d)
    qualifies for the row-pair form; the exact inputs keep every partial sum an integer below 256."""
    import numpy as np
    a, b, d = (cases.matrix(k) for k in 'abd')
    assert a.shape[0] == 7429 == 29 * 256 + 5 and np.diff(a.indptr).max() == 7
    assert b.shape[0] == 3001 and np.diff(b.indptr).min() == 0 and np.diff(b.indptr).max() == 27
    assert d.nnz >= 16 * d.shape[0]
    assert all(np.array_equal(d.indices[d.indptr[r]:d.indptr[r + 1]], d.indices[d.indptr[r + 1]:d.indptr[r + 2]])
               for r in range(0, d.shape[0], 2))
    for name in cases.NAMES:
        cases.exact_reference(name)
