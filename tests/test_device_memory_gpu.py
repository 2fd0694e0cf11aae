"""GPU tier: every handle type gives its device memory back.  rlh_device_live counts the bytes and the allocations the
library holds for handles and builds (not rlh_malloc's buffers, which the blocks of these tests live in); after a create,
the uses that allocate lazily and the destroy, both counters must be exactly where they were -- and so after a create that
the device-side checks refuse, which happens when the scratch of the build is already allocated.  Cases and the raw C ABI
calls: tests/_device_memory_cases.py."""

import gc
import os
import subprocess
import sys

import numpy as np
import pytest

import _device_memory_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture
def base():
    gc.collect()
    return cases.live()


def test_counters_before_init_and_stand_in():
    """Valid before rlh_init, where nothing is held (a fresh process); the CPU tier's stand-in reports nothing held."""
    code = ('import ctypes, sys; sys.path.insert(0, %r); from raleigh_amd import _lib; L = _lib.library(); '
            'a, b = ctypes.c_int64(-1), ctypes.c_int64(-1); rc = L.rlh_device_live(ctypes.byref(a), ctypes.byref(b)); '
            'sys.exit(0 if (rc, a.value, b.value) == (0, 0, 0) else 1)' % cases.ROOT)
    assert subprocess.run([sys.executable, '-c', code]).returncode == 0


# (matrix, creates, switches, layout, stacks expected)
CSR = [('random300', ('host', 'upper', 'device'), dict(RLH_SPMM_FORMAT='sell'), 'sell', False),
       ('stencil', ('host', 'upper'), dict(RLH_SPMM_FORMAT=None, RLH_SPMM_STACK='2', RLH_SPMM_STACK_ALIGN='2'), 'well', True),
       ('small_stencil', ('host', 'upper', 'device'), dict(RLH_SPMM_FORMAT='wide'), 'wide', False),
       ('stencil_z', ('upper',), dict(RLH_SPMM_FORMAT=None, RLH_SPMM_STACK='2', RLH_SPMM_STACK_ALIGN='2'), 'wide', True)]


@pytest.mark.parametrize('name,creates,env,layout,stacked', CSR, ids=[c[0] for c in CSR])
def test_csr(base, name, creates, env, layout, stacked):
    A = cases.matrix(name)
    with cases.Env(**env):
        for how in creates:
            rc, h = cases.csr_create(A, how)
            cases.check(rc)
            got_layout, stacks, nbytes = cases.csr_facts(h)
            assert got_layout == layout and (stacks > 0) == stacked, (how, got_layout, stacks)
            held = cases.live()
            assert held[0] - base[0] >= nbytes > 0 and held[1] > base[1], (how, held, base, nbytes)
            cases.csr_use(h, A)
            if layout != 'sell':                       # (the sliced layout has no launch order to build)
                assert cases.live()[1] > held[1], how
            cases.csr_destroy(h)
            assert cases.live() == base, how


def test_csr_schedule_cache_evicts(base):
    """The interleaved layout keeps 16 launch orders; part-1 calls at 17 own / halo boundaries drop the oldest."""
    A = cases.matrix('shard')
    with cases.Env(RLH_SPMM_FORMAT='wide'):
        rc, h = cases.csr_create(A, 'host')
    cases.check(rc)
    assert cases.csr_facts(h)[0] == 'wide'
    m, ld = 4, 1024 + 8
    x, y = cases.block(m, ld, A.dtype), cases.block(m, 512, A.dtype, 4)
    start = cases.live()[1]
    blocks = []
    for k in range(17):
        n_own = 512 + 8 * k
        cases.check(cases.L().rlh_spmm_part(h, 1, m, x.ptr, ld, n_own, x.ptr + n_own * 8, ld, y.ptr, 512))
        blocks.append(cases.live()[1] - start)
    assert blocks == list(range(1, 17)) + [16]
    cases.csr_destroy(h)
    assert cases.live() == base


@pytest.mark.parametrize('device', [False, True], ids=['host', 'device'])
def test_spd(base, device):
    A = cases.matrix('data')
    rc, h = cases.spd_create(A, device)
    cases.check(rc)
    nbytes, ws = cases.spd_bytes(h)
    held = cases.live()
    assert ws == 0 and held[0] - base[0] >= nbytes > 0 and held[1] - base[1] == 8
    cases.spd_apply(h, A, 4)
    small = cases.spd_bytes(h)[1]
    cases.spd_apply(h, A, 64)
    large = cases.spd_bytes(h)[1]
    assert 0 < small < large                          # the workspace grew twice: one block, the larger one
    held = cases.live()
    assert held[1] - base[1] == 9 and held[0] - base[0] >= cases.spd_bytes(h)[0]
    want = np.asarray(A.multiply(A).sum(axis=1)).ravel()
    assert np.allclose(cases.spd_row_sumsq(h, A), want, rtol=1e-12)
    assert cases.live() == held
    assert cases.spd_absmax(h) == np.abs(A.data).max()
    assert cases.live() == held
    cases.spd_destroy(h)
    assert cases.live() == base


@pytest.mark.parametrize('device', [False, True], ids=['host', 'device'])
def test_bytes_copied(base, device):
    D = cases.byte_matrix(100, 70)                     # 70 columns: padded to 80, so a copy from either side
    rc, h, _ = cases.bytes_create(D, device)
    cases.check(rc)
    nbytes, ws = cases.bytes_sizes(h)
    held = cases.live()
    assert nbytes == 100 * 80 and ws == 0 and held[0] - base[0] >= nbytes and held[1] - base[1] == 1
    cases.bytes_apply(h, D)
    sumsq, absmax = cases.bytes_norms(h, D)
    assert np.array_equal(sumsq, (D.astype(np.float64) ** 2).sum(axis=1)) and absmax == D.max()
    assert cases.live() == held                        # 70 columns are one K chunk: no split, no workspace
    cases.bytes_destroy(h)
    assert cases.live() == base


def test_bytes_borrowed(base):
    D = cases.byte_matrix(64, 64)                      # aligned rows of whole 16-byte pieces in device memory: borrowed
    rc, h, keep = cases.bytes_create(D, True)
    cases.check(rc)
    assert cases.bytes_sizes(h) == (0, 0) and cases.live() == base
    cases.bytes_apply(h, D)
    sumsq, absmax = cases.bytes_norms(h, D)
    assert np.array_equal(sumsq, (D.astype(np.float64) ** 2).sum(axis=1)) and absmax == D.max()
    assert cases.live() == base
    cases.bytes_destroy(h)
    assert cases.live() == base
    del keep


def test_bytes_split_k_workspace(base):
    """100 x 4100 times 4 vectors: one workgroup of output, so the split rule of launch_bytes cuts the 4100 columns into
    chunks of at least 512 (9 at the most, 16 allowed): partial tiles in the handle's workspace."""
    D = cases.byte_matrix(100, 4100)
    rc, h, _ = cases.bytes_create(D, False)
    cases.check(rc)
    held = cases.live()
    cases.bytes_apply(h, D)
    nbytes, ws = cases.bytes_sizes(h)
    assert ws >= 2 * 4 * 100 * 4 and nbytes == 100 * 4112 + ws
    now = cases.live()
    assert now[1] == held[1] + 1 and now[0] == held[0] + ws and now[0] - base[0] >= nbytes
    cases.bytes_apply(h, D)                            # the same product again: the workspace is reused
    assert cases.live() == now
    cases.bytes_destroy(h)
    assert cases.live() == base


def test_sptrsv(base):
    """float64: m = 16, 32, 64 are 1, 2 and 4 pieces per lane group (solve_chain_impl: 8 groups of 16-byte pieces), three
    plan widths for the two plan slots of an operator; the chain of two takes three block images where one takes two."""
    rc, lo = cases.trsv_create(0)
    cases.check(rc)
    rc, up = cases.trsv_create(1)
    cases.check(rc)
    created = cases.live()
    assert created[0] > base[0] and created[1] - base[1] == 6
    blocks, held = [], []
    for m in (16, 32, 64):
        cases.trsv_solve([lo], m)
        held.append(cases.live())
        blocks.append(held[-1][1] - created[1])
    assert blocks == [3, 5, 5]                         # workspace + two arrays per plan; the third plan replaces the first
    assert held[0][0] < held[1][0]
    cases.trsv_solve([lo], 16)                         # the evicted plan is built again
    assert cases.live()[1] == held[-1][1]
    cases.trsv_solve([lo, up], 64)
    chained = cases.live()
    assert chained[1] == held[-1][1] + 2 and chained[0] > held[-1][0]
    cases.trsv_destroy(lo)
    cases.trsv_destroy(up)
    assert cases.live() == base


@pytest.mark.parametrize('host', [True, False], ids=['host', 'device'])
@pytest.mark.parametrize('kind', sorted(cases.FSAI_KINDS))
def test_fsai(base, kind, host):
    A = cases.matrix('fsai')
    rc, h = cases.fsai_create(A, kind, host)
    cases.check(rc)
    held = cases.live()
    assert held[0] > base[0] and held[1] - base[1] == 8         # the operator G, G^H alone: the build's arrays are gone
    cases.fsai_apply(h, A)
    now = cases.live()
    assert now[1] == held[1] + 2 and now[0] > held[0]            # the block between the two products, and G's workspace
    cases.fsai_destroy(h)
    assert cases.live() == base


def test_refused_creates_leave_nothing(base):
    S = cases.matrix('random300')
    n = S.shape[0]
    ix = S.indices.astype(np.int64)
    r = int(np.flatnonzero(np.diff(S.indptr) >= 3)[0])
    k = int(S.indptr[r]) + 1                                     # an inner entry of a row of three at least
    rows = np.repeat(np.arange(n), np.diff(S.indptr))
    lower = int(np.flatnonzero(S.indices < rows)[40])
    D = cases.matrix('data')
    F = cases.matrix('fsai')
    refused = {'csr: column out of range': lambda: cases.csr_create(S, 'device', indices=cases.changed(ix, k, n)),
               'csr: unsorted row': lambda: cases.csr_create(S, 'device', indices=cases.swapped(ix, k, k + 1)),
               'csr: mirror_upper, missing partner': lambda: cases.csr_create(cases.without(S, lower), 'device', mirror=1),
               'spd: column out of range': lambda: cases.spd_create(D, True, indices=cases.changed(D.indices.astype(np.int64), 7, D.shape[1])),
               'fsai: column out of range': lambda: cases.fsai_create(F, 'plain', False, indices=cases.changed(F.indices, 7, F.shape[0]))}
    for what, create in refused.items():
        rc, h = create()
        msg = cases.L().rlh_last_error().decode()
        assert rc != 0 and not h.value, what
        assert ('not symmetric' if 'partner' in what else 'ascend' if 'unsorted' in what else 'out of range') in msg, (what, msg)
        assert cases.live() == base, what
    rc, h = cases.csr_create(S, 'device', mirror=1)              # the whole matrix is taken
    cases.check(rc)
    cases.csr_destroy(h)
    assert cases.live() == base


def test_twenty_cycles_hold_nothing_more(base):
    after = []
    for _ in range(20):
        for h, use, destroy in cases.small_handles():
            use()
            destroy(h)
        after.append(cases.live())
    assert after[-1] == after[0] == base


def test_destroy_after_finalize():
    """Handles that outlive the context (interpreter teardown): destroying them frees nothing and does not crash."""
    r = subprocess.run([sys.executable, os.path.join(cases.ROOT, 'tests', '_device_memory_cases.py'), 'teardown'],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
