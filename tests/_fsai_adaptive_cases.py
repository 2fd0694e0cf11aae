"""Adaptive patterns of the approximate inverse (rlh_fsai_create_adaptive*, ApproximateInverse(steps=..., step_size=...)):
cases shared by the CPU tier (tests/fake_fsai.py) and the GPU tier.  The raw entry points (`create`, `built`), matrices,
helpers and the bound of the defining property come from tests/_fsai_cases.py (`base`) and tests/_fsai_levels_cases.py (`lv`).

THE ORACLE (`oracle_row`, `oracle`) is written from the definition in include/rlhip.h and shares nothing with the
library or the stand-in.  Per row, in dense float64 / complex128 NumPy: it starts from the level pattern (`lv.oracle`:
SciPy products of boolean patterns, cut to max_row), and in every step solves S y = e_last on the pattern, forms
r_j = sum_p conj(y_p) a_pj over the members p in ascending order for every column j < i outside the pattern that a
member's row stores, scores |r_j|^2 / a_jj, and takes the largest finite positive scores (at most step_size, at most
max_row - |P|; equal scores the larger column first).  The matrix is the one the upper triangle defines.

WHAT IS COMPARED EXACTLY.  Both implementations form the scores in double, with rounding differences of order
k kappa(S) 2^-53, so a choice between two nearly equal scores may differ.  The oracle returns, per row, the smallest
relative gap (a - b) / a over every pair of scores consecutive in selection order and over the pair (last taken, first
left).  A row with a gap below 1e-9 is left out of the exact comparison; at most 1 % of a case's rows may be left out,
which every case asserts (on the matrices here none is: the smallest gap is above 1e-7).

TRUNCATED ROWS.  A row counts when its level pattern was cut, when it was full before one of its steps began, or when a
step took fewer columns than min(step_size, candidates of positive score) for lack of room.

LAUNCH GEOMETRY the loop case relies on: the enrichment kernel runs at most 8 workgroups per CU and walks the rows of
its bin in a grid-stride loop; rows go to the bin of their capacity min(max_row, k0 + steps * step_size), and the
16-lane bin takes 16 rows per workgroup in real arithmetic (256 threads).
"""

import functools

import numpy as np
import pytest
import scipy.sparse as sp

import _fsai_cases as base
import _fsai_levels_cases as lv
from _fsai_cases import (TYPES, _check, adaptive_of, built, check_row, create, csr_tensor, destroy, hermitian_from_upper, kaporin,
                         last_error, levels_of, same_bits)

BLOCKS_PER_CU = 8
ENRICH_ROWS_PER_BLOCK = {16: 16}
GAP = 1e-9
CONFIGS = ((1, 3, 1, 64), (1, 4, 2, 64), (2, 2, 4, 64), (1, 8, 8, 64), (1, 3, 2, 12))      # levels, steps, step_size, max_row
MATRICES = ('profile-d', 'profile-z', 'cut-d', 'banded-d', 'lap')


def matrix(which):
    return {'profile-d': lambda: base.matrix('d'), 'profile-z': lambda: base.matrix('z'), 'cut-d': lambda: base.matrix('d', 'cut'),
            'banded-d': lambda: lv.banded('d'), 'lap': lambda: lv.lap('d')}[which]()


# ---------------------------------------------------------------- the oracle
class Dense:
    """The operator the upper triangle defines (double / complex double) and the stored structure, with dense blocks
    taken from a dense copy (small matrices) or from the sparse one."""

    def __init__(self, A):
        self.A = A
        self.n = A.shape[0]
        wide = np.complex128 if A.dtype.kind == 'c' else np.float64
        self.F = hermitian_from_upper(A.astype(wide)).tocsr()
        self.D = self.F.toarray() if self.n <= 2048 else None
        self.diag = self.F.diagonal().real

    def block(self, rows, cols):
        if self.D is not None:
            return self.D[np.ix_(rows, cols)]
        return self.F[rows][:, cols].toarray()

    def stored(self, p):
        return self.A.indices[self.A.indptr[p]:self.A.indptr[p + 1]]


def oracle_row(M, i, start, steps, step_size, max_row):
    """Row i from its level pattern `start`: the final pattern, whether max_row held it back, the smallest gap."""
    P = [int(c) for c in start]
    limited, gap = False, np.inf
    for _ in range(steps):
        if len(P) == max_row:
            limited = True
            break
        S = M.block(P, P)
        e = np.zeros(len(P), dtype=S.dtype)
        e[-1] = 1.0
        y = np.linalg.solve(S, e)
        members = set(P)
        cand = sorted({int(j) for p in P for j in M.stored(p) if j < i and j not in members})
        if not cand:
            break
        a = M.block(P, cand)
        r = np.zeros(len(cand), dtype=S.dtype)
        for t in range(len(P)):
            r += np.conj(y[t]) * a[t]
        with np.errstate(divide='ignore', invalid='ignore'):
            score = (r.real ** 2 + r.imag ** 2) / M.diag[cand]
        ranked = sorted((t for t in range(len(cand)) if np.isfinite(score[t]) and score[t] > 0),
                        key=lambda t: (-score[t], -cand[t]))
        room = max_row - len(P)
        want = min(step_size, len(ranked))
        if room < want:
            limited = True
        take = min(want, room)
        if take == 0:
            break
        ordered = [float(score[t]) for t in ranked]
        # the scores in selection order, and the first one left (a candidate without a positive score counts as 0)
        line = ordered[:take] + ([ordered[take]] if len(ordered) > take else ([0.0] if len(cand) > take else []))
        for hi, lo in zip(line, line[1:]):
            gap = min(gap, (hi - lo) / hi)
        P = sorted(P + [cand[t] for t in ranked[:take]])
    return P, limited, gap


class Oracle:
    def __init__(self, A, levels, steps, step_size, max_row):
        M = Dense(A)
        ip0, ix0, cut, _ = lv.oracle(A, levels, max_row)
        self.level_indptr, self.level_indices = ip0, ix0
        rows, self.limited, gaps = [], [], []
        for i in range(M.n):
            P, limited, gap = oracle_row(M, i, ix0[ip0[i]:ip0[i + 1]], steps, step_size, max_row)
            rows.append(np.asarray(P, dtype=np.int64))
            self.limited.append(limited)
            gaps.append(gap)
        self.rows = rows
        lens = np.array([len(p) for p in rows])
        lens0 = np.diff(ip0)
        full0 = lv.full_pattern(A, levels)
        was_cut = np.diff(full0.indptr) > max_row
        self.limited = np.array(self.limited)
        assert np.all(self.limited[was_cut])                    # (a cut row is full before its first step)
        self.gaps = np.array(gaps)
        self.compared = self.gaps >= GAP
        self.indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        self.indices = np.concatenate(rows)
        self.truncated, self.longest = int(self.limited.sum()), int(lens.max())
        self.grew = int(np.sum(lens > lens0))
        self.stopped = int(np.sum(self.limited & (lens > lens0)))         # grew and were then held back by max_row
        self.cut_and_kept = int(np.sum(was_cut & (lens == lens0)))
        assert int(was_cut.sum()) == cut


@functools.lru_cache(maxsize=None)
def _oracle(A_id, levels, steps, step_size, max_row):
    return Oracle(_KEPT[A_id], levels, steps, step_size, max_row)


_KEPT = {}


def oracle(A, levels, steps, step_size, max_row=64):
    """Computed once per matrix object and configuration, never written."""
    _KEPT[id(A)] = A
    return _oracle(id(A), levels, steps, step_size, max_row)


def row_of(G, i):
    return G.indices[G.indptr[i]:G.indptr[i + 1]]


# ---------------------------------------------------------------- 1. the pattern, exactly
def pattern(which, config):
    """`cut-d` (every configuration) and levels = 2 on the matrices whose level-2 pattern max_row cuts (profile, cut,
    banded; the 6 x 5 x 4 Laplacian has no such row) must have cut rows that did not grow; (1, 8, 8, 64) and
    (1, 3, 2, 12) on profile and banded must have rows that grew and were then stopped by max_row."""
    levels, steps, step_size, max_row = config
    A = matrix(which)
    n = A.shape[0]
    o = oracle(A, levels, steps, step_size, max_row)
    left_out = int(np.sum(~o.compared))
    print('%s %s: %d rows grew, %d stopped by max_row, %d cut and kept, %d left out, smallest gap %.3g'
          % (which, config, o.grew, o.stopped, o.cut_and_kept, left_out, float(o.gaps.min())))
    assert left_out <= n // 100
    assert o.grew > 0
    if config in ((1, 8, 8, 64), (1, 3, 2, 12)) and which in ('profile-d', 'profile-z', 'banded-d'):
        assert o.stopped > 0
    if which == 'cut-d' or (levels == 2 and which != 'lap'):
        assert o.cut_and_kept > 0
    for bits in (32, 64):
        G, f = built(A, '_adaptive', levels, steps, step_size, bits=bits, max_row=max_row)
        assert f['nnz'] == G.nnz == int(G.indptr[-1]) and G.shape == (n, n)
        if left_out == 0:
            assert np.array_equal(G.indptr, o.indptr) and np.array_equal(G.indices, o.indices), (which, config, bits)
            assert f['longest'] == o.longest and f['truncated'] == o.truncated, (f, o.longest, o.truncated)
        else:
            for i in np.flatnonzero(o.compared):
                assert np.array_equal(row_of(G, i), o.rows[i]), (which, config, bits, i)


# ---------------------------------------------------------------- 2. padding, bit for bit
def padded_on(A, G):
    """A plus explicit zeros on the pattern of G and its mirror image (as lv.padded, from a fetched pattern)."""
    return base.padded_with(A, np.repeat(np.arange(A.shape[0]), np.diff(G.indptr)), G.indices)


def padding(code):
    for A, (levels, steps, step_size) in ((lv.lap(code), (1, 4, 2)), (lv.banded(code), (2, 2, 4)), (lv.banded(code), (1, 4, 2))):
        for max_row in (64, 12):
            G, f = built(A, '_adaptive', levels, steps, step_size, max_row=max_row)
            assert G.nnz > lv.oracle(A, levels, max_row)[1].size               # (it grew)
            want, _ = built(padded_on(A, G), max_row=max_row)
            assert same_bits(G, want), (levels, steps, step_size, max_row)
            Gh, fh = built(A, '_adaptive', levels, steps, step_size, host=True, max_row=max_row)
            assert same_bits(Gh, want) and fh['truncated'] == f['truncated'] and fh['longest'] == f['longest']


# ---------------------------------------------------------------- 3. the defining property on the adaptive pattern
def defining_property(code, config):
    levels, steps, step_size = config
    A, D = base.matrix(code), base.dense_wide(code)
    n = A.shape[0]
    B = A.copy()
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    B.data[B.indices < rows] = np.nan                      # nothing below the diagonal is read
    G, f = built(B, '_adaptive', levels, steps, step_size, bits=32)
    ip0, ix0, _, _ = lv.oracle(A, levels, 64)
    assert G.nnz > ix0.size
    worst = 0.0
    for i in range(n):
        p = row_of(G, i)
        assert np.all(np.diff(p) > 0) and p[-1] == i and p[0] >= 0
        assert np.all(np.isin(ix0[ip0[i]:ip0[i + 1]], p)), i
        worst = max(worst, check_row(G, i, p, D[np.ix_(p, p)], TYPES[code]))
    print('largest residual / bound: %.3g' % worst)


# ---------------------------------------------------------------- 4. nesting and quality
def nesting():
    for A in (lv.lap('d', 8, 8, 8), lv.banded('d', narrow=True)):
        n = A.shape[0]
        u = base.unit(np.float64)
        for step_size in (1, 3):
            before, _ = built(A, '_levels', 1, bits=32)
            for t in (1, 2, 3, 4):
                G, _ = built(A, '_adaptive', 1, t, step_size, bits=32)
                assert G.nnz > before.nnz, (t, step_size)
                for i in range(n):
                    assert np.all(np.isin(row_of(before, i), row_of(G, i))), (t, step_size, i)
                k = np.diff(G.indptr)
                assert np.all(G.diagonal() >= before.diagonal() * (1 - 100 * k * u)), (t, step_size)
                before = G


def quality():
    out = []
    for A in (lv.lap('d', 8, 8, 8), lv.banded('d', narrow=True)):
        n = A.shape[0]
        d = hermitian_from_upper(A).toarray()
        ks = []
        for steps, step_size in ((0, 0), (2, 3), (4, 4)):
            G, _ = built(A, '_adaptive', 1, steps, step_size, bits=32) if steps else built(A, '_levels', 1, bits=32)
            g = G.toarray()
            ks.append(kaporin(g @ d @ g.T))
        print('Kaporin numbers at level 1, + 2 steps of 3, + 4 steps of 4 (n = %d): %.6f %.6f %.6f' % ((n,) + tuple(ks)))
        for a, b in zip(ks, ks[1:]):
            assert b <= a * (1 + 100 * n * base.unit(np.float64))
        out.append(ks)
    return out


# ---------------------------------------------------------------- 5. steps = 0 and the defaults
def unchanged_without_steps(code, device):
    from raleigh_amd.algebra.hip.precond import ApproximateInverse
    A = base.matrix(code)
    want, _ = built(A, bits=32)
    made = [ApproximateInverse(A), ApproximateInverse(A, steps=0, step_size=5), ApproximateInverse(csr_tensor(A, device), steps=0)]
    for T in made:
        assert same_bits(T.csr(), want) and (T.levels, T.steps) == (1, 0)
        assert adaptive_of(T._h) == (0, 0)
    assert made[0].step_size == 1 and made[1].step_size == 5
    two, _ = built(A, '_levels', 2, bits=32)
    assert same_bits(ApproximateInverse(A, levels=2, steps=0).csr(), two)


# ---------------------------------------------------------------- 6. the bins
def bins(code, monkeypatch):
    A = lv.banded(code)
    monkeypatch.setenv('RLH_FSAI_BINS', '0')
    two, f2 = built(A, '_adaptive', 1, 4, 2, bits=32)
    monkeypatch.delenv('RLH_FSAI_BINS')
    four, f4 = built(A, '_adaptive', 1, 4, 2, bits=32)
    assert same_bits(two, four) and f2['truncated'] == f4['truncated'] and f2['longest'] == f4['longest']
    lens = np.diff(four.indptr)
    for lo, hi in lv.CLASSES[:4]:
        assert np.any((lens >= lo) & (lens <= hi)), (lo, hi)


# ---------------------------------------------------------------- 7. past one pass of the enrichment grid (GPU tier)
def loops(cu):
    """A band of w = 4 at (1, 2, 2): level rows of 5 entries with capacity 9, the 16-lane bin, more of them than one
    pass of its grid holds."""
    w, levels, steps, step_size = 4, 1, 2, 2
    per_pass = cu * BLOCKS_PER_CU * ENRICH_ROWS_PER_BLOCK[16]
    n = per_pass + 300
    A = lv.band(np.full(n, w), np.float64, 33)
    G, f = built(A, '_adaptive', levels, steps, step_size, bits=32)
    lens0 = np.minimum(np.arange(n), w) + 1
    in_bin = np.flatnonzero(lens0 + steps * step_size > 8)               # ascending: the order of the bin's list
    assert in_bin.size > per_pass and np.all(lens0[in_bin] + steps * step_size <= 16)
    rows = [0, 1, w, in_bin[per_pass - 1], in_bin[per_pass], n - 1]
    M = Dense(A)
    for i in sorted(set(int(r) for r in rows)):
        start = np.arange(max(i - w, 0), i + 1)
        P, limited, gap = oracle_row(M, i, start, steps, step_size, 64)
        assert gap >= GAP and not limited, (i, gap)
        p = np.asarray(P)
        check_row(G, i, p, M.block(p, p).astype(np.longdouble), np.float64)      # (asserts the pattern too)
    assert f['truncated'] == 0 and f['longest'] == int(np.diff(G.indptr).max()) <= w + 1 + steps * step_size


# ---------------------------------------------------------------- 8. rejections
def indefinite():
    """Tridiagonal, every 2 x 2 block on consecutive indices positive definite, the 3 x 3 block on 19, 20, 21 not: row
    21 (level pattern 20, 21) takes column 19 in its first step."""
    n = 50
    d = np.full(n, 4.0)
    o = np.full(n - 1, -1.0)
    d[19:22] = 1.0
    o[19:21] = 0.8
    A = sp.csr_matrix(sp.diags([o, d, o], [-1, 0, 1]))
    A.sort_indices()
    return A


def rejections_raw():
    A = base.matrix('d')
    for host, name in ((False, 'rlh_fsai_create_adaptive_device'), (True, 'rlh_fsai_create_adaptive')):
        for args, kw, text in (((1, 0, 1), {}, 'steps must lie in [1, 63], got 0'), ((1, 64, 1), {}, 'steps must lie in [1, 63], got 64'),
                               ((1, 1, 0), {}, 'step_size must lie in [1, 16], got 0'),
                               ((1, 1, 17), {}, 'step_size must lie in [1, 16], got 17'),
                               ((0, 1, 1), {}, 'levels must lie in [1, 8], got 0'), ((9, 1, 1), {}, 'levels must lie in [1, 8], got 9'),
                               ((1, 1, 1), {'max_row': 65}, 'max_row must lie in [1, 64], got 65')):
            rc, h = create(A, '_adaptive', *args, host=host, **kw)
            assert rc != 0 and not h.value, (name, args)
            assert last_error().endswith('%s: %s' % (name, text)), last_error()
        B = indefinite()
        for steps in (1, 2):                # found by the set-up of the final pattern, by the second step's own solve
            rc, h = create(B, '_adaptive', 1, steps, 1, host=host)
            assert rc != 0 and not h.value
            assert last_error().endswith('%s: local block of row 21 is not positive definite' % name), last_error()
        rc, h = create(A, '_adaptive', 8, 63, 16, host=host, max_row=3)
        _check(rc)
        assert levels_of(h) == 8 and adaptive_of(h) == (63, 16)
        destroy(h)
    rc, h = create(B, '_levels', 1)                             # (the level pattern alone is fine)
    _check(rc)
    assert adaptive_of(h) == (0, 0)
    destroy(h)


def rejections_class(fake=None):
    from raleigh_amd.algebra.hip.precond import ApproximateInverse
    A = base.matrix('d')
    before = dict(fake.calls) if fake is not None else None
    for steps in (-1, 64):
        with pytest.raises(ValueError, match=r'steps must lie in \[0, 63\], got %d' % steps):
            ApproximateInverse(A, steps=steps)
    for step_size in (0, 17):
        with pytest.raises(ValueError, match=r'step_size must lie in \[1, 16\], got %d' % step_size):
            ApproximateInverse(A, steps=1, step_size=step_size)
    for levels in (0, 9):
        with pytest.raises(ValueError, match=r'levels must lie in \[1, 8\], got %d' % levels):
            ApproximateInverse(A, levels=levels, steps=1)
    with pytest.raises(ValueError, match='max_row'):
        ApproximateInverse(A, max_row=65, steps=1)
    if fake is not None:
        assert dict(fake.calls) == before                   # refused before any library call


# ---------------------------------------------------------------- 9. the class: three kinds of input
def class_inputs(device):
    from raleigh_amd.algebra.hip.precond import ApproximateInverse
    A = lv.banded('d')
    want, f = built(A, '_adaptive', 1, 4, 2)
    made = [ApproximateInverse(A, steps=4, step_size=2), ApproximateInverse(csr_tensor(A, device), steps=4, step_size=2),
            ApproximateInverse(csr_tensor(A, 'cpu'), steps=4, step_size=2)]
    for T in made:
        assert (T.levels, T.steps, T.step_size) == (1, 4, 2) and same_bits(T.csr(), want)
        assert adaptive_of(T._h) == (4, 2) and levels_of(T._h) == 1
        assert T.truncated_rows == f['truncated'] and T.longest_row == f['longest'] and T.nnz == want.nnz
        assert abs(T.fill - want.nnz / A.nnz) < 1e-15
    return made


# ---------------------------------------------------------------- 10. end to end
def end_to_end(device):
    import scipy.linalg
    import torch
    from raleigh_amd.interfaces import partial_hevp
    from raleigh_amd.algebra.hip.precond import ApproximateInverse
    A = lv.lap('d', 12, 11, 10)
    which = 6
    exact = scipy.linalg.eigvalsh(hermitian_from_upper(A).toarray())[:which]
    a = csr_tensor(A, device)
    its = {}
    for steps in (2, 0):
        T = ApproximateInverse(a, steps=steps, step_size=3)
        np.random.seed(1)
        lmd, x, status = partial_hevp(a, T=T, which=which, tol=1e-6, verb=-1)
        its[steps] = partial_hevp.last['iterations']
        assert status == 0
        if steps:
            assert np.max(np.abs(lmd[:which] - exact)) <= 1e-10
            assert isinstance(x, torch.Tensor) and x.device.type == torch.device(device).type
    print('iterations: %d at level 1 + 2 steps of 3, %d at level 1' % (its[2], its[0]))
    assert its[2] < its[0]
    return its
