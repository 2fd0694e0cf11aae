"""Device-resident preconditioners.

The reference's preconditioner is MKL's ILUT applied on the host with two triangular solves
per vector (raleigh/algebra/mkl_wrap.py:279-347).  `IncompleteLU` is its device counterpart:
the same dual-threshold factorisation on the host once, the triangular solves on the whole
block in HBM (`TriangularChain`: one persistent launch per application).  `ApproximateInverse` is
the preconditioner that is also SET UP on the device (a factorised sparse approximate inverse: one
small dense solve per row, applied by two sparse products), from a SciPy matrix or a tensor on the GPU.
`ChebyshevPreconditioner` is what the survey lists as the alternative: a
fixed polynomial p(A) ~ A^-1 (Chebyshev semi-iteration on [lo, hi]) built only from the
operator's ``apply`` and the block operations, so every block stays in HBM.  p(A) is
symmetric positive definite for a positive definite A (0 < 1 - r(x) on (0, hi], r the
Chebyshev residual polynomial), as the solver requires of a preconditioner
(raleigh/interfaces/partial_hevp.py:41-49).  It changes iteration counts relative to ILU, so
runs using it are reported separately from the reference's.
"""

import ctypes

import numpy as np

from ... import _lib


class TriangularChain:
    """X = T_k^-1 ... T_1^-1 B on the device for sparse triangular factors given as SciPy matrices
    (one persistent launch over the whole n x m block: rlh_sptrsv_create / rlh_sptrsv_solve_chain).

    factors: list of (matrix, lower, unit_diag); a unit-diagonal factor must not store its diagonal.
    perm_in / perm_out: optional row permutations (row r of the internal block is row perm_in[r] of
    B, and is written to row perm_out[r] of X)."""

    def __init__(self, factors, dtype, perm_in=None, perm_out=None):
        import scipy.sparse as scs
        L = self._L = _lib.lib()                          # (the handles belong to THIS library object)
        self._dtype = np.dtype(dtype).type
        self._code = _lib.dtype_code(self._dtype)
        self._ops = []
        self._n = None
        self.levels, self.nnz = [], []
        prepared = []
        for mat, lower, unit in factors:
            a = scs.csr_matrix(mat, dtype=self._dtype)
            a.sort_indices()
            n = a.shape[0]
            if self._n not in (None, n) or a.shape[0] != a.shape[1]:
                raise ValueError('the triangular factors must be square and of one size')
            self._n = n
            prepared.append((np.ascontiguousarray(a.indptr, dtype=np.int64), np.ascontiguousarray(a.indices, dtype=np.int32),
                             np.ascontiguousarray(a.data), 1 if lower else 0, 1 if unit else 0))

        def create(args):
            indptr, indices, values, lower, unit = args
            h = ctypes.c_void_p()
            rc = L.rlh_sptrsv_create(ctypes.byref(h), self._code, self._n, _lib.host_ptr(indptr), _lib.host_ptr(indices),
                                     _lib.host_ptr(values), lower, unit)
            err = None
            if rc != 0:                                    # (the library's error text is per thread: read where it was set)
                try:
                    _lib.check(rc)
                except _lib.RlhError as e:
                    err = e
            return err, h
        # the host side of rlh_sptrsv_create (diagonal-block transform, levels, units) is serial per factor and the factors of
        # a chain are independent: large ones are set up side by side (ctypes releases the GIL for the call; 0.67 -> 0.35 s for
        # the two ILUT factors of the config-3 surrogate)
        if len(prepared) > 1 and sum(len(p[1]) for p in prepared) > 2_000_000:
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(max_workers=len(prepared)) as ex:
                made = list(ex.map(create, prepared))
        else:
            made = [create(p) for p in prepared]
        for err, h in made:
            if h:
                self._ops.append(h)
        for err, h in made:
            if err is not None:
                raise err
        for h in self._ops:
            nnz, lev, nb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
            _lib.check(L.rlh_sptrsv_info(h, ctypes.byref(nnz), ctypes.byref(lev), ctypes.byref(nb)))
            self.levels.append(int(lev.value))
            self.nnz.append(int(nnz.value))
        self._arr = (ctypes.c_void_p * len(self._ops))(*[h.value for h in self._ops])
        self._perms = []
        for perm in (perm_in, perm_out):
            if perm is None:
                self._perms.append(None)
                continue
            from .memory import DeviceBuffer
            host = np.ascontiguousarray(perm, dtype=np.int64)
            buf = DeviceBuffer(host.nbytes, zero=False)
            _lib.check(L.rlh_h2d(buf.ptr, _lib.host_ptr(host), host.nbytes))
            self._perms.append(buf)

    def __del__(self):
        ops, self._ops = getattr(self, '_ops', []), []
        for h in ops:
            try:
                self._L.rlh_sptrsv_destroy(h)
            except Exception:
                pass

    def size(self):
        return self._n

    def algorithmic_bytes(self, m):
        """Entries of the factors (value + 4-byte column index) + one read of B and one write of X."""
        es = np.dtype(self._dtype).itemsize
        return sum(self.nnz) * (es + 4) + 2 * self._n * m * es

    def solve(self, b, x):
        """x = chain^-1 b for Vectors windows of equal size (b may be x)."""
        m = b.nvec()
        if m != x.nvec():
            raise ValueError('Numbers of input and output vectors differ')
        if b.data_type() != self._dtype or x.data_type() != self._dtype:
            raise ValueError('Factors and vectors data types differ')
        n = getattr(b, 'local_dimension', b.dimension)()
        if n != self._n:
            raise ValueError('Factors and vectors dimensions incompatible')
        pin, pout = self._perms
        _lib.check(self._L.rlh_sptrsv_solve_chain(
            len(self._ops), self._arr, pin.ptr if pin else None, pout.ptr if pout else None, m,
            b.data_ptr(), b.ld(), x.data_ptr(), x.ld()))

    apply = solve


def ilut(matrix, tol=1e-6, maxfil=None):
    """Dual-threshold incomplete LU of a SciPy sparse matrix (rlh_ilut_factor: the host
    factorisation behind IncompleteLU; counterpart of mkl dcsrilut, mkl_wrap.py:305-331).
    Returns (L strictly lower with unit diagonal implied, U upper) as CSR in double / complex double."""
    import scipy.sparse as scs
    a = scs.csr_matrix(matrix)
    a.sort_indices()
    n = a.shape[0]
    cplx = np.iscomplexobj(a.data)
    dt = np.complex128 if cplx else np.float64
    if maxfil is None:
        maxfil = min(n - 1, a.nnz // max(n, 1))
    indptr = np.ascontiguousarray(a.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(a.indices, dtype=np.int32)
    values = np.ascontiguousarray(a.data, dtype=dt)
    L = _lib.library()                         # host-only entry points: no device needed
    f = ctypes.c_void_p()
    _lib.check(L.rlh_ilut_factor(ctypes.byref(f), _lib.DTYPE_CODE[dt], n, _lib.host_ptr(indptr), _lib.host_ptr(indices),
                                 _lib.host_ptr(values), float(tol), int(maxfil)))
    try:
        nl, nu = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(L.rlh_factors_nnz(f, ctypes.byref(nl), ctypes.byref(nu)))
        out = []
        for which, nnz in ((0, nl.value), (1, nu.value)):
            ip = np.zeros(n + 1, dtype=np.int64)
            ix = np.zeros(max(nnz, 1), dtype=np.int32)
            va = np.zeros(max(nnz, 1), dtype=dt)
            _lib.check(L.rlh_factors_get(f, which, _lib.host_ptr(ip), _lib.host_ptr(ix), _lib.host_ptr(va)))
            m = scs.csr_matrix((va[:nnz], ix[:nnz], ip), shape=(n, n))
            m.sort_indices()
            out.append(m)
    finally:
        L.rlh_factors_destroy(f)
    return out[0], out[1]


class IncompleteLU:
    """Incomplete LU preconditioner applied on the device (same surface as the reference's
    IncompleteLU, raleigh/algebra/sparse_mkl.py:122-140: construct from the matrix, `factorize(tol,
    max_fill)`, `apply(x, y)`).  The reference factorises with mkl dcsrilut and applies two
    mkl_dcsrtrsv per vector on the host; here the same dual-threshold ILUT runs once on the host
    (rlh_ilut_factor) and the two triangular solves run on the whole block in HBM."""

    def __init__(self, matrix):
        import scipy.sparse as scs
        self._a = scs.csr_matrix(matrix)
        self._a.sort_indices()
        self._chain = None

    def factorize(self, tol=1e-6, max_fill=1):
        n = self._a.shape[0]
        maxfil = min(n - 1, (self._a.nnz // n) * max_fill)       # mkl_wrap.py:306
        lo, up = ilut(self._a, tol, maxfil)
        self._chain = TriangularChain([(lo, True, True), (up, False, False)], self._a.dtype)
        self.fill = (lo.nnz + up.nnz) / float(self._a.nnz)
        self.levels = tuple(self._chain.levels)

    def chain(self):
        return self._chain

    def apply(self, x, y):
        if self._chain is None:
            self.factorize()
        self._chain.solve(x, y)


# The forms of the approximate inverse's own application (`work` of ApproximateInverse and of
# dist.ShardedApproximateInverse) and the code the library's plans take for each.
WORK = {'native': 0, 'float32': 1, 'bf16': 2}


def check_work(work, dtype=None, none_ok=False):
    """Refuses a `work` that is no key of WORK (None passes with none_ok) and, once the matrix type is known, 'bf16'
    on a complex one."""
    if not (work in WORK or (none_ok and work is None)):
        raise ValueError("work must be %s'native', 'float32' or 'bf16', got %r" % ('None, ' if none_ok else '', work))
    if dtype is not None and work == 'bf16' and np.dtype(dtype).kind == 'c':
        raise ValueError("work='bf16' is for real matrices only")


def work_element_bytes(work, dtype):
    """(bytes of a stored value of G and G^H, bytes of an element of W) of a `work` plan on a matrix of type dtype."""
    es = np.dtype(dtype).itemsize
    ev = es if work == 'native' else min(es, 8 if np.dtype(dtype).kind == 'c' else 4)
    return ev, (2 if work == 'bf16' else ev)


def create_entry(levels, steps, step_size, drop, prefilter):
    """The library's create call for these (checked) arguments: (stem, the arguments after max_row).  The entry point
    is stem + '_device' for a tensor on the GPU and stem for host arrays.  Level 1 without anything else goes through
    the entry points it always had."""
    if prefilter:
        return 'rlh_fsthreshold_create', (levels, steps, step_size, drop, prefilter)
    if drop:
        return 'rlh_fsfilter_create', (levels, steps, step_size, drop)
    if steps:
        return 'rlh_fsai_create_adaptive', (levels, steps, step_size)
    if levels > 1:
        return 'rlh_fsai_create_levels', (levels,)
    return 'rlh_fsai_create', ()


class ApproximateInverse:
    """Factorised sparse approximate inverse T = G^H G ~ A^-1 (Kolotilina-Yeremin) of a Hermitian positive definite
    matrix, built AND applied on the device (rlh_fsai_*): the preconditioner for a matrix that already lies on the
    GPU, and for matrices whose ILU application is bound by the triangular solves' dependency chain.

    matrix: a SciPy sparse matrix, a square ``torch.sparse_csr`` tensor on the bound GPU (built by kernels from its
    three arrays: nothing visits the host) or a CPU tensor (taken as its SciPy matrix).  Both triangles must be stored;
    the UPPER one defines the operator, as for SparseSymmetricMatrix, and values below the diagonal are never read.

    Row i of the lower triangular G lives on the stored columns j <= i of row i (the `max_row` largest of them, 1 ..
    64, if there are more) and solves S g^H = e_k / g_kk, g_kk > 0, S the matching block of A, in double precision
    whatever the storage type.  T is Hermitian positive definite by construction, as the solver requires;
    ``apply`` is two sparse products.  It changes iteration counts relative to ILU, so runs using it are reported
    separately from the reference's.

    levels (1 .. 8) widens the pattern to that of the `levels`-th power of the lower triangle of A: with L(i) the
    stored columns j <= i of row i, level 1 is L(i) and level l + 1 the union of L(j) over the columns j of level l.
    The patterns are nested, so without truncation a higher level never has a larger Kaporin number; it costs more
    entries per row (on a 7-point stencil 4, 10 and 20 at levels 1, 2 and 3) and a longer set-up.  Rows keep the
    `max_row` largest columns of their pattern; `truncated_rows` counts those whose full pattern has more.
    ``levels=1`` is the build described above, bit for bit.

    steps (0 .. 63) and step_size (1 .. 16) make the pattern adaptive: after the level pattern every row goes through
    `steps` enrichment steps, each adding the (at most `step_size`) columns j < i outside its pattern P, stored in some
    row of P, that lower the Kaporin functional g A g^H of the row most: those of the largest |sum_p g_p a_pj|^2 / a_jj,
    g the row solved on P.  The choice is by value, made on the device, and invariant under diagonal scaling; a row
    stops at `max_row` columns or when no candidate lowers the functional.  `truncated_rows` then counts the rows that
    `max_row` held back: cut level patterns, rows full before one of their steps, steps that had to leave candidates
    for lack of room.  ``steps=0`` (the default) is the build without enrichment through the entry points it always had.

    work (None, 'native', 'float32' or 'bf16') chooses how T is applied.  ``None`` (the default) is the application it
    always had: two products of the general sparse data operator (rlh_fsai_apply).  The other values make a plan
    (rlh_fsapply_*) after the build and apply T by its own two kernels, W = G x held between them in a layout made for
    the second product's gathers: 'native' keeps the values of G and W in the matrix type, 'float32' rounds G once to
    float32 / complex64 and keeps W in that type (on float32 / complex64 matrices it is 'native'), 'bf16' (real
    matrices only) keeps G in float32 and W in bfloat16.  The arithmetic stays in the matrix type.  The low-precision
    forms are for blocks inside the float32 range.  They change iteration counts by a few, not the accuracy of the
    eigenpairs, because the residuals are formed with A in full precision; the solver then sees a preconditioner that
    is linear only up to the rounding of W, exactly as with ``ChebyshevPreconditioner(storage='bf16')``.  `csr()` still
    returns G in the matrix type: the handle keeps it.

    drop (0 <= drop < 1) filters the computed G by value (post-filtration): in row i the entry g_ij, j < i, stays iff
    |g_ij| sqrt(a_jj) >= drop g_ii sqrt(a_ii), a measure that does not change under diagonal scaling of A; the diagonal
    always stays.  Every row is then solved again on the columns that are left, so G is still the Kaporin minimiser on
    its pattern and T stays Hermitian positive definite: fewer entries to stream in every application for (on the
    matrices measured) a few more iterations.  The build stays on the device (rlh_fsfilter_create*), one filter and
    one more solve per row.  `dropped_entries` counts what was removed; `nnz`, `fill`, `longest_row`, `csr()` and a
    `work` plan describe the filtered G, `truncated_rows` what `max_row` held back before it.  ``drop=0`` (the default)
    is the build without filtration through the entry points it always had.

    prefilter (0 <= prefilter < 1) chooses the level pattern by value (prefiltration, Chow's a-priori patterns of the
    thresholded matrix): the stored entry (i, j), j < i, is strong iff |a_ij| >= prefilter sqrt(a_ii a_jj), a measure that
    does not change under diagonal scaling of A, and the pattern of row i is that of the `levels`-th power of the lower
    triangle of the strong entries, the diagonal always a member, cut to the `max_row` largest columns after every level
    as before.  The weak entries shape the pattern, not the matrix: every row is solved on its pattern with the full
    block of A, enrichment takes its candidates from the full rows, `drop` filters the computed G, and `update_values`
    keeps the pattern without applying the rule again.  Where the unfiltered level pattern overflows `max_row` the cut
    keeps columns by position alone; with the filter fewer rows overflow, and the cut, which still applies after every
    level, has less to cut.  Measured (profiles/r22_approx_inverse_prefilter.txt): fewer entries to stream at every level;
    the iterations stay where the weak couplings are weak by orders of magnitude (anisotropic Laplacian, level 3: 3.9
    entries per row for 19.3, 603 iterations for 602), fall where the cut did the damage (FE surrogate, level 3,
    prefilter 0.02: 63 for 93) and rise, by more than the cheaper application wins back, where the couplings are all
    of one size (lap3d with couplings 1 : 1.01 : 1.02, every line loses).  The build stays on
    the device (rlh_fsthreshold_create*).  `weak_entries` counts the stored entries below the diagonal that were not
    strong.  ``prefilter=0`` (the default) is the build by position through the entry points it always had.

    `update_values(matrix)` keeps the pattern and solves every row again for a new matrix of the same size and type:
    the set-up of a sequence of matrices (continuation, a parameter sweep, a nonlinear or time-dependent operator)
    pays for the pattern once.  The result is the Kaporin minimiser for the new matrix on the kept pattern.  It is bit
    for bit the fresh build where the pattern came from `levels` alone and the structure of the matrix is unchanged;
    where the pattern was chosen by value (`steps`, `drop`) for the old values it is a different, still Hermitian
    positive definite, preconditioner than a fresh build would give."""

    WORK = WORK

    def __init__(self, matrix, max_row=64, levels=1, steps=0, step_size=1, work=None, drop=0.0, prefilter=0.0):
        L = self._L = _lib.lib()                          # (the handle belongs to THIS library object)
        self._h = self._plan = None
        check_work(work, none_ok=True)
        self.work = work
        max_row = int(max_row)
        if not 1 <= max_row <= 64:
            raise ValueError('max_row must lie in [1, 64], got %d' % max_row)
        levels = int(levels)
        if not 1 <= levels <= 8:
            raise ValueError('levels must lie in [1, 8], got %d' % levels)
        steps, step_size = int(steps), int(step_size)
        if not 0 <= steps <= 63:
            raise ValueError('steps must lie in [0, 63], got %d' % steps)
        if not 1 <= step_size <= 16:
            raise ValueError('step_size must lie in [1, 16], got %d' % step_size)
        drop = float(drop)
        if not 0.0 <= drop < 1.0:                           # (false for NaN)
            raise ValueError('drop must lie in [0, 1), got %g' % drop)
        prefilter = float(prefilter)
        if not 0.0 <= prefilter < 1.0:                      # (false for NaN)
            raise ValueError('prefilter must lie in [0, 1), got %g' % prefilter)
        self.levels, self.steps, self.step_size, self.drop, self.prefilter = levels, steps, step_size, drop, prefilter
        name, more = create_entry(levels, steps, step_size, drop, prefilter)
        self._dtype, self._n, self._nnz_a, bits, pointers, _alive = self._matrix_arrays(matrix)
        code = _lib.DTYPE_CODE[self._dtype]
        # the arguments between the handle and max_row (the arrays they point at live to the call)
        if bits is not None:
            name, args = name + '_device', (code, self._n, bits) + pointers
        else:
            args = (code, self._n) + pointers
        h = ctypes.c_void_p()
        check_work(work, self._dtype, none_ok=True)
        self._create(getattr(L, name), name, h, *args, max_row, *more)
        self._finish(h)
        if work is not None:
            plan = ctypes.c_void_p()
            _lib.check(L.rlh_fsapply_create(ctypes.byref(plan), h, self.WORK[work]))
            self._plan = plan

    @staticmethod
    def _matrix_arrays(matrix):
        """What the constructor and `update_values` take as a matrix: (type, n, stored entries, index bits, the pointers
        to row pointers, columns and values, the arrays those point at).  index bits 32 / 64: a tensor on the GPU, used
        where it is (DEVICE pointers); None: a SciPy matrix or a CPU tensor as its SciPy matrix, canonical CSR with int64
        row pointers and int32 columns (host pointers)."""
        from . import device_data
        t = None
        if device_data.is_tensor(matrix):
            from .sparse import operator_tensor
            t = operator_tensor(matrix)
            if not device_data._on_device(t):
                matrix, t = device_data.to_host(t), None
        if t is not None:
            import torch
            crow, col, val = t.crow_indices(), t.col_indices(), t.values()
            if col.dtype != crow.dtype:                     # (torch takes mixed index types: both as the wider one)
                crow, col = crow.to(torch.int64), col.to(torch.int64)
            crow, col = crow.contiguous(), col.contiguous()
            val = val.detach().resolve_conj().resolve_neg().contiguous()
            if val.is_cuda:                                 # the conversions may have launched work on torch's stream
                torch.cuda.current_stream(val.device).synchronize()
            pointers = (ctypes.c_void_p(crow.data_ptr()), ctypes.c_void_p(col.data_ptr()), ctypes.c_void_p(val.data_ptr()))
            return (device_data.numpy_type(t), int(t.shape[0]), int(val.numel()), 32 if crow.element_size() == 4 else 64,
                    pointers, (crow, col, val))
        from .sparse_data import canonical_csr
        a = canonical_csr(matrix)
        if a.shape[0] != a.shape[1]:
            raise ValueError('a square matrix is needed, got %d x %d' % a.shape)
        indptr = np.ascontiguousarray(a.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(a.indices, dtype=np.int32)
        values = np.ascontiguousarray(a.data)
        pointers = (_lib.host_ptr(indptr), _lib.host_ptr(indices), _lib.host_ptr(values))
        return a.dtype.type, int(a.shape[0]), int(a.nnz), None, pointers, (indptr, indices, values)

    @staticmethod
    def _create(fn, name, h, *args):
        ApproximateInverse._checked(fn, name, ctypes.byref(h), *args)

    @staticmethod
    def _checked(fn, name, *args):
        try:
            _lib.check(fn(*args))
        except _lib.RlhError as e:
            text = str(e)
            if ': %s:' % name not in text:                  # a HIP failure, not the library's own check
                raise
            if 'indptr' in text or 'column' in text:
                raise ValueError('the sparse matrix is not canonical CSR: %s' % e)
            raise

    def _finish(self, h):
        self._h = h
        n, nnz, longest, cut, nbytes, sec = (ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(),
                                             ctypes.c_int64(), ctypes.c_double())
        _lib.check(self._L.rlh_fsai_info(h, ctypes.byref(n), ctypes.byref(nnz), ctypes.byref(longest), ctypes.byref(cut),
                                         ctypes.byref(nbytes), ctypes.byref(sec)))
        self.nnz = int(nnz.value)
        self.longest_row = int(longest.value)
        self.truncated_rows = int(cut.value)
        self.setup_seconds = float(sec.value)
        self.fill = self.nnz / float(max(self._nnz_a, 1))
        self.dropped_entries = 0
        self.updates, self.update_seconds = 0, 0.0
        if self.drop:
            drop, removed = ctypes.c_double(), ctypes.c_int64()
            _lib.check(self._L.rlh_fsfilter_info(h, ctypes.byref(drop), ctypes.byref(removed)))
            self.dropped_entries = int(removed.value)
        self.weak_entries = 0
        if self.prefilter:
            tau, weak = ctypes.c_double(), ctypes.c_int64()
            _lib.check(self._L.rlh_fsthreshold_info(h, ctypes.byref(tau), ctypes.byref(weak)))
            self.weak_entries = int(weak.value)

    def __del__(self):
        plan, self._plan = getattr(self, '_plan', None), None
        if plan:
            try:
                self._L.rlh_fsapply_destroy(plan)
            except Exception:
                pass
        h, self._h = getattr(self, '_h', None), None
        if h:
            try:
                self._L.rlh_fsai_destroy(h)
            except Exception:
                pass

    def update_values(self, matrix):
        """New matrix values on the kept pattern: every row of G is solved again for `matrix` on the columns it has
        (rlh_fsvalues_update*: the numeric phase of the build alone, on the device), then the plan of a `work` form is
        refilled.  matrix: what the constructor takes, of the same size and type; its structure may differ (a position
        it does not store counts as zero).  `updates` counts the successful calls, `update_seconds` holds the device
        seconds of the last; `nnz`, `fill`, `longest_row`, `truncated_rows`, `dropped_entries`, `weak_entries` and `setup_seconds` keep
        describing the build.  A refused matrix leaves the preconditioner as it was."""
        dtype, n, _, bits, pointers, _alive = self._matrix_arrays(matrix)
        if n != self._n:
            raise ValueError('the preconditioner was built for a matrix of size %d, got one of size %d' % (self._n, n))
        if np.dtype(dtype) != np.dtype(self._dtype):
            raise ValueError('the preconditioner was built for a matrix of type %s, got one of type %s'
                             % (np.dtype(self._dtype).name, np.dtype(dtype).name))
        L = self._L
        if bits is not None:
            self._checked(L.rlh_fsvalues_update_device, 'rlh_fsvalues_update_device', self._h, bits, *pointers)
        else:
            self._checked(L.rlh_fsvalues_update, 'rlh_fsvalues_update', self._h, *pointers)
        if self._plan:
            _lib.check(L.rlh_fsvalues_plan(self._plan, self._h))
        updates, sec = ctypes.c_int64(), ctypes.c_double()
        _lib.check(L.rlh_fsvalues_info(self._h, ctypes.byref(updates), ctypes.byref(sec)))
        self.updates, self.update_seconds = int(updates.value), float(sec.value)

    def size(self):
        return self._n

    def data_type(self):
        return np.dtype(self._dtype)

    def device_bytes(self):
        """Device memory held: G, G^H, their partitions and the workspaces; with `work`, the plan's layouts and its W too."""
        nb, more = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(self._L.rlh_fsai_info(self._h, None, None, None, None, ctypes.byref(nb), None))
        if self._plan:
            _lib.check(self._L.rlh_fsapply_info(self._plan, None, None, None, ctypes.byref(more)))
        return int(nb.value) + int(more.value)

    def csr(self):
        """G as a SciPy CSR matrix (one copy to the host: rlh_fsai_get)."""
        import scipy.sparse as scs
        ip = np.zeros(self._n + 1, dtype=np.int64)
        ix = np.zeros(max(self.nnz, 1), dtype=np.int32)
        va = np.zeros(max(self.nnz, 1), dtype=self._dtype)
        _lib.check(self._L.rlh_fsai_get(self._h, _lib.host_ptr(ip), _lib.host_ptr(ix), _lib.host_ptr(va)))
        return scs.csr_matrix((va[:self.nnz], ix[:self.nnz], ip), shape=(self._n, self._n))

    def algorithmic_bytes(self, m):
        """Entries of G and of G^H (value + 4-byte column index) + one read and one write of a block per product."""
        es = np.dtype(self._dtype).itemsize
        if self.work is None:
            return 2 * self.nnz * (es + 4) + 4 * self._n * m * es
        # with a plan: entries at 4 + sizeof V, x read and y written in the matrix type, W written and read in its own
        ev, ew = work_element_bytes(self.work, self._dtype)
        return 2 * self.nnz * (ev + 4) + self._n * m * (2 * es + 2 * ew)

    def apply(self, x, y):
        """y = G^H (G x) for Vectors windows of equal size (y may be x)."""
        if hasattr(x, 'comm') or hasattr(y, 'comm'):
            raise ValueError('ApproximateInverse does not take row-sharded blocks')
        m = x.nvec()
        if m != y.nvec():
            raise ValueError('Numbers of input and output vectors differ')
        if x.data_type() != self._dtype or y.data_type() != self._dtype:
            raise ValueError('Matrix and vectors data types differ')
        if x.dimension() != self._n or y.dimension() != self._n:
            raise ValueError('Matrix and vectors dimensions incompatible')
        if self._plan:
            _lib.check(self._L.rlh_fsapply_run(self._plan, m, x.data_ptr(), x.ld(), y.data_ptr(), y.ld()))
        else:
            _lib.check(self._L.rlh_fsai_apply(self._h, m, x.data_ptr(), x.ld(), y.data_ptr(), y.ld()))


def gershgorin_upper_bound(matrix):
    """max_i sum_j |a_ij| >= lambda_max for a symmetric / Hermitian matrix (SciPy sparse)."""
    a = abs(matrix)
    return float(np.max(np.asarray(a.sum(axis=1)).ravel()))


class ChebyshevPreconditioner:

    def __init__(self, op, hi, ratio=50.0, degree=6, low_precision_op=None, storage=None):
        """op: operator with apply(x, y); hi: upper bound of its spectrum; the polynomial
        approximates 1/x on [hi / ratio, hi]; degree: number of operator applications.

        low_precision_op: the same operator in float32 / complex64.  When given, the polynomial
        is evaluated in that precision (half the bytes through the gather-bound SpMM); the input
        and the result are converted on the device.  A preconditioner only has to be a fixed,
        (nearly) symmetric positive definite approximation of A^-1, which single precision is."""
        if degree < 1:
            raise ValueError('degree must be at least 1')
        if storage not in (None, 'bf16'):
            raise ValueError("storage must be None or 'bf16'")
        # storage='bf16' (with a float32 low_precision_op in the 1024-row windowed or the 256-row
        # interleaved device layout -- the latter is what an operator built from a GPU tensor, rows
        # of more than 8 entries, FE matrices and bands get): the three work blocks are kept in
        # bfloat16, arithmetic stays float32 -- half the bytes again per step; on lap3d 64^3
        # (degree 24) the iteration count goes from 27 to 28.  Ignored (float32 storage) where the
        # operator cannot do it (supports_bf16() false: sliced layout, float64, complex).
        self._bf16 = storage == 'bf16'
        self._work16 = None
        self._op = op if low_precision_op is None else low_precision_op
        self._low = low_precision_op is not None
        self._lo, self._hi = float(hi) / float(ratio), float(hi)
        self._degree = int(degree)
        self._work = None

    def apply(self, x, y):
        """y = p(A) x by the three-term Chebyshev semi-iteration for A u = x from u_0 = 0:
        u_1 = x / theta,  u_{k+1} = u_k + rho_k rho_{k-1} (u_k - u_{k-1}) + (2 rho_k / delta) (x - A u_k).
        u_{k+1} overwrites u_{k-1} (only its own row is needed), so two blocks ping-pong and a
        fused step reads u_k, u_{k-1}, x and writes u_{k+1} (`cheb_step`)."""
        m = x.nvec()
        if self._bf16 and self._low and not x.is_complex() and getattr(self._op, 'supports_bf16', lambda: False)():
            try:
                self._apply_bf16(x, y, m)
                return
            except _lib.RlhError as e:
                # An unsharded operator whose layout the 2-byte staging cannot take after all: the same polynomial on
                # float32 work blocks.  On a row-sharded operator the error is final: supports_bf16() above is agreed on
                # by all ranks BEFORE any exchange is posted, and a rank falling back alone would break the exchange.
                if 'rlh_spmm_cheb_bf16' not in str(e) or hasattr(x, 'comm'):
                    raise
                import warnings
                warnings.warn('bfloat16 work blocks refused by the operator (%s): float32 work blocks instead' % e)
                self._bf16 = False
        nwork = 3 if self._low else 2
        # (capacity = shape()[0]: nvec() is the current selection and shrinks with the solver's block)
        if self._work is None or self._work[0].shape()[0] < m or self._work[0].dimension() != x.dimension():
            dt = None
            if self._low:
                dt = np.complex64 if x.is_complex() else np.float32
            self._work = [x.new_vectors(m, data_type=dt) for _ in range(nwork)]
        for v in self._work:
            v.select(m)
        if self._low:
            b, ua, ub = self._work
            x.convert_to(b)
        else:
            b = x
            # the last step must land in y: with an even number of steps u_1 starts in y
            steps = self._degree - 1
            ua, ub = (y, self._work[0]) if steps % 2 == 0 else (self._work[0], y)
            t = self._work[1]
        theta, delta = 0.5 * (self._hi + self._lo), 0.5 * (self._hi - self._lo)
        sigma1 = theta / delta
        rho = 1.0 / sigma1
        fused = hasattr(self._op, 'cheb_step')
        if not fused and self._low:
            raise ValueError('low-precision evaluation needs an operator with cheb_step')
        ua.lincomb(1.0 / theta, b, 0.0, b)          # u_1 = x / theta
        if self._degree > 1:
            ub.zero()                               # u_0 = 0 (a defined value: 0 * garbage could be NaN)
        for _ in range(self._degree - 1):
            rho_new = 1.0 / (2.0 * sigma1 - rho)
            c, cb = rho_new * rho, 2.0 * rho_new / delta
            if fused:       # ub = (1 + c) ua - c ub + cb (b - A ua) in one pass: u_{k+1} over u_{k-1}
                self._op.cheb_step(ua, ub, b, 1.0 + c, -c, cb)
            else:
                self._op.apply(ua, t)               # t = A u_k
                t.lincomb(-cb, t, cb, b)            # t = cb (b - A u_k)
                ub.lincomb(-c, ub, 1.0, t)
                ub.add(ua, 1.0 + c)
            ua, ub = ub, ua
            rho = rho_new
        if self._low:
            ua.convert_to(y)

    def _apply_bf16(self, x, y, m):
        from .sparse import Bf16Block
        n = x._vdim                                 # local rows (a row shard packs its own part)
        if self._work16 is None or self._work16[0].m < m or self._work16[0].n != n:
            self._work16 = [Bf16Block(n, m) for _ in range(3)]
        b, ua, ub = self._work16
        theta, delta = 0.5 * (self._hi + self._lo), 0.5 * (self._hi - self._lo)
        sigma1 = theta / delta
        rho = 1.0 / sigma1
        b.pack(x, 1.0)
        ua.pack(x, 1.0 / theta)                     # u_1 = x / theta
        if self._degree > 1:
            ub.zero(m)                              # u_0 = 0
        for _ in range(self._degree - 1):
            rho_new = 1.0 / (2.0 * sigma1 - rho)
            c, cb = rho_new * rho, 2.0 * rho_new / delta
            self._op.cheb_step_bf16(m, ua, ub, b, 1.0 + c, -c, cb)
            ua, ub = ub, ua
            rho = rho_new
        ua.unpack(y)
        self._work16 = [b, ua, ub]
