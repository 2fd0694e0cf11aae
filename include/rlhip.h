/*
 * rlhip.h -- C ABI of librlhip.so, the MI355X (gfx950) abstract-vectors backend
 * for the RALEIGH block-JCG eigensolver.
 *
 * This is the drop-in boundary: the entry points a ctypes binding of the
 * reference would call in place of libcudart / libcublas / libcusolver
 * (raleigh/algebra/cuda_wrap.py, cublas_wrap.py) and libmkl_rt
 * (raleigh/algebra/mkl_wrap.py).  Every entry point cites the reference
 * interface it replaces (paths relative to the reference tree).
 *
 * Conventions
 *  - A block of vectors is a column-major n x m matrix in device memory with
 *    leading dimension ld (in ELEMENTS, ld >= n): vector j starts at
 *    base + j*ld.  This is the reference's (nvec, dim) C-ordered array
 *    (dense_ndarray.py:52-83, dense_cublas.py:355-428) with ld = dim; a
 *    `select(nv, first)` window is the pointer base + first*ld.
 *  - All sizes are int64_t (the reference passes c_int and overflows at 2^31).
 *  - dtype: RLH_S float, RLH_D double, RLH_C complex64, RLH_Z complex128
 *    (interleaved re,im).
 *  - Small coefficient arrays (q, s, ind) are HOST pointers, borrowed for the
 *    call only; q is addressed through element strides so C- and F-ordered
 *    numpy arrays need no copy (dense_cublas.py:283-294).
 *  - Results that feed host math are written to HOST pointers; such calls
 *    synchronise the stream before returning.  Device-only calls are
 *    asynchronous on the library stream (rlh_set_stream).
 *  - Every function returns 0 on success, non-zero on failure;
 *    rlh_last_error() gives the message (the reference raises
 *    RuntimeError('cuda error %d'), dense_cublas.py:779-781).
 *  - One calling thread per process; one device per process (one process per
 *    GPU, RCCL reductions are driven by the caller on the same stream).
 */
#ifndef RLHIP_H
#define RLHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RLH_VERSION 100

enum { RLH_S = 0, RLH_D = 1, RLH_C = 2, RLH_Z = 3 };

/* ---- context (cuda_wrap.py:139-162; cublas_wrap.py Cublas.__init__) ---- */
int rlh_version(void);
const char *rlh_last_error(void);
int rlh_device_count(int *count);
/* Binds the process to `device`, creates the stream, pinned staging ring and
 * reduction workspace.  Idempotent for the same device. */
int rlh_init(int device);
int rlh_finalize(void);
/* Use an externally owned hipStream_t (e.g. torch's current stream) so that
 * RCCL collectives issued by the caller are ordered with the kernels;
 * NULL restores the library's own stream. */
int rlh_set_stream(void *hip_stream);
int rlh_sync(void);                          /* cuda_wrap.py synchronize */
int rlh_mem_info(int64_t *free_bytes, int64_t *total_bytes);
/* Device memory the library holds for its handles and their builds (not rlh_malloc's buffers, not the context's own):
 * bytes and allocations alive now.  Valid before rlh_init (0, 0). */
int rlh_device_live(int64_t *bytes, int64_t *blocks);

/* ---- device memory (cuda_wrap.py malloc/free/memset/memcpy/memcpy2D;
 *      dense_cublas.py:801-811 _Data) ---- */
int rlh_malloc(void **dptr, int64_t bytes);
int rlh_free(void *dptr);
int rlh_memset(void *dptr, int value, int64_t bytes);            /* async */
int rlh_h2d(void *dptr, const void *hptr, int64_t bytes);        /* sync  */
int rlh_d2h(void *hptr, const void *dptr, int64_t bytes);        /* sync  */
int rlh_d2d(void *dst, const void *src, int64_t bytes);          /* async */
/* small device result -> host through the library's pinned buffer (one stream synchronisation);
 * used after an RCCL all-reduce of a Gram / dots result */
int rlh_fetch(void *hptr, const void *dptr, int64_t bytes);      /* sync  */
/* rows x width_bytes strided copy, kind: 0 h2d, 1 d2h, 2 d2d
 * (dense_cublas.py:61-68 append(axis=1); padded-ld upload/download). */
int rlh_copy2d(void *dst, int64_t dpitch, const void *src, int64_t spitch,
               int64_t width_bytes, int64_t rows, int kind);

/* ---- K1: Gram / dot (dense_numpy.py:78-82; dense_cublas.py:245-269) ----
 * out[i*mx + j] = sum_r conj(Y[r,i]) * X[r,j], i < my, j < mx
 * (shape (my, mx), C order == `X.dot(Y)` of the reference).
 * d_out: device buffer of my*mx elements or NULL (internal buffer);
 * h_out: host buffer or NULL.  With h_out the call synchronises; with d_out
 * only, it is asynchronous (the caller all-reduces d_out with RCCL, then
 * rlh_d2h).  X == Y with equal shapes is detected and read once. */
int rlh_gram(int dtype, int64_t n, int64_t mx, const void *X, int64_t ldx,
             int64_t my, const void *Y, int64_t ldy, void *d_out, void *h_out);

/* Gram of two CONCATENATED windows in one pass (the solver's back-to-back Gram
 * pairs share an operand -- solver.py:854-861 XAX + XBX, :1321-1339 ZAY + ZBY, :1376-1381
 * XBY + YBY, :1444-1447 XAY + YAY): out = [Y_0 | ... | Y_{ny-1}]^H [X_0 | ... | X_{nx-1}], shape
 * (sum my, sum mx), C order; up to 4 blocks per window, every block is read once.  X, ldx, mx,
 * Y, ldy, my: HOST arrays of nx / ny device pointers, leading dimensions and column counts.
 * d_out / h_out as rlh_gram. */
int rlh_gram_multi(int dtype, int64_t n, int nx, const void *const *X, const int64_t *ldx,
                   const int64_t *mx, int ny, const void *const *Y, const int64_t *ldy,
                   const int64_t *my, void *d_out, void *h_out);

/* ---- K2: column-wise dots (dense_numpy.py:68-76; dense_cublas.py:233-243)
 * out[i] = sum_r conj(Y[r,i]) * X[r,i], i < m.  Any m >= 0 in one call: the library walks the
 * block in column panels that one launch can index, so the rows of a tall data matrix viewed as
 * vectors (AMatrix.dots / frobenius2: m = number of rows) need nothing from the caller.  The
 * other column-wise entry points (rlh_axpy, rlh_axpy_cols, rlh_lincomb_cols, rlh_scale_cols,
 * rlh_copy, rlh_copy_cols, rlh_conj, rlh_convert, rlh_fill_random, rlh_bf16_pack / unpack,
 * rlh_gather_rows*) do the same; only rlh_gram / rlh_gram_multi, whose result is m x m, keep
 * a limit of 32768 vectors per window. */
int rlh_dots(int dtype, int64_t n, int64_t m, const void *X, int64_t ldx,
             const void *Y, int64_t ldy, void *d_out, void *h_out);

/* ---- K2t: transposed dots (dense_numpy.py:55-66; dense_cublas.py:175-221)
 * d_out[r] = sum_i conj(Y[r,i]) * X[r,i], r < n; device output of n elements. */
int rlh_dots_transp(int dtype, int64_t n, int64_t m, const void *X, int64_t ldx,
                    const void *Y, int64_t ldy, void *d_out);
/* Largest modulus of the real / imaginary parts of the entries of a block (AMatrix.scale():
 * the reference scans the host array, raleigh/algebra/dense_matrix.py:44-49); *h_out is a host
 * double; the call synchronises.  Any m >= 0 in one call (column panels, as rlh_dots). */
int rlh_absmax(int dtype, int64_t n, int64_t m, const void *X, int64_t ldx, double *h_out);

/* ---- K3/K4: block update (dense_numpy.py:84-105; dense_cublas.py:271-342)
 * Out[:,j] = beta*Out[:,j] + alpha * sum_{i<k} q[i,j] * X[:,i], j < m.
 * q: HOST, element (i,j) at q[i*q_rs + j*q_cs]; alpha: HOST, 2 doubles (re,im);
 * beta is 0 (multiply) or 1 (add).  Out must not overlap X. */
int rlh_block_update(int dtype, int64_t n, int64_t k, const void *X, int64_t ldx,
                     int64_t m, void *Out, int64_t ldo, const void *q,
                     int64_t q_rs, int64_t q_cs, const double *alpha, int beta);

/* ---- fused forms used by this repository's driver; the reference issues the
 *      same arithmetic as multiply + add (solver.py:1609-1656) and copy + add (solver.py:942-952).
 * rlh_block_update2: Out[:,j] = beta*Out[:,j] + alpha*(sum_i q1[i,j] X1[:,i] + sum_i q2[i,j] X2[:,i])
 * in one pass over X1 and X2.
 * rlh_lincomb_cols: Out[:,i] = a[i]*A[:,i] + b[i]*B[:,i]; a, b HOST arrays of the vectors' dtype;
 * Out may alias A or B. */
int rlh_block_update2(int dtype, int64_t n, int64_t k1, const void *X1, int64_t ldx1,
                      const void *q1, int64_t q1_rs, int64_t q1_cs, int64_t k2,
                      const void *X2, int64_t ldx2, const void *q2, int64_t q2_rs,
                      int64_t q2_cs, int64_t m, void *Out, int64_t ldo,
                      const double *alpha, int beta);
/* Two result blocks from ONE pass over the two sources (the Rayleigh-Ritz update forms the new
 * X and the new search directions Z from the same X, Y -- solver.py:1609-1656 issues a
 * multiply + add pair for each):  [OutA | OutB] = X1 * q1 + X2 * q2,  q1: k1 x (ma + mb),
 * q2: k2 x (ma + mb) host matrices (element strides as above), the first ma result columns go
 * to OutA, the other mb to OutB. */
int rlh_block_update2x2(int dtype, int64_t n, int64_t k1, const void *X1, int64_t ldx1,
                        const void *q1, int64_t q1_rs, int64_t q1_cs, int64_t k2, const void *X2,
                        int64_t ldx2, const void *q2, int64_t q2_rs, int64_t q2_cs, int64_t ma,
                        void *OutA, int64_t ldoa, int64_t mb, void *OutB, int64_t ldob);
int rlh_lincomb_cols(int dtype, int64_t n, int64_t m, const void *a, const void *A,
                     int64_t lda, const void *b, const void *B, int64_t ldb, void *Out,
                     int64_t ldo);

/* ---- K5: Y += alpha * X on an n x m window (dense_cublas.py:311-316) ---- */
int rlh_axpy(int dtype, int64_t n, int64_t m, const double *alpha,
             const void *X, int64_t ldx, void *Y, int64_t ldy);
/* ---- K6: Y[:,i] += s[i] * X[:,i]; s HOST, vectors' dtype
 *      (dense_cublas.py:343-350) ---- */
int rlh_axpy_cols(int dtype, int64_t n, int64_t m, const void *s,
                  const void *X, int64_t ldx, void *Y, int64_t ldy);
/* ---- K7: window copy / column gather (dense_cublas.py:133-153)
 * rlh_copy: Y[:, j] = X[:, j], j < m.
 * rlh_copy_cols: Y[:, k] = Xall[:, ind[k]], k < m; ind HOST int64, absolute
 * indices into the storage Xall points at. */
int rlh_copy(int dtype, int64_t n, int64_t m, const void *X, int64_t ldx,
             void *Y, int64_t ldy);
int rlh_copy_cols(int dtype, int64_t n, int64_t m, const int64_t *ind,
                  const void *Xall, int64_t ldx, void *Y, int64_t ldy);
/* ---- K8: column scale (dense_numpy.py:44-52; dense_cublas.py:155-172)
 * s HOST doubles (re,im pairs when the dtype is complex).
 * mode 1: X[:,i] *= s[i]; mode 0: X[:,i] /= s[i] unless s[i] == 0. */
int rlh_scale_cols(int dtype, int64_t n, int64_t m, const double *s, int mode,
                   void *X, int64_t ldx);
/* precision conversion Y = (dst type) X between s<->d or c<->z blocks (mixed-precision
 * preconditioning; not in the reference) */
int rlh_convert(int src_dtype, int dst_dtype, int64_t n, int64_t m, const void *X,
                int64_t ldx, void *Y, int64_t ldy);
/* Vectors.fill_random for large blocks (dense_cublas.py:119-131 draws numpy.random.rand on the
 * host and uploads: 0.6 s for 10^7 x 20): X[i, j] = uniform in [-1, 1), a pure function of
 * (seed, col0 + j, row0 + i) -- splitmix64 of the counter, restated in oracle/ops.py
 * uniform_block -- so row shards generate their rows of one global block; imaginary parts 0. */
int rlh_fill_random(int dtype, int64_t n, int64_t m, void *X, int64_t ldx, uint64_t seed,
                    int64_t row0, int64_t col0);
/* in-place complex conjugate (dense_cublas.py:503-511); no-op for real */
int rlh_conj(int dtype, int64_t n, int64_t m, void *X, int64_t ldx);

/* ---- K13: sparse symmetric/Hermitian operator
 *      (sparse_mkl.py:16-48; mkl_wrap.py:204-276 mkl_?csrmm 'SUNF'/'HUNF')
 * The caller passes the FULL matrix (both triangles) as 0-based CSR in host
 * memory; rows [row0, row0+n_rows) of a matrix with n_cols columns (row-shard
 * of the operator).  The library converts to one of three device layouts
 * (rlh_csr_layout).
 * Y[:, j] = A * X[:, j]; X has n_cols rows, Y has n_rows rows. */
typedef struct rlh_csr *rlh_csr_t;
int rlh_csr_create(rlh_csr_t *h, int dtype, int64_t n_rows, int64_t n_cols,
                   const int64_t *indptr, const int32_t *indices,
                   const void *values);
/* The Hermitian operator defined by the UPPER triangle of a square 0-based CSR matrix with sorted rows, as the
 * reference hands it to mkl_?csrmm with the 'SUNF' / 'HUNF' descriptor (mkl_wrap.py:211-276: A = U + U^H - diag(U));
 * entries below the diagonal, if stored, are ignored.  Single-GPU operator (n_own = n). */
int rlh_csr_create_upper(rlh_csr_t *h, int dtype, int64_t n, const int64_t *indptr,
                         const int32_t *indices, const void *values);
/* The operator from a FULL 0-based CSR matrix that already lies in DEVICE memory (`index_bits` 32 or 64: the type
 * of both index arrays), built by kernels on the library stream: no entry, index or value visits the host.  The
 * input must be canonical -- indptr[0] == 0, indptr non-decreasing, its last entry the number of stored entries,
 * columns inside [0, n_cols) and strictly ascending within each row -- and is checked on the device first: a
 * violation returns non-zero, a message that names the first offending row and a null handle.  mirror_upper = 1
 * (square matrices): the Hermitian operator defined by the upper triangle, as rlh_csr_create_upper defines it -- an
 * entry (i, j), j < i, takes the conjugate of the stored (j, i).  The stored STRUCTURE must be symmetric: an entry
 * without its partner on the other side is an error that names its row and column (the device build creates no
 * entries).  The caller's arrays are never written and are not referenced after the call returns.  The result is
 * an ordinary handle in the interleaved layout (2) or, where that one does not qualify, sliced ELL (0); the
 * 1024-row windowed layout (1) is built from host arrays only: RLH_SPMM_FORMAT=sell|wide act as at rlh_csr_create,
 * =well is an error here. */
int rlh_csr_create_device(rlh_csr_t *h, int dtype, int64_t n_rows, int64_t n_cols, int index_bits,
                          const void *d_indptr, const void *d_indices, const void *d_values, int mirror_upper);
int rlh_csr_destroy(rlh_csr_t h);
int rlh_csr_info(rlh_csr_t h, int64_t *n_rows, int64_t *n_cols, int64_t *nnz,
                 int64_t *device_bytes);
/* Device layout the library chose for the handle (diagnostic): *layout = 0 sliced ELL
 * (one gather per stored entry and vector: no column locality), 1 windowed ELL (rows of at most
 * 8 entries of a real type: the column windows of every 1024-row block are staged through the
 * LDS, the row's entries stay in registers), 2 interleaved windowed layout (any row length, any
 * type: 256-row blocks, LDS image [column][vector], entries streamed in chunks of 8);
 * *stored = entry slots incl. padding; *staged_per_slot = staged vector elements per entry
 * slot (windowed-layout analysis; 0 if it was not run).  RLH_SPMM_FORMAT=sell|well|wide in the
 * environment of rlh_csr_create overrides the choice. */
int rlh_csr_layout(rlh_csr_t h, int *layout, int64_t *stored, double *staged_per_slot);
/* Stacked row blocks of the windowed layout (diagnostic): *stacks = workgroup-sized stacks of two 1024-row blocks whose
 * column windows overlap (0: the layout was not built: no windowed layout, or stacking stages less than 10 % fewer
 * elements); *staged_per_row / *staged_per_row_stacked = vector elements staged per row and vector without / with the
 * stacks (3.42 / 2.42 for the 7-point stencil on 215^3).  rlh_spmm on the whole operator uses the stacks when they exist;
 * RLH_SPMM_STACK=0 in the environment (create or call time) turns them off, =2 at create time builds them regardless. */
int rlh_csr_stacks(rlh_csr_t h, int64_t *stacks, double *staged_per_row, double *staged_per_row_stacked);
/* Whether rlh_spmm_cheb_bf16_part would take this operator: *ok = 1 if it is a float32 operator in the 256-row interleaved
 * layout (built on the host or by rlh_csr_create_device; any shape: groups that reach past the last column are staged
 * element by element) or in the 1024-row windowed layout with every staging group inside the column range, and -- with a
 * halo block (n_own < the column count: a row shard) of leading dimension ldh -- n_own and ldh are multiples of 8 and the
 * groups start on multiples of 8 columns, so that the 2-byte staging stays on 16-byte pieces.  0 for the sliced layout and
 * for every other element type.  The layout conditions depend on the SHARD, so ranks of one row-sharded
 * operator can differ: callers agree on the answer (all-reduce MIN) BEFORE the first halo exchange of a bfloat16 step,
 * never by catching the launch's error afterwards. */
int rlh_csr_bf16_ready(rlh_csr_t h, int64_t n_own, int64_t ldh, int *ok);
/* Columns [0, n_own) are read from X, columns [n_own, n_cols) from the halo block
 * H (row c - n_own), which holds the off-shard rows received from other ranks;
 * single GPU: n_own = n_cols, H = NULL.  A row with at least one stored entry reads only the columns it stores (the
 * layouts' padding slots point at the row's own first column), so a non-finite element of X reaches only the rows that
 * reference it.  A row without entries is +0 for finite X; its padding points at the first column its block stages
 * (column 0 in the sliced layout), and the row is NaN where that element is not finite. */
int rlh_spmm(rlh_csr_t h, int64_t m, const void *X, int64_t ldx, int64_t n_own,
             const void *H, int64_t ldh, void *Y, int64_t ldy);
/* One step of the Chebyshev semi-iteration (three-term form) fused with the operator
 * application (device polynomial preconditioner): per row and vector
 *   P = cy*Y + cp*P + cb*(B - A*Y)
 * in one pass: Y = y_k (gathered, read only), P = y_{k-1} on entry and y_{k+1} on return
 * (updated in place), B the right-hand side.  A square in the own rows; P distinct from Y, B. */
int rlh_spmm_cheb(rlh_csr_t h, int64_t m, const void *Y, int64_t ldy, int64_t n_own,
                  const void *H, int64_t ldh, void *P, int64_t ldp, const void *B, int64_t ldb,
                  double cy, double cp, double cb);
/* The same two operations on a part of the rows, so that a row shard can overlap its halo
 * exchange with the rows that do not need it: part 1 = the rows whose entries all lie in columns
 * < n_own (H is not read and may still be in flight), part 2 = the other rows, part 0 = all.
 * Parts 1 and 2 together write every row exactly once.  (Granularity: the layout's 1024-row blocks;
 * with the sliced layout part 1 is empty and part 2 is everything.) */
int rlh_spmm_part(rlh_csr_t h, int part, int64_t m, const void *X, int64_t ldx, int64_t n_own,
                  const void *H, int64_t ldh, void *Y, int64_t ldy);
int rlh_spmm_cheb_part(rlh_csr_t h, int part, int64_t m, const void *Y, int64_t ldy, int64_t n_own,
                       const void *H, int64_t ldh, void *P, int64_t ldp, const void *B, int64_t ldb,
                       double cy, double cp, double cb);
/* What the last rlh_spmm* / rlh_spmm_cheb* call of the process launched (diagnostic; the tests' way of knowing which
 * kernel ran), as text in buf[0 .. len): the kernel and its template parameters, the grid and the schedule length --
 *   sell jt=J tt=T tpb=W cheb=0|1       sliced ELL             well epl=E cheb=0|1               1024-row windowed
 *   stack reg                           stacks, register-staged stack dma pat|vals dtab|idx cheb=0|1   stacks, LDS-DMA ring
 *   wide nv=N vs=V k=K vec|elem cheb=0|1                       256-row interleaved
 *   well bf16 / stack bf16 vps=V pat|vals dtab|idx / wide bf16 nv=N vs=V k=K vec|elem     the bfloat16 step
 * followed by " grid=G len=L" -- or "none" when the call had nothing to launch (m = 0, no rows, an empty part).  The record
 * is written where the launch is made, not derived from the dispatch rules.  ONE record per process, written without
 * any synchronisation by every product call: a diagnostic for a single calling thread (the tests), not thread-safe and
 * not something to build on. */
int rlh_spmm_last_launch(char *buf, int64_t len);
/* bfloat16 storage for the device polynomial preconditioner (not in the reference).  A bf16 block
 * is a column-major array of 16-bit words, leading dimension in elements (a multiple of 8), base
 * 16-byte aligned.  pack: Y16 = bf16(scale * X) (round to nearest even) from a float32 / float64
 * block; unpack: back to float32 / float64.  rlh_spmm_cheb_bf16 is rlh_spmm_cheb on three bf16
 * blocks with float32 arithmetic against a square float32 operator in the 1024-row windowed layout
 * (and its stacks) or in the 256-row interleaved layout, wide_k 1 or 2 (rlh_csr_bf16_ready tells;
 * an error otherwise -- sliced layout, other types --, the caller then stays in float32): t = A y
 * accumulated in float32, p <- cy y + cp p + cb (b - t) rounded once to bfloat16 (nearest even);
 * y and b, rows from n_rows on and vectors from m on are not written. */
int rlh_bf16_pack(int src_dtype, int64_t n, int64_t m, const void *X, int64_t ldx, double scale,
                  void *Y16, int64_t ldy);
int rlh_bf16_unpack(int dst_dtype, int64_t n, int64_t m, const void *X16, int64_t ldx, void *Y,
                    int64_t ldy);
int rlh_spmm_cheb_bf16(rlh_csr_t h, int64_t m, const void *Y16, int64_t ldy, void *P16, int64_t ldp,
                       const void *B16, int64_t ldb, double cy, double cp, double cb);
/* The bfloat16 step on a row shard (n_own / H16 / part as in rlh_spmm_part; n_own and ldh multiples
 * of 8), and the row packing of its halo exchange. */
int rlh_spmm_cheb_bf16_part(rlh_csr_t h, int part, int64_t m, const void *Y16, int64_t ldy,
                            int64_t n_own, const void *H16, int64_t ldh, void *P16, int64_t ldp,
                            const void *B16, int64_t ldb, double cy, double cp, double cb);
int rlh_gather_rows_bf16(int64_t nidx, const int64_t *d_idx, int64_t m, const void *X16,
                         int64_t ldx, void *Out16, int64_t ldo);
/* Packs rows for the halo exchange: Out[i, j] = X[idx[i], j], i < nidx, j < m;
 * idx: DEVICE int64 (built once per operator). */
int rlh_gather_rows(int dtype, int64_t nidx, const int64_t *d_idx, int64_t m,
                    const void *X, int64_t ldx, void *Out, int64_t ldo);

/* ---- incomplete LU preconditioner on the device
 *      (sparse_mkl.py:122-140 IncompleteLU -> mkl_wrap.py:279-347: mkl dcsrilut once, then two
 *      mkl_dcsrtrsv per VECTOR on the host)
 * rlh_ilut_factor: dual-threshold ILUT(p = maxfil, tau = tol) of the FULL matrix given as 0-based
 * CSR in HOST memory (dtype RLH_D or RLH_Z); runs on the host (no GPU needed): entries below
 * tol * ||row||_2 are dropped, at most maxfil entries are kept in the L part and in the U part of
 * every row (mkl_wrap.py:305-331: tol, max_fill_rel * nnz / n).  The factors are read back as CSR
 * with rlh_factors_get: which = 0 -> L strictly lower (unit diagonal implied), 1 -> U upper
 * including the diagonal (diagonal first in every row, then ascending columns). */
typedef struct rlh_factors *rlh_factors_t;
int rlh_ilut_factor(rlh_factors_t *f, int dtype, int64_t n, const int64_t *indptr,
                    const int32_t *indices, const void *values, double tol, int64_t maxfil);
int rlh_factors_nnz(rlh_factors_t f, int64_t *nnz_l, int64_t *nnz_u);
int rlh_factors_get(rlh_factors_t f, int which, int64_t *indptr, int32_t *indices, void *values);
int rlh_factors_destroy(rlh_factors_t f);
/* Sparse triangular operator for blocks of vectors (mkl_wrap.py:333-347 mkl_dcsrtrsv 'L','N','U'
 * and 'U','N','N').  The triangular factor is given as 0-based CSR in HOST memory (the diagonal
 * stored unless unit_diag); rows are grouped into dependency levels at creation.
 * rlh_sptrsv_solve_chain: X = op[nops-1]^-1 ... op[0]^-1 B for column-major n x m blocks (B may be
 * X); d_perm_in / d_perm_out: DEVICE int64 arrays or NULL -- row r of the internal scratch is row
 * d_perm_in[r] of B, and is written to row d_perm_out[r] of X (row / column permutations of a
 * factorisation P_r A P_c = L U).  Asynchronous on the library stream. */
typedef struct rlh_sptrsv *rlh_sptrsv_t;
int rlh_sptrsv_create(rlh_sptrsv_t *t, int dtype, int64_t n, const int64_t *indptr,
                      const int32_t *indices, const void *values, int lower, int unit_diag);
int rlh_sptrsv_info(rlh_sptrsv_t t, int64_t *nnz, int64_t *levels, int64_t *device_bytes);
int rlh_sptrsv_solve_chain(int nops, const rlh_sptrsv_t *ops, const int64_t *d_perm_in,
                           const int64_t *d_perm_out, int64_t m, const void *B, int64_t ldb,
                           void *X, int64_t ldx);
int rlh_sptrsv_destroy(rlh_sptrsv_t t);

/* ---- symmetric indefinite factorisation for the direct shift-invert operator
 *      (sparse_mkl.py:51-119 SparseSymmetricSolver -> mkl_wrap.py:354-489 class ParDiSo: PARDISO
 *      mtype -2 / -4 (2 / 4 when pos_def), phases 11 / 22 / 33, inertia from iparm[21], iparm[22])
 * rlh_ldlt_factor: P A P^T = L D L^H of a real symmetric / Hermitian matrix given by its UPPER
 * triangle (entries below the diagonal are ignored) as 0-based CSR in HOST memory (dtype RLH_D or
 * RLH_Z); runs on the host (no GPU needed).  perm: NULL -> own minimum-degree ordering, else
 * perm[new] = old.  D has 1 x 1 and 2 x 2 blocks chosen by threshold partial pivoting among the
 * fully summed variables of a front (pivot_threshold u in [0, 0.5]: 0.01 is the usual choice, 0
 * = no pivoting, for positive definite matrices); variables with no acceptable pivot are delayed
 * to the parent front.  perturb: a pivot below perturb * (largest entry of A in its column) is
 * taken for zero: such a pivot is replaced and counted (info[3]) -- the matrix is numerically
 * singular.
 * rlh_ldlt_info: info[0] entries of L, [1] negative and [2] positive eigenvalues of D (the
 * inertia of A), [3] perturbed pivots, [4] 2 x 2 pivots, [5] delayed pivots, [6] largest front,
 * [7] supernodes, [8] multiply-adds (estimate), [9] pivots forced at a root.
 * rlh_ldlt_get: L strictly lower (unit diagonal implied) as CSR in PIVOT order; diag[k] = D[k, k];
 * subdiag[k] = D[k + 1, k] where block[k] == 1 (first row of a 2 x 2 pivot; block 2 = second row,
 * 0 = 1 x 1 pivot); order[k] = the row of A eliminated k-th, so that with c[k] = b[order[k]]
 * the solution of A x = b is x[order[k]] = (L^-H D^-1 L^-1 c)[k].  Any pointer may be NULL. */
#define RLH_LDLT_INFO 10
typedef struct rlh_ldlt *rlh_ldlt_t;
int rlh_ldlt_factor(rlh_ldlt_t *f, int dtype, int64_t n, const int64_t *indptr,
                    const int32_t *indices, const void *values, const int64_t *perm,
                    double pivot_threshold, double perturb);
int rlh_ldlt_info(rlh_ldlt_t f, int64_t *info);
int rlh_ldlt_get(rlh_ldlt_t f, int64_t *indptr, int32_t *indices, void *values, void *diag,
                 void *subdiag, int8_t *block, int64_t *order);
/* L^H (strictly upper, unit diagonal implied, entries conjugated, columns ascending) as CSR in pivot order: the operator
 * of the backward solve (PARDISO phase 333), which the factorisation holds anyway (it produces L by columns). */
int rlh_ldlt_get_transposed(rlh_ldlt_t f, int64_t *indptr, int32_t *indices, void *values);
int rlh_ldlt_destroy(rlh_ldlt_t f);
/* X <- D^-1 X for the block diagonal D of such a factorisation, on a column-major n x m block in
 * DEVICE memory (PARDISO phase 332): d_coef holds two entries per row (DEVICE, the block's dtype):
 * X'[i] = coef[2i] X[i] + coef[2i+1] X[i + d_shift[i]], d_shift[i] in {-1, 0, +1} (DEVICE int32). */
int rlh_bdiag_solve(int dtype, int64_t n, const void *d_coef, const int32_t *d_shift, int64_t m,
                    void *X, int64_t ldx);

/* ---- sum of a SMALL host array over the processes of one node (shared memory; host only, no GPU needed)
 *      The reductions of the hot path end on the host (solver.py:1117-1187 reads the Gram matrices as NumPy arrays):
 *      on a row-sharded run each rank fetches its partial result and the ranks add them up here -- a flag-per-rank
 *      hand-off in a POSIX shared-memory segment, the slots summed in rank order (the same bits on every rank) --
 *      instead of one RCCL launch + copy per reduction.  name: "/..." chosen by rank 0 and told to the others;
 *      rank 0 creates the segment, the others wait for it; slot_bytes = the largest array ever reduced; after all
 *      ranks hold a handle rank 0 may remove the name (rlh_shm_unlink: the mappings live on).  dtype: RLH_S or RLH_D
 *      (complex data as pairs).  All ranks must make the same sequence of calls.  A rank that waits longer than
 *      RLH_SHM_TIMEOUT seconds (300) for another gets an error. */
typedef struct rlh_shm *rlh_shm_t;
int rlh_shm_create(rlh_shm_t *s, const char *name, int rank, int nranks, int64_t slot_bytes);
int rlh_shm_unlink(const char *name);
int rlh_shm_allreduce(rlh_shm_t s, int dtype, int64_t count, void *inout);
int rlh_shm_destroy(rlh_shm_t s);

/* ---- K12: dense operator (dense_numpy.py:153-175; dense_cublas.py:732-776)
 * A: DEVICE, M x N, row-major (order 0, numpy C_CONTIGUOUS, lda >= N) or
 * column-major (order 1, F_CONTIGUOUS, lda >= M).
 * transp 0: Y[:, j] = A   * X[:, j]   (X: N rows, Y: M rows)
 * transp 1: Y[:, j] = A^H * X[:, j]   (X: M rows, Y: N rows)
 * What is read.  A as stored is R lines of len elements, lda apart (row-major: R = M, len = N; column-major: R = N,
 * len = M).  The library reads (R - 1) * lda + len elements from A, where the matrix-core kernels (A and X 16-byte
 * aligned, lda and ldx multiples of 16 bytes) round len up to a multiple of 16 bytes, never beyond lda; of a vector of
 * X likewise its rows rounded up to 16 bytes, never beyond ldx.  What is read past len reaches no result.  So A may be a
 * window of a wider parent (A + j0 with the parent's lda): with j0 * element size a multiple of 16 bytes the rounded
 * window ends inside the parent's line, because j0, lda and the rounded len are all multiples of the 16-byte unit. */
int rlh_dense_apply(int dtype, int64_t M, int64_t N, const void *A, int64_t lda,
                    int order, int transp, int64_t m, const void *X,
                    int64_t ldx, void *Y, int64_t ldy);

/* The same product with a rank-one correction folded into its epilogue (no further pass over Y):
 *   Y[:, j] = Op(A) X[:, j] - c[j] * u,   u, c DEVICE arrays (u of the output dimension, NULL = a
 * vector of ones; c of m coefficients; both NULL = rlh_dense_apply).  This is how the mean shift
 * of the PCA operator A_s = A - e a^T is applied (raleigh/interfaces/partial_svd.py:258-291 removes
 * it from the intermediate block with two dot + add passes per product): c is produced on the
 * device by rlh_gram / rlh_dots with d_out, so one operator application is two GEMMs and two small
 * reductions with no host synchronisation. */
int rlh_dense_apply_r1(int dtype, int64_t M, int64_t N, const void *A, int64_t lda, int order,
                       int transp, int64_t m, const void *X, int64_t ldx, void *Y, int64_t ldy,
                       const void *d_u, const void *d_c);

/* ---- general (rectangular) sparse data matrix: the operator of truncated SVD and PCA on sparse data
 *      (the reference's interfaces take dense arrays only; raleigh/examples/truncated_svd.py:63-72 compares
 *      against scipy's svds on the host)
 * A: M x N, 0-based CSR in HOST memory (indptr: M + 1 int64, indices: int32 column indices, values of the
 * dtype), duplicates summed; the order of the entries within a row does not matter.  rlh_spd_create copies
 * A to the device and builds a CSR copy of A^H once (values conjugated, each row in ascending order of A's
 * row index; on the host threads, RLH_HOST_THREADS), so that both products run on one row-parallel kernel
 * with the work split by nonzeros (long rows of A and of A^H are shared among several wave subgroups and
 * their partial sums combined in a fixed order: results are bit-identical from call to call and between
 * handles of the same matrix).  Needs rlh_init; M, N < 2^31.
 * rlh_spd_apply:  Y[:, j] = Op(A) X[:, j] - c[j] u,  Op(A) = A (transp 0: X has N rows, Y M rows) or A^H
 * (transp 1: X has M rows, Y N rows); X, Y column-major DEVICE blocks of m vectors; u, c DEVICE arrays with
 * the meaning of rlh_dense_apply_r1 (u NULL: a vector of ones; u and c NULL: the plain product).  The
 * handle owns a workspace (the block interleaved by rows, the result by rows, the partial sums) that grows
 * when a wider block than before is applied (that call synchronises the stream once); otherwise the call is
 * asynchronous on the library stream and allocates nothing.
 * rlh_spd_info: sizes, stored entries, device bytes held (both CSR copies, the partition, the workspace).
 * rlh_spd_stats: workspace bytes and the seconds taken by the transpose at creation. */
typedef struct rlh_spd *rlh_spd_t;
int rlh_spd_create(rlh_spd_t *h, int dtype, int64_t n_rows, int64_t n_cols, const int64_t *indptr,
                   const int32_t *indices, const void *values);
/* The same operator from CSR arrays that already lie in DEVICE memory (`index_bits` 32 or 64: the type of both
 * index arrays).  The input must be canonical -- indptr[0] == 0, indptr non-decreasing, its last entry the
 * number of stored entries, columns inside [0, N) and strictly ascending within each row -- and is checked on
 * the device before anything is built: a violation returns non-zero, a message that names it and a null handle
 * (the last entry is held against what the allocations of the index and value arrays can hold, where the
 * runtime knows them).  The handle's arrays are exactly those rlh_spd_create makes for the same matrix, built
 * by kernels on the library stream (no floating-point atomics; integer atomics only for counts); the caller's
 * arrays are copied, never written and not needed after the call.  One 16-byte status record is all that goes
 * to the host.  rlh_spd_stats then reports the device time of the transpose.  RLH_SPD_TABLE_BYTES (read at
 * creation, default 512 MB) caps the table of places of the transpose. */
int rlh_spd_create_device(rlh_spd_t *h, int dtype, int64_t n_rows, int64_t n_cols, int index_bits,
                          const void *d_indptr, const void *d_indices, const void *d_values);
/* the sums of the squared moduli of the M rows as M HOST doubles (float64 accumulation in entry order) and
 * the largest |re| / |im| of the entries as a HOST double, from the device copy; both calls synchronise */
int rlh_spd_row_sumsq(rlh_spd_t h, double *h_out);
int rlh_spd_absmax(rlh_spd_t h, double *h_out);
int rlh_spd_destroy(rlh_spd_t h);
int rlh_spd_info(rlh_spd_t h, int64_t *n_rows, int64_t *n_cols, int64_t *nnz, int64_t *device_bytes);
int rlh_spd_stats(rlh_spd_t h, int64_t *workspace_bytes, double *transpose_seconds);
int rlh_spd_apply(rlh_spd_t h, int transp, int64_t m, const void *X, int64_t ldx, void *Y, int64_t ldy,
                  const void *d_u, const void *d_c);

/* ---- dense 8-bit data matrix: the operator of PCA and truncated SVD on uint8 / int8 data (images)
 *      (the reference's dense path takes the data as float32 and runs one gemm per application,
 *      raleigh/algebra/dense_cublas.py:732-776; here the data stay bytes and the products run on the bfloat16
 *      matrix cores with float32 vectors: every 8-bit integer is exactly a bfloat16, every float32 is exactly the
 *      sum of three bfloat16 numbers and their products are exact in float32, so the only error is that of
 *      the float32 accumulation)
 * rlh_bytes_create: A is M x N, row-major in HOST memory, `kind` RLH_BYTES_U8 or RLH_BYTES_I8, `row_stride` bytes
 * from one row to the next (>= N).  The handle holds ONE device copy of A as bytes (rows padded with zeros to a
 * multiple of 16 bytes; nothing is widened on the host or the device) and the split-K workspace.  Needs rlh_init. */
#define RLH_BYTES_U8 0
#define RLH_BYTES_I8 1
typedef struct rlh_bytes *rlh_bytes_t;
/* stands for the upload of the data (Matrix.__init__, dense_cublas.py:635-700) */
int rlh_bytes_create(rlh_bytes_t *h, int kind, int64_t n_rows, int64_t n_cols, const void *h_data,
                     int64_t row_stride);
/* The same from row-major bytes that already lie in DEVICE memory.  The handle BORROWS the caller's buffer (which
 * must then outlive it and is never written) when N, row_stride and the address are all multiples of 16: every
 * 16-byte piece the kernels read then lies within the N columns of a row.  Otherwise it makes the padded copy with
 * a kernel on the library stream.  rlh_bytes_info counts only what the handle owns: the workspace alone for a
 * borrowed matrix. */
int rlh_bytes_create_device(rlh_bytes_t *h, int kind, int64_t n_rows, int64_t n_cols, const void *d_data,
                            int64_t row_stride);
int rlh_bytes_destroy(rlh_bytes_t h);
/* sizes, device bytes held (data and workspace) and the workspace bytes alone (the split-K partial tiles; it
 * grows when a product needs more than before: that call synchronises the stream once) */
int rlh_bytes_info(rlh_bytes_t h, int64_t *n_rows, int64_t *n_cols, int64_t *device_bytes,
                   int64_t *workspace_bytes);
/* Matrix.apply (dense_cublas.py:732-776): Y[:, j] = Op(A) X[:, j] - c[j] u, Op(A) = A (transp 0: X has N rows,
 * Y M rows) or A^T (transp 1: X has M rows, Y N rows); X, Y column-major float32 DEVICE blocks of m vectors with
 * any leading dimensions >= their rows; u, c DEVICE arrays with the meaning of rlh_dense_apply_r1 (u NULL: a
 * vector of ones; u and c NULL: the plain product).  Asynchronous on the library stream; no atomics: results
 * are bit-identical from call to call and between handles of the same data. */
int rlh_bytes_apply(rlh_bytes_t h, int transp, int64_t m, const void *X, int64_t ldx, void *Y, int64_t ldy,
                    const void *d_u, const void *d_c);
/* Matrix.dots (dense_cublas.py:715-718): the sums of squares of the M rows, accumulated in 64-bit integers
 * (exact), as M HOST doubles; the call synchronises. */
int rlh_bytes_row_sumsq(rlh_bytes_t h, double *h_out);
/* AMatrix.scale() (raleigh/algebra/dense_matrix.py:44-49): the largest modulus of the entries (exact), a HOST
 * double; the call synchronises. */
int rlh_bytes_absmax(rlh_bytes_t h, double *h_out);

/* ---- factorised sparse approximate inverse preconditioner T = G^H G ~ A^-1 (Kolotilina-Yeremin), built and
 *      applied on the device
 *      (the reference preconditions with MKL's ILUT, factorised and applied on the host: raleigh/algebra/
 *      mkl_wrap.py:279-347; its device counterpart here is the rlh_ilut_factor / rlh_sptrsv_* pair, whose application
 *      is bound by the dependency chain of the triangular solves.  This one is set up by independent small dense
 *      solves, one per row, and applied by two sparse products.)
 * A: Hermitian positive definite, n x n, a full 0-based canonical CSR matrix (both triangles stored, columns
 * strictly ascending within a row).  The UPPER triangle defines A: values stored below the diagonal are never read.
 * Row i of G, lower triangular, lives on P_i = the stored columns j <= i of row i -- the `max_row` (1 .. 64) largest
 * of them if there are more -- and is g = conj(y)^T / sqrt(y_k), S y = e_k, S = A[P_i, P_i], k = |P_i|: then
 * S g^H = e_k / g_kk with g_kk > 0 and G^H G is Hermitian positive definite.  The local systems are solved in
 * double / complex double for every dtype and G is rounded to the dtype once.  G is the same bits in every run,
 * for either index type and from host or device arrays.  Needs rlh_init; n < 2^31 - 1.
 * A violation returns non-zero, a message that names the entry point, what is wrong and the smallest offending row,
 * and a null handle: indptr / columns not canonical; a row that does not store its diagonal; an entry below the
 * diagonal whose partner above is not stored; a local block that is not positive definite.
 * rlh_fsai_create_device: the three arrays lie in DEVICE memory (`index_bits` 32 or 64: the type of both index
 * arrays); they are never written and not referenced after the return; nothing but status records visits the host.
 * rlh_fsai_create: the same from HOST arrays, which are uploaded and take the same path.
 * The _levels forms put row i of G on the pattern of row i of tril(A)^levels, levels in [1, 8]: with L(i) the stored
 * columns j <= i of row i, P_1(i) = L(i) and P_{l+1}(i) the union of L(j) over j in P_l(i); the row keeps the max_row
 * largest columns of P_levels(i), and truncated_rows counts the rows whose full pattern has more.  levels = 1 is what
 * the two forms above build, bit for bit.  A build takes rows of at most 8, 16, 32 and 64 kept entries on as many lanes
 * each; with RLH_FSAI_BINS=0 in the environment (read by every create call) only on 8 or 64.  G does not depend on it. */
typedef struct rlh_fsai *rlh_fsai_t;
int rlh_fsai_create_device(rlh_fsai_t *h, int dtype, int64_t n, int index_bits, const void *d_indptr,
                           const void *d_indices, const void *d_values, int max_row);
int rlh_fsai_create(rlh_fsai_t *h, int dtype, int64_t n, const int64_t *indptr, const int32_t *indices,
                    const void *values, int max_row);
int rlh_fsai_create_levels_device(rlh_fsai_t *h, int dtype, int64_t n, int index_bits, const void *d_indptr,
                                  const void *d_indices, const void *d_values, int max_row, int levels);
int rlh_fsai_create_levels(rlh_fsai_t *h, int dtype, int64_t n, const int64_t *indptr, const int32_t *indices,
                           const void *values, int max_row, int levels);
/* the levels a handle was built with */
int rlh_fsai_levels(rlh_fsai_t h, int *levels);
/* The _adaptive forms start from the level pattern above and carry out `steps` (1 .. 63) enrichment steps per row, each
 * adding up to `step_size` (1 .. 16) columns chosen by value.  One step on the pattern P of row i: with S y = e_last,
 * S = A[P, P], g = y^H (double / complex double), the candidates are the columns j < i outside P that some row p of P
 * stores (explicit zeros count; a_pj below the diagonal is conj of the stored (j, p)), r_j = sum_p g_p a_pj over p
 * ascending and score_j = |r_j|^2 / a_jj: the decrease of the Kaporin functional g A g^H from adding j alone.  The
 * candidates of the largest finite positive scores are taken, at most step_size and at most max_row - |P|, equal
 * scores the larger column first; a row stops when it holds max_row columns or a step takes nothing.  G is then
 * computed on the final pattern as by the forms above: bit for bit the plain build of A with explicit zeros on that
 * pattern and its mirror image, the same in every run, for both index widths and both settings of RLH_FSAI_BINS.
 * truncated_rows (rlh_fsai_info) counts the rows max_row held back: the level pattern was cut, the row was full before
 * one of its steps began, or a step took fewer columns than min(step_size, candidates of positive score) for lack of
 * room.  A local block that is not positive definite, at any step, fails the build and names the row. */
int rlh_fsai_create_adaptive_device(rlh_fsai_t *h, int dtype, int64_t n, int index_bits, const void *d_indptr,
                                    const void *d_indices, const void *d_values, int max_row, int levels, int steps,
                                    int step_size);
int rlh_fsai_create_adaptive(rlh_fsai_t *h, int dtype, int64_t n, const int64_t *indptr, const int32_t *indices,
                             const void *values, int max_row, int levels, int steps, int step_size);
/* the enrichment a handle was built with (0, 0: none) */
int rlh_fsai_adaptive(rlh_fsai_t h, int *steps, int *step_size);
/* ---- post-filtration by value: rlh_fsfilter_create and rlh_fsfilter_create_device make a handle of the same kind
 *      (rlh_fsai_t: every rlh_fsai_* and rlh_fsapply_* call takes it); they build G as above, drop its small entries
 *      and solve every row once more on what is left.
 * Let G0 be the G, rounded to the dtype, that the forms above build for the same max_row, levels, steps
 * and step_size (steps == 0: no enrichment, step_size is then ignored; otherwise both as for the _adaptive forms), and
 * a_jj the real diagonal of A in double.  For row i and a stored column j < i the scaled size is
 *   r_ij = |g0_ij| sqrt(a_jj) / (g0_ii sqrt(a_ii));
 * the entry is kept iff r_ij >= drop, the diagonal always.  The decision is formed without a division or a square
 * root, in double: |g0_ij|^2 * a_jj >= ((drop * drop) * (g0_ii * g0_ii)) * a_ii, with |z|^2 = fma(re, re, im * im).
 * The final row i is the row of the forms above on the kept columns: the same local solve in double / complex double
 * and the same single rounding at the store.  A principal sub-block of a positive definite block is positive definite,
 * so the second solve cannot fail where the first did not.  One pass: filter once, solve once.
 * Every decision reads row i of G0 and the diagonal of A only: nothing depends on scheduling, the filtered G is the same
 * bits in every run, for both index widths, from host or device arrays and for both settings of RLH_FSAI_BINS (rows go
 * to the bins of their NEW lengths for the second solve).  r_ij does not change under A -> D A D, D diagonal positive;
 * with every d_i a power of two the whole build is exact: equal patterns and G' = G D^-1 bit for bit.
 * drop must be finite with 0 < drop < 1.  nnz, longest_row, device_bytes, rlh_fsai_get, rlh_fsai_apply and a plan
 * made from the handle describe the filtered G; truncated_rows keeps its meaning (what max_row held back before
 * filtering); setup_seconds covers the whole build. */
int rlh_fsfilter_create_device(rlh_fsai_t *h, int dtype, int64_t n, int index_bits, const void *d_indptr,
                                    const void *d_indices, const void *d_values, int max_row, int levels, int steps,
                                    int step_size, double drop);
int rlh_fsfilter_create(rlh_fsai_t *h, int dtype, int64_t n, const int64_t *indptr, const int32_t *indices,
                             const void *values, int max_row, int levels, int steps, int step_size, double drop);
/* the threshold a handle was filtered with and the entries that removed (0, 0: a handle of the other forms) */
int rlh_fsfilter_info(rlh_fsai_t h, double *drop, int64_t *removed);
/* ---- prefiltration by value: rlh_fsthreshold_create and rlh_fsthreshold_create_device make a handle of the same kind
 *      (rlh_fsai_t: every rlh_fsai_*, rlh_fsfilter_info, rlh_fsapply_* and rlh_fsvalues_* call takes it) whose level
 *      pattern is that of the STRONG entries of A (Chow's a-priori patterns of the thresholded matrix).
 * Only the upper triangle of A is read.  For a stored entry (i, j), j < i, the partner a_ji stored in row j decides:
 * the entry is strong iff
 *   |a_ji|^2 >= (tau^2 * a_ii) * a_jj,      tau = prefilter,
 * evaluated in double on the widened values: |z|^2 = re * re + im * im (each product and the sum rounded on its own),
 * a_ii and a_jj the real parts of the stored diagonals, tau^2 = tau * tau, the right-hand side formed in exactly that
 * order with i the row; no division and no square root.  A comparison that involves a NaN is false: the entry is weak.
 * The diagonal is always a member.  In exact arithmetic the rule is |a_ij| >= tau sqrt(a_ii a_jj), which does not
 * change under A -> D A D, D diagonal positive; with every d_i a power of two the evaluation itself is exact and the
 * patterns are equal.
 * With L_tau(i) = {i} and the strong stored j < i of row i: P_1(i) = L_tau(i), P_{l+1}(i) the union of L_tau(j) over j
 * in P_l(i); after every level the pattern is cut to its max_row largest columns, as for the forms above
 * (truncated_rows, longest_row and the bins keep their meaning).  Where nothing is cut the patterns are nested in the
 * level and in tau.
 * Everything after the pattern is that of the forms above, on the FULL matrix: the local block is S = A[P, P] with all
 * its stored entries, weak ones included (they shape the pattern, not the matrix); enrichment (steps > 0; steps == 0:
 * none, step_size is then ignored) takes its candidates from the stored rows of A; drop (0: none) filters the computed
 * G as rlh_fsfilter_create does; rlh_fsvalues_update* keeps the pattern and does not apply the rule again.
 * prefilter must be finite with 0 < prefilter < 1.  The decisions read A alone, every row's members are written in
 * ascending order by ranks: G is the same bits in every run, for both index widths, from host or device arrays and for
 * both settings of RLH_FSAI_BINS.  With no weak entry G is bit for bit that of the forms above.
 * rlh_fsthreshold_info: the threshold a handle was built with and the stored entries below the diagonal that were not
 * strong (0, 0: a handle of the other forms). */
int rlh_fsthreshold_create_device(rlh_fsai_t *h, int dtype, int64_t n, int index_bits, const void *d_indptr,
                                  const void *d_indices, const void *d_values, int max_row, int levels, int steps,
                                  int step_size, double drop, double prefilter);
int rlh_fsthreshold_create(rlh_fsai_t *h, int dtype, int64_t n, const int64_t *indptr, const int32_t *indices,
                           const void *values, int max_row, int levels, int steps, int step_size, double drop,
                           double prefilter);
int rlh_fsthreshold_info(rlh_fsai_t h, double *prefilter, int64_t *weak_entries);
/* Y = G^H (G X) for column-major DEVICE blocks of m vectors (leading dimensions >= n; Y may be X): two sparse
 * products (the kernels of rlh_spd_apply, bit-identical from call to call) through an n x m workspace of the handle,
 * which grows when a wider block than before arrives (that call synchronises the stream once); otherwise
 * asynchronous on the library stream. */
int rlh_fsai_apply(rlh_fsai_t h, int64_t m, const void *X, int64_t ldx, void *Y, int64_t ldy);
/* size, stored entries of G, its longest row, the rows cut to max_row, device bytes held (G, G^H, their partitions,
 * the workspaces) and the seconds the set-up took on the device (events around the whole build) */
int rlh_fsai_info(rlh_fsai_t h, int64_t *n, int64_t *nnz, int64_t *longest_row, int64_t *truncated_rows,
                  int64_t *device_bytes, double *setup_seconds);
/* G as CSR in HOST arrays: n + 1 int64 row pointers, nnz int32 columns, nnz values of the dtype; synchronises */
int rlh_fsai_get(rlh_fsai_t h, int64_t *indptr, int32_t *indices, void *values);
int rlh_fsai_destroy(rlh_fsai_t h);

/* ---- the approximate inverse's own application: Y = G^H (G X) in two kernels, the work block W = G X kept in the
 *      handle's type or narrower.  A plan is made from a built handle and owns copies of G and G^H in a layout of its
 *      own (slices of 64 rows stored position-major, the long rows' remainders in a CSR tail; never more than twice
 *      the entries in slots: before the first product device_bytes <= 2 (nnz(G) + nnz(G^H)) (4 + sizeof V) + 64 n +
 *      4096 for every matrix); the handle is not referenced after the return and may be destroyed first.
 * work 0 (native): values and W in the handle's dtype T.  work 1 (float32): values rounded once to float / complex
 * float (V), W kept in that type.  work 2 (bf16, real dtypes only): values in float, W in bfloat16 (rounded once per
 * element to nearest even on the float32 bits, as rlh_bf16_pack does).  All arithmetic is in T.  On float / complex
 * float handles work 1 is work 0.  The narrow forms are for blocks within the float32 range.
 * rlh_fsapply_create ends with a checking pass over the finished layout; a violation, an unknown `work`, work 2 on a
 * complex handle or a null argument return non-zero, a message that names the entry point, and a null plan.  n = 0
 * gives a valid empty plan.
 * rlh_fsapply_run: column-major DEVICE blocks of m vectors at element alignment, leading dimensions >= n, Y may be X;
 * rows from n on and vectors from m on are neither read nor written.  The order of every sum is fixed by the layout:
 * the same bits from call to call, and column j of a call with m vectors has the bits of the same vector applied
 * alone.  W grows when a wider block than before arrives (that call synchronises the stream once); otherwise
 * asynchronous on the library stream.
 * rlh_fsapply_info: the work form, the slots of the sliced parts (padding included) and the entries in the tails, both
 * layouts together, and the device bytes held (layouts and W). */
typedef struct rlh_fsapply *rlh_fsapply_t;
int rlh_fsapply_create(rlh_fsapply_t *p, rlh_fsai_t h, int work);
int rlh_fsapply_run(rlh_fsapply_t p, int64_t m, const void *X, int64_t ldx, void *Y, int64_t ldy);
int rlh_fsapply_info(rlh_fsapply_t p, int *work, int64_t *stored_slots, int64_t *tail_entries, int64_t *device_bytes);
int rlh_fsapply_destroy(rlh_fsapply_t p);

/* ---- new matrix values on the kept pattern: every row of G is solved again, for a new matrix A', on the columns the
 *      handle already has, and the new values go everywhere the handle and a plan keep them.  Only the numeric phase
 *      of a build runs: no pattern walk, no enrichment, no filter, no transpose, no partition; nothing but status
 *      records travels to the host.  What a handle of any create call above paid for its pattern is paid once for a
 *      whole sequence of matrices (continuation, parameter sweeps, nonlinear or time-dependent operators).
 * rlh_fsvalues_update_device: a canonical CSR matrix of the handle's n and dtype in DEVICE memory (index_bits 32 or
 * 64).  The upper triangle defines A'; nothing below the diagonal is read.  The checks are those of the create calls on
 * indptr[0], a decreasing indptr, the last entry against the allocations, the column range, strict ascent and a stored
 * diagonal, with their messages under this entry point's name, each naming the smallest offending row.  The structure
 * of A' may differ from that of the matrix the handle was built from: a position of a local block that A' does not
 * store is zero, explicit zeros change nothing, and there is no partner check.
 * rlh_fsvalues_update: the same from HOST arrays (int64 row pointers, int32 columns), which are uploaded and take the
 * same path.
 * Row i keeps its columns P; its values become those of the local solve of the create calls on S = A'[P, P] (the
 * same kernel in the bin of the row's length, RLH_FSAI_BINS read as a create call reads it; a row's bits do not depend
 * on its bin).  They are written into G and, conjugated, into the matching places of G^H: the bits a build on the
 * same pattern would store.  Where the pattern came from levels alone and the structure of A' is that of A, the
 * handle is bit for bit the fresh build of A'; where it was chosen by value (steps, drop) it is the Kaporin minimiser
 * for A' on the pattern chosen for A.  A block that is not positive definite fails the call with the build's message.
 * All or nothing: the rows are solved into scratch and committed when every one succeeded; after a failed call the
 * handle holds the bits it held before.  Afterwards rlh_fsai_get and rlh_fsai_apply act on the new G; rlh_fsai_info
 * (nnz, longest_row, truncated_rows, setup_seconds), rlh_fsfilter_info, rlh_fsai_levels and rlh_fsai_adaptive keep
 * describing how the pattern was made.  The scratch lives for the call only: device_bytes does not change and
 * rlh_device_live returns to its level.  n = 0 is a valid update that does nothing.  Synchronises.
 * rlh_fsvalues_plan: refills the values of both layouts of a plan made from that handle from the handle's current
 * arrays, rounded to the plan's V as at creation; W and the layout's structure stay.  A plan that is not refilled
 * keeps applying the old values.  Refused, with a message naming the entry point, when n, the dtype, the entries or
 * the row lengths of plan and handle do not match.  (Row-shard plans are refilled by rlh_shardvalues_refill, below.)
 * rlh_fsvalues_info: the successful updates of the handle and the device seconds of the last one (events). */
int rlh_fsvalues_update_device(rlh_fsai_t h, int index_bits, const void *d_indptr, const void *d_indices,
                               const void *d_values);
int rlh_fsvalues_update(rlh_fsai_t h, const int64_t *indptr, const int32_t *indices, const void *values);
int rlh_fsvalues_plan(rlh_fsapply_t p, rlh_fsai_t h);
int rlh_fsvalues_info(rlh_fsai_t h, int64_t *updates, double *seconds);

/* ---- the same application on a ROW SHARD of G: rank r owns the rows [r0, r1) of the vectors, G_loc = the rows
 *      [r0, r1) of G and GH_loc = the rows [r0, r1) of G^H (the own COLUMNS of G, values conjugated by the caller).
 * rlh_fsshard_create: HOST CSR arrays of the two matrices, n_own rows each.  A column c of G_loc is own row c for
 * c < n_own and row c - n_own of the x-halo block (n_xhalo rows, of lower ranks) otherwise; the columns of GH_loc
 * number the rows of W the same way (n_whalo halo rows, of higher ranks).  The entries of a row are multiplied in
 * the order given.  dtype, work, the rounding of the values to V, the layout, its memory condition (with the entries
 * of G_loc and GH_loc) and the checking pass are those of rlh_fsapply_create; null pointers, negative sizes, an indptr
 * that does not start at 0 or decreases, and a column outside [0, n_own + halo rows) return non-zero, a message that
 * names the entry point, and a null plan.  n_own = 0 gives a valid empty plan.
 * One application is
 *   rlh_fsshard_first   W[own rows] = G_loc [X ; XH]: X the own rows (column-major DEVICE block, ldx >= n_own), XH the
 *                       x-halo block (ldxh >= n_xhalo; may be null iff n_xhalo == 0); a halo row that no entry
 *                       references is never read.  Starts a new application: the count of placed halo rows is reset.
 *   rlh_fsshard_pack    out[tile][i][8] = W[tile][d_idx[i]][8], i < nidx: the rows of W a peer needs, whole 16-byte
 *                       pieces; d_idx: DEVICE int64 (as for rlh_gather_rows), every index in [0, n_own) -- the
 *                       caller's contract (the indices are in device memory; an index outside is not followed, its
 *                       row arrives as zeros); out: ((m + 7) / 8) * nidx * w_row_bytes bytes.
 *   rlh_fsshard_halo    places a received packed block [tile][count][8] into the halo rows first .. first + count of
 *                       W; the plan counts the rows placed since the last rlh_fsshard_first.
 *   rlh_fsshard_second  Y[own rows] = GH_loc W over all n_own + n_whalo rows of W (ldy >= n_own; Y may be X).  Refused
 *                       when no rlh_fsshard_first with the same m came before or fewer than n_whalo halo rows have
 *                       been placed ("halo rows missing"): a forgotten exchange is a message, not a read of
 *                       undefined memory.
 * All four are asynchronous on the library stream (rlh_fsshard_first synchronises once when W grows); the order of
 * every sum is fixed by the layout, as for rlh_fsapply_run.
 * rlh_fsshard_info: as rlh_fsapply_info, and the bytes of one row of W in a tile, w_row_bytes = 8 * sizeof(Wt)
 * (16, 32, 64 or 128): what a row costs in a message. */
typedef struct rlh_fsshard *rlh_fsshard_t;
int rlh_fsshard_create(rlh_fsshard_t *p, int dtype, int work, int64_t n_own, int64_t n_xhalo, int64_t n_whalo,
                       const int64_t *g_indptr, const int32_t *g_indices, const void *g_values,
                       const int64_t *gh_indptr, const int32_t *gh_indices, const void *gh_values);
int rlh_fsshard_first(rlh_fsshard_t p, int64_t m, const void *X, int64_t ldx, const void *XH, int64_t ldxh);
int rlh_fsshard_pack(rlh_fsshard_t p, int64_t m, int64_t nidx, const int64_t *d_idx, void *out);
int rlh_fsshard_halo(rlh_fsshard_t p, int64_t m, int64_t first, int64_t count, const void *src);
int rlh_fsshard_second(rlh_fsshard_t p, int64_t m, void *Y, int64_t ldy);
int rlh_fsshard_info(rlh_fsshard_t p, int *work, int64_t *stored_slots, int64_t *tail_entries, int64_t *device_bytes,
                     int64_t *w_row_bytes);
int rlh_fsshard_destroy(rlh_fsshard_t p);

/* ---- new matrix values on a ROW SHARD: a row-shard plan refilled from the builder handle h that made the shard's rows
 *      of G (the build on the shard's extended block: the rows of lower ranks its rows reference, then its own rows
 *      from `first_row` on) after rlh_fsvalues_update* has given that handle new values on its kept pattern.  Nothing
 *      but a status record visits the host.  Positions count entries from the first entry of row first_row of the
 *      handle's G, indptr[first_row].
 * rlh_shardvalues_pack: d_out[i] = the handle's value of G at entry indptr[first_row] + d_pos[i], i < count, in the
 * handle's type: the values that lower ranks own as columns, in the order the caller's position list gives.  d_pos:
 * DEVICE int64.  A position outside the entries of the rows first_row .. n is not followed: its value arrives as zero
 * (the contract of rlh_fsshard_pack).  Read-only on the handle; asynchronous on the library stream.
 * rlh_shardvalues_refill: the rows first_row .. n of the handle's G must be the plan's G_loc entry for entry and in the
 * same order (the plan keeps its own column numbering).  Entry k of GH_loc, in the CSR order given to
 * rlh_fsshard_create, becomes the conjugate of the handle's entry d_src[k] (a position as above) where d_src[k] >= 0,
 * and of d_recv[-1 - d_src[k]] otherwise; d_src: DEVICE int64, one per entry of GH_loc; d_recv: n_recv values of the
 * handle's type in DEVICE memory (what rlh_shardvalues_pack made on the higher ranks; may be null iff n_recv == 0).  Both
 * layouts get values only, rounded once to the plan's V as at creation; columns, slots, tails and W are not touched.
 * The row pointers of GH_loc are not kept by the plan: they are rebuilt from the layout's row lengths in scratch.
 * Before any write: null arguments, the dtype of plan and handle, n - first_row against the plan's own rows, the
 * entries of those rows against the plan's G_loc, every row length, and every d_src[k] in [-n_recv, entries) -- a
 * violation returns non-zero with a message that names the entry point and the smallest offending row or entry, and
 * the plan applies the bits it applied before.  The scratch lives for the call only: rlh_device_live returns to its
 * level.  A plan without own rows is a valid refill that does nothing.  Synchronises for the status, and when the
 * values are in (nothing of the caller's is referenced after the return).
 * rlh_shardvalues_info: the successful refills of the plan and the device seconds of the last one (events). */
int rlh_shardvalues_pack(rlh_fsai_t h, int64_t first_row, int64_t count, const int64_t *d_pos, void *d_out);
int rlh_shardvalues_refill(rlh_fsshard_t p, rlh_fsai_t h, int64_t first_row, const int64_t *d_src, int64_t n_recv,
                           const void *d_recv);
int rlh_shardvalues_info(rlh_fsshard_t p, int64_t *updates, double *seconds);

/* ---- profiling aid: HIP-event time of the last `count` kernels ---- */
int rlh_timer_start(void);
int rlh_timer_stop(float *milliseconds);

#ifdef __cplusplus
}
#endif
#endif /* RLHIP_H */
