// General (rectangular) sparse data matrix: Y = Op(A) X - u c^T for Op(A) = A or A^H, A an M x N CSR matrix.
//
// The operator of truncated SVD / PCA on sparse data (rlh_spd_*, include/rlhip.h).  Both products run on the
// same row-parallel kernel: the handle holds A and a CSR copy of A^H (values conjugated, entries of each row in
// ascending order of A's row index) built once: on the host threads from host arrays (rlh_spd_create), by kernels
// from arrays that already lie in device memory (rlh_spd_create_device; the same arrays either way).
//
// One product of a panel of at most kPanel vectors is four launches on the library stream:
//   1. interleave: the column-major input block -> a row-major workspace Xi (row stride wp >= w, padded with
//      zeros to whole 16-byte pieces), so that one stored entry gathers ONE contiguous row of w values;
//   2. merge: the work is split by nonzeros, not by rows (merge path over the row ends and the nonzeros:
//      every subgroup of L lanes consumes kItems of the M + nnz items).  Rows that lie inside one subgroup's
//      range are written to the row-major result Yi; the part of a row a subgroup holds at the start of its
//      range (head) or at its end (tail) goes to a partials slot of its own;
//   3. fixup: the subgroup that consumes the end of a split row adds that row's partials in subgroup order
//      (a fixed order: no floating-point atomics, the same bits on every call and for every handle of the
//      same matrix);
//   4. deinterleave: Yi -> Y by columns (coalesced stores) with the rank-one epilogue Y[:, j] -= c[j] u.
// The partition (the row at which each subgroup starts) depends on the matrix alone and is built with the
// handle.  Every offset that scales with nnz or rows x vectors is 64-bit.
// spd_set_values (spmm_data.h) gives an operator new values on the structure it has: A's values are copied, those of
// A^H written by spd_conj_values; index arrays and partitions stay.
#include "common.h"
#include "device_build.h"
#include "spmm_data.h"

#include <algorithm>
#include <chrono>

namespace rlh {
namespace {

constexpr int kItems = 256;       // merge-path items (row ends + nonzeros) per subgroup
constexpr int kPanel = 64;        // vectors per panel: one interleaved row is at most 64 x 16 B
constexpr int kUnroll = 8;

template <typename T> struct alignas(16) Pack {
  static constexpr int n = 16 / (int)sizeof(T);
  T v[n];
};

__device__ __forceinline__ float one_of(float) { return 1.f; }
__device__ __forceinline__ double one_of(double) { return 1.0; }
__device__ __forceinline__ c32 one_of(c32) { return c32{1.f, 0.f}; }
__device__ __forceinline__ c64 one_of(c64) { return c64{1.0, 0.0}; }
__device__ __forceinline__ float sub_of(float a, float b) { return a - b; }
__device__ __forceinline__ double sub_of(double a, double b) { return a - b; }
__device__ __forceinline__ c32 sub_of(c32 a, c32 b) { return c32{a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ c64 sub_of(c64 a, c64 b) { return c64{a.re - b.re, a.im - b.im}; }

template <typename T> __device__ __forceinline__ void pack_zero(Pack<T> &p) {
#pragma unroll
  for (int e = 0; e < Pack<T>::n; ++e) p.v[e] = zero_of(T{});
}
template <typename T> __device__ __forceinline__ void pack_fma(Pack<T> &acc, T a, const Pack<T> &x) {
#pragma unroll
  for (int e = 0; e < Pack<T>::n; ++e) fma_acc(acc.v[e], a, x.v[e]);
}
template <typename T> __device__ __forceinline__ void pack_add(Pack<T> &acc, const Pack<T> &x) {
#pragma unroll
  for (int e = 0; e < Pack<T>::n; ++e) acc.v[e] = add_of(acc.v[e], x.v[e]);
}

// Xi[r * wp + j] = X[r + j * ldx] for j < w, 0 for w <= j < wp; tiles of 64 rows x 16 columns through the LDS
// (loads run down the columns of X, stores along the rows of Xi)
template <typename T>
__global__ __launch_bounds__(kBlock) void spd_interleave(int64_t n, int w, int wp, const T *__restrict__ X, int64_t ldx,
                                                         T *__restrict__ Xi) {
  __shared__ T tile[64][17];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  const int j0 = blockIdx.y * 16;
  for (int jj = ty; jj < 16; jj += 4) {
    const int64_t r = r0 + tx;
    const int j = j0 + jj;
    tile[tx][jj] = (r < n && j < w) ? X[r + (int64_t)j * ldx] : zero_of(T{});
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 64 * 16; e += kBlock) {
    const int rr = e >> 4, jj = e & 15;
    const int64_t r = r0 + rr;
    const int j = j0 + jj;
    if (r < n && j < wp) Xi[r * wp + j] = tile[rr][jj];
  }
}

// Y[r + j * ldy] = Yi[r * wp + j] - c[j] u[r] (u NULL: ones; c NULL: no rank-one term), j < w
template <typename T>
__global__ __launch_bounds__(kBlock) void spd_deinterleave(int64_t n, int w, int wp, const T *__restrict__ Yi,
                                                           T *__restrict__ Y, int64_t ldy, const T *__restrict__ u,
                                                           const T *__restrict__ c) {
  __shared__ T tile[64][17];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  const int j0 = blockIdx.y * 16;
  for (int e = threadIdx.x; e < 64 * 16; e += kBlock) {
    const int rr = e >> 4, jj = e & 15;
    const int64_t r = r0 + rr;
    const int j = j0 + jj;
    if (r < n && j < w) tile[rr][jj] = Yi[r * wp + j];
  }
  __syncthreads();
  for (int jj = ty; jj < 16; jj += 4) {
    const int64_t r = r0 + tx;
    const int j = j0 + jj;
    if (r < n && j < w) {
      T y = tile[tx][jj];
      if (c) y = sub_of(y, mul_of(c[j], u ? u[r] : one_of(T{})));
      Y[r + (int64_t)j * ldy] = y;
    }
  }
}

// Subgroup g (L lanes, lane owns the 16-byte piece `lane` of a row) consumes the merge items
// [d_g, d_{g+1}), d_g = min(g * kItems, M + nnz), starting at row row_at[g] and nonzero d_g - row_at[g].
// Row i is complete in this range when its end item is consumed (i < the next start row).  A complete row
// that began in an earlier range (the start nonzero lies past indptr[i]) goes to the head slot 2g, the row
// in progress at the end of the range to the tail slot 2g + 1; every other row straight to Yi.
template <typename T>
__global__ __launch_bounds__(kBlock) void spd_merge(int64_t M, int64_t total, int64_t G, int Lshift,
                                                    const int64_t *__restrict__ indptr, const int32_t *__restrict__ idx,
                                                    const T *__restrict__ val, const int32_t *__restrict__ row_at,
                                                    const Pack<T> *__restrict__ Xi, Pack<T> *__restrict__ Yi,
                                                    Pack<T> *__restrict__ part) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t g = t >> Lshift;
  const int L = 1 << Lshift;
  const int lane = (int)(t & (L - 1));
  if (g >= G) return;
  const int64_t i0 = row_at[g], i1 = row_at[g + 1];
  const int64_t k0 = std::min(g * (int64_t)kItems, total) - i0;
  const int64_t k1 = std::min((g + 1) * (int64_t)kItems, total) - i1;
  const Pack<T> *xl = Xi + lane;
  for (int64_t i = i0; i <= i1 && i < M; ++i) {
    const int64_t kb = (i == i0) ? k0 : indptr[i];
    const int64_t ke = (i == i1) ? k1 : indptr[i + 1];
    Pack<T> acc;
    pack_zero(acc);
    int64_t k = kb;
    for (; k + kUnroll <= ke; k += kUnroll) {
      int32_t cc[kUnroll];
      T vv[kUnroll];
      Pack<T> xx[kUnroll];
#pragma unroll
      for (int q = 0; q < kUnroll; ++q) { cc[q] = idx[k + q]; vv[q] = val[k + q]; }
#pragma unroll
      for (int q = 0; q < kUnroll; ++q) xx[q] = xl[(int64_t)cc[q] << Lshift];
#pragma unroll
      for (int q = 0; q < kUnroll; ++q) pack_fma(acc, vv[q], xx[q]);
    }
    for (; k < ke; ++k) pack_fma(acc, val[k], xl[(int64_t)idx[k] << Lshift]);
    Pack<T> *dst;
    if (i < i1)
      dst = (i == i0 && k0 > indptr[i0]) ? part + ((2 * g) << Lshift) : Yi + (i << Lshift);
    else
      dst = part + ((2 * g + 1) << Lshift);
    dst[lane] = acc;
  }
}

// The subgroup g that completes a split row r (it starts inside r and ends past it) writes
// Yi[r] = tail(ga) + ... + tail(g - 1) + head(g), ga = the last subgroup that started before r (or the first
// that started in it when r begins at item 0): the partials in subgroup order.
template <typename T>
__global__ __launch_bounds__(kBlock) void spd_fixup(int64_t M, int64_t total, int64_t G, int Lshift,
                                                    const int64_t *__restrict__ indptr, const int32_t *__restrict__ row_at,
                                                    const Pack<T> *__restrict__ part, Pack<T> *__restrict__ Yi) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t g = t >> Lshift;
  const int lane = (int)(t & ((1 << Lshift) - 1));
  if (g >= G) return;
  const int64_t r = row_at[g];
  if (r >= M || row_at[g + 1] <= r) return;
  const int64_t k0 = std::min(g * (int64_t)kItems, total) - r;
  if (k0 <= indptr[r]) return;
  int64_t lo = 0, hi = g;                // gf = the first subgroup that starts in row r (row_at is nondecreasing)
  while (lo < hi) {
    const int64_t mid = (lo + hi) / 2;
    if (row_at[mid] < r) lo = mid + 1; else hi = mid;
  }
  const int64_t ga = lo > 0 ? lo - 1 : 0;
  Pack<T> acc;
  pack_zero(acc);
  int64_t h = ga;
  for (; h + kUnroll <= g; h += kUnroll) {  // loads issued together, added in subgroup order
    Pack<T> pp[kUnroll];
#pragma unroll
    for (int q = 0; q < kUnroll; ++q) pp[q] = part[((2 * (h + q) + 1) << Lshift) + lane];
#pragma unroll
    for (int q = 0; q < kUnroll; ++q) pack_add(acc, pp[q]);
  }
  for (; h < g; ++h) pack_add(acc, part[((2 * h + 1) << Lshift) + lane]);
  pack_add(acc, part[((2 * g) << Lshift) + lane]);
  Yi[(r << Lshift) + lane] = acc;
}

// One orientation of the operator on the device: CSR arrays and the merge-path partition.
struct Side {
  int64_t rows = 0, cols = 0, nnz = 0, G = 0;
  DevBuf<int64_t> indptr;
  DevBuf<int32_t> idx;
  DevBuf<void> val;
  DevBuf<int32_t> row_at;         // G + 1 start rows
};

}  // namespace
}  // namespace rlh

struct rlh_spd {
  int dtype = 0;
  rlh::Side side[2];              // 0: A, 1: A^H
  double transpose_seconds = 0;
  // workspace, grown on demand: Xi, Yi, partials
  rlh::DevBuf<char> work;
};

namespace rlh {
namespace {

int64_t side_bytes(const Side &s, int64_t es) {
  return 8 * (s.rows + 1) + s.nnz * (4 + es) + 4 * (s.G + 1);
}

// row_at[g] = the largest i in [0, rows] with i + indptr[i] <= min(g * kItems, rows + nnz)
void partition(const int64_t *indptr, int64_t rows, int64_t nnz, int64_t G, std::vector<int32_t> &row_at) {
  row_at.resize(G + 1);
  const int64_t total = rows + nnz;
  host_parallel((int)std::min<int64_t>(16, G / 4096 + 1), [&](int t, int nt) {
    for (int64_t g = t; g <= G; g += nt) {
      const int64_t d = std::min(g * (int64_t)kItems, total);
      int64_t lo = 0, hi = rows;           // invariant: lo + indptr[lo] <= d
      while (lo < hi) {
        const int64_t mid = (lo + hi + 1) / 2;
        if (mid + indptr[mid] <= d) lo = mid; else hi = mid - 1;
      }
      row_at[g] = (int32_t)lo;
    }
  });
}

static inline float host_conj(float a) { return a; }
static inline double host_conj(double a) { return a; }
static inline c32 host_conj(c32 a) { return c32{a.re, -a.im}; }
static inline c64 host_conj(c64 a) { return c64{a.re, -a.im}; }

// CSR of A^H: stable counting sort by column over row chunks (thread t owns rows [r_t, r_{t+1}) and, in every
// column, the places after those of threads < t), so entries keep ascending row order; values conjugated.
template <typename T>
void transpose_host(int64_t M, int64_t N, const int64_t *ip, const int32_t *ix, const T *va, std::vector<int64_t> &tp,
                    std::vector<int32_t> &tx, std::vector<T> &tv) {
  const int64_t nnz = ip[M];
  int nt = (int)std::min<int64_t>(host_threads(), nnz / (1 << 16) + 1);
  nt = (int)std::max<int64_t>(1, std::min<int64_t>(nt, (int64_t)(512 << 20) / (8 * (N + 1))));
  std::vector<int64_t> rstart(nt + 1);
  for (int t = 0; t <= nt; ++t) {        // row chunks of about equal nonzeros
    const int64_t target = nnz * t / nt;
    rstart[t] = t == nt ? M : std::lower_bound(ip, ip + M + 1, target) - ip;
  }
  std::vector<std::vector<int64_t>> cnt(nt, std::vector<int64_t>(N, 0));
  host_parallel(nt, [&](int t, int) {
    auto &c = cnt[t];
    for (int64_t k = ip[rstart[t]]; k < ip[rstart[t + 1]]; ++k) ++c[ix[k]];
  });
  tp.assign(N + 1, 0);
  for (int64_t j = 0; j < N; ++j) {
    int64_t s = 0;
    for (int t = 0; t < nt; ++t) s += cnt[t][j];
    tp[j + 1] = tp[j] + s;
  }
  host_parallel(nt, [&](int t, int) {      // cnt[t][j] becomes thread t's first place in column j
    for (int64_t j = (int64_t)N * t / nt; j < (int64_t)N * (t + 1) / nt; ++j) {
      int64_t o = tp[j];
      for (int s = 0; s < nt; ++s) { const int64_t c = cnt[s][j]; cnt[s][j] = o; o += c; }
    }
  });
  tx.resize(nnz);
  tv.resize(nnz);
  host_parallel(nt, [&](int t, int) {
    auto &c = cnt[t];
    for (int64_t r = rstart[t]; r < rstart[t + 1]; ++r)
      for (int64_t k = ip[r]; k < ip[r + 1]; ++k) {
        const int64_t p = c[ix[k]]++;
        tx[p] = (int32_t)r;
        tv[p] = host_conj(va[k]);
      }
  });
}

int upload_side(Side &s, int64_t rows, int64_t cols, const int64_t *ip, const int32_t *ix, const void *va, int64_t es) {
  s.rows = rows;
  s.cols = cols;
  s.nnz = ip[rows];
  s.G = (rows + s.nnz + kItems - 1) / kItems;
  std::vector<int32_t> row_at;
  partition(ip, rows, s.nnz, s.G, row_at);
  if (int rc = s.indptr.upload(ip, 8 * (rows + 1))) return rc;
  if (int rc = s.idx.upload(ix, 4 * s.nnz, 4)) return rc;
  if (int rc = s.val.upload(va, es * s.nnz, 16)) return rc;
  return s.row_at.upload(row_at.data(), 4 * (s.G + 1));
}

template <typename T>
int create_impl(rlh_spd *h, int64_t M, int64_t N, const int64_t *ip, const int32_t *ix, const void *va) {
  const int64_t es = sizeof(T);
  if (int rc = upload_side(h->side[0], M, N, ip, ix, va, es)) return rc;
  auto t0 = std::chrono::steady_clock::now();
  std::vector<int64_t> tp;
  std::vector<int32_t> tx;
  std::vector<T> tv;
  transpose_host<T>(M, N, ip, ix, (const T *)va, tp, tx, tv);
  h->transpose_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return upload_side(h->side[1], N, M, tp.data(), tx.data(), tv.data(), es);
}

// ---------------------------------------------------------------- the operator built on the device
// rlh_spd_create_device: the same arrays as create_impl, made by kernels on the library stream from CSR arrays
// that already lie in device memory.  The input is checked first (indptr, then the columns of every row); the
// host sees one 16-byte status record (the first violation, the number of stored entries) and nothing else.
// The transpose is transpose_host's stable counting sort with C row chunks of about equal nonzeros in place of
// the host threads: entries per (chunk, column) counted with integer atomics (sums: their order does not
// matter), a scan over the chunks within each column and over the columns, then one single-wave workgroup per
// chunk walks its rows in order with the lanes on the entries of ONE row -- a canonical row has distinct
// columns, so no two lanes take the same cursor and every entry's place is fixed by the matrix alone.

// row_at[g], g <= G: partition() on the device, one binary search per subgroup
__global__ __launch_bounds__(kBlock) void spd_partition(int64_t rows, int64_t nnz, int64_t G, const int64_t *__restrict__ indptr,
                                                        int32_t *__restrict__ row_at) {
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g > G) return;
  const int64_t d = std::min(g * (int64_t)kItems, rows + nnz);
  int64_t lo = 0, hi = rows;               // invariant: lo + indptr[lo] <= d
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) / 2;
    if (mid + indptr[mid] <= d) lo = mid; else hi = mid - 1;
  }
  row_at[g] = (int32_t)lo;
}

// rstart[t], t <= C: the first row whose entries begin at or after nnz * t / C (rstart[C] = M)
__global__ __launch_bounds__(kBlock) void spd_chunk_rows(int64_t M, int64_t nnz, int64_t C, const int64_t *__restrict__ ip,
                                                         int64_t *__restrict__ rstart) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t > C) return;
  if (t == C) { rstart[t] = M; return; }
  const int64_t target = (nnz / C) * t + (nnz % C) * t / C;
  int64_t lo = 0, hi = M;                  // lower_bound over ip[0 .. M]: ip[M] = nnz >= target
  while (lo < hi) {
    const int64_t mid = (lo + hi) / 2;
    if (ip[mid] < target) lo = mid + 1; else hi = mid;
  }
  rstart[t] = lo;
}

// cnt[t][c] = entries of chunk t in column c; S workgroups share the entries of one chunk
__global__ __launch_bounds__(kBlock) void spd_count(int64_t N, int S, const int64_t *__restrict__ ip, const int64_t *__restrict__ rstart,
                                                    const int32_t *__restrict__ ix, unsigned long long *cnt) {
  const int64_t t = blockIdx.x / S;
  const int s = (int)(blockIdx.x % S);
  const int64_t kb = ip[rstart[t]], ke = ip[rstart[t + 1]];
  unsigned long long *row = cnt + t * N;
  for (int64_t k = kb + (int64_t)s * kBlock + threadIdx.x; k < ke; k += (int64_t)S * kBlock) atomicAdd(row + ix[k], 1ull);
}

__global__ __launch_bounds__(kBlock) void spd_column_totals(int64_t N, int64_t C, const int64_t *__restrict__ cnt, int64_t *__restrict__ tot) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= N) return;
  int64_t s = 0;
  for (int64_t t = 0; t < C; ++t) s += cnt[t * N + j];
  tot[j] = s;
}

// cnt[t][j] becomes chunk t's first place in column j
__global__ __launch_bounds__(kBlock) void spd_chunk_places(int64_t N, int64_t C, const int64_t *__restrict__ tp, int64_t *__restrict__ cnt) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= N) return;
  int64_t o = tp[j];
  for (int64_t t = 0; t < C; ++t) {
    const int64_t c = cnt[t * N + j];
    cnt[t * N + j] = o;
    o += c;
  }
}

// one single-wave workgroup per chunk: the rows in order, the lanes on the entries of one row (distinct
// columns: distinct cursors); the barrier orders the cursor updates of one row before the reads of the next
template <typename T>
__global__ __launch_bounds__(64) void spd_scatter(const int64_t *__restrict__ ip, const int64_t *__restrict__ rstart,
                                                  const int32_t *__restrict__ ix, const T *__restrict__ va, int64_t N, int64_t *cur_all,
                                                  int32_t *__restrict__ tx, T *__restrict__ tv) {
  const int64_t t = blockIdx.x;
  int64_t *cur = cur_all + t * N;
  const int64_t r1 = rstart[t + 1];
  for (int64_t r = rstart[t]; r < r1; ++r) {
    const int64_t kb = ip[r], ke = ip[r + 1];
    if (kb == ke) continue;                // (the same decision in every lane)
    for (int64_t k = kb + threadIdx.x; k < ke; k += 64) {
      const int32_t c = ix[k];
      const int64_t p = cur[c];
      cur[c] = p + 1;
      tx[p] = (int32_t)r;
      tv[p] = dev_conj(va[k]);
    }
    __syncthreads();
  }
}

int alloc_side(Side &s, int64_t rows, int64_t cols, int64_t nnz, int64_t es) {
  s.rows = rows;
  s.cols = cols;
  s.nnz = nnz;
  s.G = (rows + nnz + kItems - 1) / kItems;
  if (int rc = s.indptr.alloc(rows + 1)) return rc;
  if (int rc = s.idx.alloc(std::max<int64_t>(nnz, 1))) return rc;
  if (int rc = s.val.alloc(std::max<int64_t>(es * nnz, 16))) return rc;
  return s.row_at.alloc(s.G + 1);
}

// the number of row chunks: about kChunkNnz entries each, the C x N table of places within the cap
// (RLH_SPD_TABLE_BYTES, 512 MB as transpose_host caps its own), at least one
constexpr int64_t kChunkNnz = 8192;
int64_t chunk_count(int64_t nnz, int64_t N) {
  const char *e = getenv("RLH_SPD_TABLE_BYTES");
  int64_t cap = (e && *e) ? atoll(e) : (int64_t)512 << 20;
  int64_t C = nnz / kChunkNnz + 1;
  C = std::min<int64_t>(C, cap / (8 * (N + 1)));
  return std::max<int64_t>(C, 1);
}

template <typename T, typename I>
int create_device_impl(rlh_spd *h, int64_t M, int64_t N, const I *ip, const I *ix, const T *va) {
  const int64_t es = sizeof(T);
  hipStream_t st = ctx().stream;
  const dim3 blk(kBlock);
  StreamTimer timer;
  DevBuf<BuildStatus> status;
  DevBuf<int64_t> rstart, cnt, tot, bsum;
  // ---- the checks (device_build.h; what they find is placed by its entry): one status record comes back
  constexpr const char *name = "rlh_spd_create_device";
  int64_t cap;
  BuildStatus hs;
  if (int rc = input_cap(name, "n_rows", M, ip, ix, va, &cap)) return rc;
  if (int rc = launch_input_checks<true>(M, N, ip, ix, cap, status, &hs)) return rc;
  if (int rc = fetch_input_status(name, status.get(), &hs, cap, true)) return rc;
  const int64_t nnz = hs.nnz;
  // ---- A: indptr as int64, columns as int32, the values
  Side &a = h->side[0], &b = h->side[1];
  if (int rc = alloc_side(a, M, N, nnz, es)) return rc;
  hipLaunchKernelGGL((spd_convert_index<I, int64_t>), dim3(blocks_for(M + 1, kBlock, 4096)), blk, 0, st, M + 1, ip, a.indptr);
  if (nnz) {
    hipLaunchKernelGGL((spd_convert_index<I, int32_t>), dim3(blocks_for(nnz, kBlock, 8192)), blk, 0, st, nnz, ix, a.idx);
    RLH_HIP(hipMemcpyAsync(a.val, va, es * nnz, hipMemcpyDeviceToDevice, st));
  }
  hipLaunchKernelGGL(spd_partition, dim3(blocks_for(a.G + 1, kBlock, INT32_MAX)), blk, 0, st, M, nnz, a.G, a.indptr, a.row_at);
  RLH_HIP(hipGetLastError());
  // ---- A^H
  if (int rc = alloc_side(b, N, M, nnz, es)) return rc;
  const int64_t C = chunk_count(nnz, N);
  const int64_t nb = (N + kScanTile - 1) / kScanTile;
  if (int rc = rstart.alloc(C + 1)) return rc;
  if (int rc = cnt.alloc(std::max<int64_t>(C * N, 1))) return rc;
  if (int rc = tot.alloc(std::max<int64_t>(N, 1))) return rc;
  if (int rc = bsum.alloc(nb + 1)) return rc;
  if (int rc = timer.start()) return rc;
  RLH_HIP(hipMemsetAsync(cnt, 0, std::max<int64_t>(8 * C * N, 8), st));
  hipLaunchKernelGGL(spd_chunk_rows, dim3(blocks_for(C + 1, kBlock, INT32_MAX)), blk, 0, st, M, nnz, C, a.indptr, rstart);
  const int S = (int)std::max<int64_t>(1, std::min<int64_t>(64, 2048 / C));
  if (nnz && N)
    hipLaunchKernelGGL(spd_count, dim3((unsigned)(C * S)), blk, 0, st, N, S, a.indptr, rstart, a.idx, (unsigned long long *)cnt);
  if (N) hipLaunchKernelGGL(spd_column_totals, dim3(blocks_for(N, kBlock, INT32_MAX)), blk, 0, st, N, C, cnt, tot);
  if (int rc = exclusive_scan(N, tot, bsum, b.indptr)) return rc;
  if (N) hipLaunchKernelGGL(spd_chunk_places, dim3(blocks_for(N, kBlock, INT32_MAX)), blk, 0, st, N, C, b.indptr, cnt);
  if (nnz && N)
    hipLaunchKernelGGL(spd_scatter<T>, dim3((unsigned)C), dim3(64), 0, st, a.indptr, rstart, a.idx, (const T *)a.val, N, cnt,
                       b.idx, (T *)b.val);
  hipLaunchKernelGGL(spd_partition, dim3(blocks_for(b.G + 1, kBlock, INT32_MAX)), blk, 0, st, N, nnz, b.G, b.indptr, b.row_at);
  RLH_HIP(hipGetLastError());
  if (int rc = timer.stop()) return rc;
  h->transpose_seconds = timer.seconds();
  return 0;
}

// ---------------------------------------------------------------- new values on the structure the operator has
constexpr int kValuesBlocksPerCu = 8;   // grid of spd_conj_values: at most this many workgroups per CU

// Entry k of A^H is (j, i): j the last row of A^H with tp[j] <= k (tp[N] = nnz > k; empty rows share their start with
// the row that holds k and come before it), i = tx[k].  It takes the conjugate of A's entry (i, j), found by a binary
// search for column j in the sorted row i of A: every place is written once, by one thread, from one value -- the
// bits spd_scatter makes.  A thread per entry in a grid-stride loop; no atomics, no LDS.
template <typename T>
__global__ __launch_bounds__(kBlock) void spd_conj_values(int64_t N, int64_t nnz, const int64_t *__restrict__ ip,
                                                          const int32_t *__restrict__ ix, const T *__restrict__ va,
                                                          const int64_t *__restrict__ tp, const int32_t *__restrict__ tx,
                                                          T *__restrict__ tv) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < nnz; k += stride) {
    int64_t lo = 0, hi = N;                // invariant: tp[lo] <= k < tp[hi]
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) / 2;
      if (tp[mid] <= k) lo = mid; else hi = mid;
    }
    const int64_t j = lo, i = tx[k];
    int64_t f = ip[i];
    const int64_t fe = ip[i + 1];
    for (int64_t e = fe; f < e;) {         // the first entry of row i whose column is not below j
      const int64_t mid = (f + e) / 2;
      if ((int64_t)ix[mid] < j) f = mid + 1; else e = mid;
    }
    if (f < fe && (int64_t)ix[f] == j) tv[k] = dev_conj(va[f]);
  }
}

template <typename T> int set_values_impl(rlh_spd *h, const void *d_values) {
  Side &a = h->side[0], &b = h->side[1];
  hipStream_t st = ctx().stream;
  RLH_HIP(hipMemcpyAsync(a.val, d_values, sizeof(T) * a.nnz, hipMemcpyDeviceToDevice, st));
  const int64_t most = (int64_t)ctx().num_cu * kValuesBlocksPerCu;
  hipLaunchKernelGGL(spd_conj_values<T>, dim3(blocks_for(b.nnz, kBlock, most)), dim3(kBlock), 0, st, b.rows, b.nnz, a.indptr.get(),
                     a.idx.get(), (const T *)a.val.get(), b.indptr.get(), b.idx.get(), (T *)b.val.get());
  RLH_HIP(hipGetLastError());
  return 0;
}

// sums of squares of the rows in float64, entry by entry in the stored order (what numpy.bincount forms on the
// host: the same bits for real data), the modulus first, as numpy.abs forms it, then squared
// (the compiler must not contract these into fused multiply-adds: NumPy rounds every product and every sum)
__device__ __forceinline__ double mul_rounded(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ double add_rounded(double a, double b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ double modulus2(float v) { return mul_rounded((double)v, (double)v); }
__device__ __forceinline__ double modulus2(double v) { return mul_rounded(v, v); }
// numpy.abs of complex64 step by step in float32 (NumPy's vectorised loop: larger * sqrt(fma(r, r, 1)), r = smaller /
// larger; division, square root and the fused multiply-add are correctly rounded on both sides), so the host values
// of SparseMatrix.__init__ -- which carry this float32 rounding of the modulus -- are reproduced, not approximated
__device__ __forceinline__ double modulus2(c32 v) {
#pragma clang fp contract(off)
  const float re = fabsf(v.re), im = fabsf(v.im);
  const float larger = fmaxf(re, im), smaller = fminf(re, im);
  float m;
  if (larger == 0.f || isinf(larger)) m = larger;
  else {
    const float r = smaller / larger;
    m = sqrtf(fmaf(r, r, 1.0f)) * larger;
  }
  return mul_rounded((double)m, (double)m);
}
__device__ __forceinline__ double modulus2(c64 v) {     // the same steps in float64, as numpy.abs of complex128
#pragma clang fp contract(off)
  const double re = fabs(v.re), im = fabs(v.im);
  const double larger = fmax(re, im), smaller = fmin(re, im);
  double m;
  if (larger == 0.0 || isinf(larger)) m = larger;
  else {
    const double r = smaller / larger;
    m = sqrt(fma(r, r, 1.0)) * larger;
  }
  return mul_rounded(m, m);
}
__device__ __forceinline__ double part_max(float v) { return fabs((double)v); }
__device__ __forceinline__ double part_max(double v) { return fabs(v); }
__device__ __forceinline__ double part_max(c32 v) { return fmax(fabs((double)v.re), fabs((double)v.im)); }
__device__ __forceinline__ double part_max(c64 v) { return fmax(fabs(v.re), fabs(v.im)); }

template <typename T>
__global__ __launch_bounds__(kBlock) void spd_row_sumsq_kernel(int64_t M, const int64_t *__restrict__ ip, const T *__restrict__ va,
                                                               double *__restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= M) return;
  double s = 0.0;
  for (int64_t k = ip[r]; k < ip[r + 1]; ++k) s = add_rounded(s, modulus2(va[k]));
  out[r] = s;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void spd_absmax_kernel(int64_t nnz, const T *__restrict__ va, double *__restrict__ out) {
  __shared__ double red[kBlock / 64];
  double mx = 0.0;
  for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < nnz; k += (int64_t)gridDim.x * kBlock) mx = fmax(mx, part_max(va[k]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_down(mx, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 1; q < kBlock / 64; ++q) mx = fmax(mx, red[q]);
    out[blockIdx.x] = mx;
  }
}

template <typename T> int row_sumsq_impl(const Side &s, double *d_out) {
  hipLaunchKernelGGL(spd_row_sumsq_kernel<T>, dim3((unsigned)((s.rows + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx().stream, s.rows,
                     s.indptr, (const T *)s.val, d_out);
  return 0;
}
template <typename T> int absmax_impl(const Side &s, unsigned nb, double *d_out) {
  hipLaunchKernelGGL(spd_absmax_kernel<T>, dim3(nb), dim3(kBlock), 0, ctx().stream, s.nnz, (const T *)s.val, d_out);
  return 0;
}

// panel geometry: L lanes of 16 bytes hold one interleaved row of wp >= w elements (L a power of two)
void panel_shape(int w, int64_t es, int *Lshift, int *wp) {
  const int pieces = (int)((w * es + 15) / 16);
  int s = 0;
  while ((1 << s) < pieces) ++s;
  *Lshift = s;
  *wp = (int)(((int64_t)16 << s) / es);
}

int64_t work_need(const Side &s, int wp, int64_t es) {
  return es * wp * (s.cols + s.rows + 2 * s.G) + 3 * 256;
}

template <typename T>
int apply_impl(rlh_spd *h, const Side &s, int64_t m, const T *X, int64_t ldx, T *Y, int64_t ldy, const T *u, const T *c) {
  const int64_t es = sizeof(T);
  hipStream_t st = ctx().stream;
  const int wmax = (int)std::min<int64_t>(m, kPanel);
  int Lshift, wpmax;
  panel_shape(wmax, es, &Lshift, &wpmax);
  const int64_t need = work_need(s, wpmax, es);
  if (int rc = h->work.reserve(need)) return rc;      // grows once per larger block, then reused without allocation
  for (int64_t j0 = 0; j0 < m; j0 += kPanel) {
    const int w = (int)std::min<int64_t>(kPanel, m - j0);
    int wp;
    panel_shape(w, es, &Lshift, &wp);
    auto align = [](int64_t b) { return (b + 255) & ~(int64_t)255; };
    T *Xi = (T *)h->work;
    T *Yi = (T *)(h->work + align(es * wp * s.cols));
    T *part = (T *)((char *)Yi + align(es * wp * s.rows));
    const dim3 blk(kBlock);
    if (s.cols > 0) {
      const dim3 grid((unsigned)((s.cols + 63) / 64), (unsigned)((wp + 15) / 16));
      hipLaunchKernelGGL(spd_interleave<T>, grid, blk, 0, st, s.cols, w, wp, X + j0 * ldx, ldx, Xi);
    }
    const int64_t threads = s.G << Lshift;
    if (threads > 0) {
      const unsigned nb = (unsigned)((threads + kBlock - 1) / kBlock);
      const int64_t total = s.rows + s.nnz;
      hipLaunchKernelGGL(spd_merge<T>, dim3(nb), blk, 0, st, s.rows, total, s.G, Lshift, s.indptr, s.idx,
                         (const T *)s.val, s.row_at, (const Pack<T> *)Xi, (Pack<T> *)Yi, (Pack<T> *)part);
      hipLaunchKernelGGL(spd_fixup<T>, dim3(nb), blk, 0, st, s.rows, total, s.G, Lshift, s.indptr, s.row_at,
                         (const Pack<T> *)part, (Pack<T> *)Yi);
    }
    const dim3 grid((unsigned)((s.rows + 63) / 64), (unsigned)((w + 15) / 16));
    hipLaunchKernelGGL(spd_deinterleave<T>, grid, blk, 0, st, s.rows, w, wp, Yi, Y + j0 * ldy, ldy, u,
                       c ? c + j0 : nullptr);
    RLH_HIP(hipGetLastError());
  }
  return 0;
}

}  // namespace
}  // namespace rlh

rlh::SpdArrays rlh::spd_arrays(const rlh_spd *h, int transp) {
  const Side &s = h->side[transp ? 1 : 0];
  SpdArrays a;
  a.rows = s.rows; a.cols = s.cols; a.nnz = s.nnz;
  a.indptr = s.indptr; a.idx = s.idx; a.val = s.val;
  return a;
}

int rlh::spd_set_values(rlh_spd *h, const void *d_values) {
  if (!h->side[0].nnz) return 0;
  switch (h->dtype) {
    case RLH_S: return set_values_impl<float>(h, d_values);
    case RLH_D: return set_values_impl<double>(h, d_values);
    case RLH_C: return set_values_impl<c32>(h, d_values);
    case RLH_Z: return set_values_impl<c64>(h, d_values);
  }
  return 1;
}

using namespace rlh;

extern "C" int rlh_spd_create(rlh_spd_t *ph, int dtype, int64_t n_rows, int64_t n_cols, const int64_t *indptr,
                              const int32_t *indices, const void *values) {
  if (int rc = require_ready()) return rc;
  RLH_REQUIRE(ph, "rlh_spd_create: null handle pointer");
  *ph = nullptr;
  RLH_REQUIRE(dtype_valid(dtype), "rlh_spd_create: unknown dtype %d", dtype);
  RLH_REQUIRE(n_rows >= 0 && n_cols >= 0 && n_rows < INT32_MAX && n_cols < INT32_MAX,
              "rlh_spd_create: sizes must lie in [0, 2^31 - 1)");
  RLH_REQUIRE(indptr, "rlh_spd_create: null indptr");
  RLH_REQUIRE(indptr[0] == 0, "rlh_spd_create: indptr[0] must be 0");
  const int64_t nnz = indptr[n_rows];
  RLH_REQUIRE(nnz == 0 || (indices && values), "rlh_spd_create: null indices or values");
  for (int64_t r = 0; r < n_rows; ++r)
    RLH_REQUIRE(indptr[r + 1] >= indptr[r], "rlh_spd_create: indptr decreases at row %lld", (long long)r);
  for (int64_t k = 0; k < nnz; ++k)
    RLH_REQUIRE(indices[k] >= 0 && indices[k] < n_cols, "rlh_spd_create: column index out of range at entry %lld",
                (long long)k);
  rlh_spd *h = new rlh_spd();
  h->dtype = dtype;
  int rc = 1;
  switch (dtype) {
    case RLH_S: rc = create_impl<float>(h, n_rows, n_cols, indptr, indices, values); break;
    case RLH_D: rc = create_impl<double>(h, n_rows, n_cols, indptr, indices, values); break;
    case RLH_C: rc = create_impl<c32>(h, n_rows, n_cols, indptr, indices, values); break;
    case RLH_Z: rc = create_impl<c64>(h, n_rows, n_cols, indptr, indices, values); break;
  }
  if (rc) {
    rlh_spd_destroy(h);
    return rc;
  }
  *ph = h;
  return 0;
}

extern "C" int rlh_spd_create_device(rlh_spd_t *ph, int dtype, int64_t n_rows, int64_t n_cols, int index_bits,
                                     const void *d_indptr, const void *d_indices, const void *d_values) {
  if (int rc = require_ready()) return rc;
  RLH_REQUIRE(ph, "rlh_spd_create_device: null handle pointer");
  *ph = nullptr;
  RLH_REQUIRE(dtype_valid(dtype), "rlh_spd_create_device: unknown dtype %d", dtype);
  RLH_REQUIRE(index_bits == 32 || index_bits == 64, "rlh_spd_create_device: index_bits must be 32 or 64, got %d", index_bits);
  RLH_REQUIRE(n_rows >= 0 && n_cols >= 0 && n_rows < INT32_MAX && n_cols < INT32_MAX,
              "rlh_spd_create_device: sizes must lie in [0, 2^31 - 1)");
  RLH_REQUIRE(d_indptr, "rlh_spd_create_device: null indptr");
  rlh_spd *h = new rlh_spd();
  h->dtype = dtype;
  int rc = 1;
#define RLH_SPD_BUILD(T)                                                                                              \
  rc = index_bits == 32 ? create_device_impl<T, int32_t>(h, n_rows, n_cols, (const int32_t *)d_indptr,                \
                                                         (const int32_t *)d_indices, (const T *)d_values)             \
                        : create_device_impl<T, int64_t>(h, n_rows, n_cols, (const int64_t *)d_indptr,                \
                                                         (const int64_t *)d_indices, (const T *)d_values)
  switch (dtype) {
    case RLH_S: RLH_SPD_BUILD(float); break;
    case RLH_D: RLH_SPD_BUILD(double); break;
    case RLH_C: RLH_SPD_BUILD(c32); break;
    case RLH_Z: RLH_SPD_BUILD(c64); break;
  }
#undef RLH_SPD_BUILD
  if (rc) {
    rlh_spd_destroy(h);
    return rc;
  }
  *ph = h;
  return 0;
}

extern "C" int rlh_spd_row_sumsq(rlh_spd_t h, double *h_out) {
  if (int rc = require_ready()) return rc;
  RLH_REQUIRE(h, "rlh_spd_row_sumsq: null handle");
  const Side &s = h->side[0];
  if (s.rows == 0) return 0;
  RLH_REQUIRE(h_out, "rlh_spd_row_sumsq: null output");
  DevBuf<double> d;
  if (int rc = d.alloc(s.rows)) return rc;
  switch (h->dtype) {
    case RLH_S: row_sumsq_impl<float>(s, d); break;
    case RLH_D: row_sumsq_impl<double>(s, d); break;
    case RLH_C: row_sumsq_impl<c32>(s, d); break;
    case RLH_Z: row_sumsq_impl<c64>(s, d); break;
  }
  RLH_HIP(hipGetLastError());
  RLH_HIP(hipStreamSynchronize(ctx().stream));
  RLH_HIP(hipMemcpy(h_out, d, s.rows * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int rlh_spd_absmax(rlh_spd_t h, double *h_out) {
  if (int rc = require_ready()) return rc;
  RLH_REQUIRE(h && h_out, "rlh_spd_absmax: null handle or output");
  *h_out = 0.0;
  const Side &s = h->side[0];
  if (s.nnz == 0) return 0;
  const unsigned nb = blocks_for(s.nnz, kBlock, 1024);
  DevBuf<double> d;
  if (int rc = d.alloc(nb)) return rc;
  switch (h->dtype) {
    case RLH_S: absmax_impl<float>(s, nb, d); break;
    case RLH_D: absmax_impl<double>(s, nb, d); break;
    case RLH_C: absmax_impl<c32>(s, nb, d); break;
    case RLH_Z: absmax_impl<c64>(s, nb, d); break;
  }
  std::vector<double> host(nb);
  RLH_HIP(hipGetLastError());
  RLH_HIP(hipStreamSynchronize(ctx().stream));
  RLH_HIP(hipMemcpy(host.data(), d, nb * sizeof(double), hipMemcpyDeviceToHost));
  double mx = 0.0;
  for (double v : host) mx = v > mx ? v : mx;
  *h_out = mx;
  return 0;
}

extern "C" int rlh_spd_destroy(rlh_spd_t h) {
  if (!h) return 0;
  if (ctx().ready) (void)hipStreamSynchronize(ctx().stream);
  delete h;
  return 0;
}

extern "C" int rlh_spd_info(rlh_spd_t h, int64_t *n_rows, int64_t *n_cols, int64_t *nnz, int64_t *device_bytes) {
  RLH_REQUIRE(h, "rlh_spd_info: null handle");
  const int64_t es = dtype_size(h->dtype);
  if (n_rows) *n_rows = h->side[0].rows;
  if (n_cols) *n_cols = h->side[0].cols;
  if (nnz) *nnz = h->side[0].nnz;
  if (device_bytes) *device_bytes = side_bytes(h->side[0], es) + side_bytes(h->side[1], es) + (int64_t)h->work.bytes();
  return 0;
}

extern "C" int rlh_spd_stats(rlh_spd_t h, int64_t *workspace_bytes, double *transpose_seconds) {
  RLH_REQUIRE(h, "rlh_spd_stats: null handle");
  if (workspace_bytes) *workspace_bytes = (int64_t)h->work.bytes();
  if (transpose_seconds) *transpose_seconds = h->transpose_seconds;
  return 0;
}

extern "C" int rlh_spd_apply(rlh_spd_t h, int transp, int64_t m, const void *X, int64_t ldx, void *Y, int64_t ldy,
                             const void *d_u, const void *d_c) {
  if (int rc = require_ready()) return rc;
  RLH_REQUIRE(h, "rlh_spd_apply: null handle");
  RLH_REQUIRE(transp == 0 || transp == 1, "rlh_spd_apply: transp must be 0 or 1");
  RLH_REQUIRE(d_c || !d_u, "rlh_spd_apply: a vector u without coefficients c");
  RLH_REQUIRE(m >= 0, "rlh_spd_apply: negative number of vectors");
  const Side &s = h->side[transp];
  if (m == 0 || s.rows == 0) return 0;
  RLH_REQUIRE(Y && (s.cols == 0 || X), "rlh_spd_apply: null pointer");
  RLH_REQUIRE(ldx >= s.cols && ldy >= s.rows, "rlh_spd_apply: Matrix and vectors dimensions incompatible");
  switch (h->dtype) {
    case RLH_S: return apply_impl<float>(h, s, m, (const float *)X, ldx, (float *)Y, ldy, (const float *)d_u, (const float *)d_c);
    case RLH_D: return apply_impl<double>(h, s, m, (const double *)X, ldx, (double *)Y, ldy, (const double *)d_u, (const double *)d_c);
    case RLH_C: return apply_impl<c32>(h, s, m, (const c32 *)X, ldx, (c32 *)Y, ldy, (const c32 *)d_u, (const c32 *)d_c);
    case RLH_Z: return apply_impl<c64>(h, s, m, (const c64 *)X, ldx, (c64 *)Y, ldy, (const c64 *)d_u, (const c64 *)d_c);
  }
  return 1;
}
