// The approximate inverse's own application Y = G^H (G X) in two kernels (rlh_fsapply_*, include/rlhip.h).
//
// Types.  T: the handle's dtype, the type of X and Y and of all arithmetic.  V: the stored values of G and G^H (T, or
// float / complex float: G rounded once, to nearest).  Wt: the work block W = G X (T, float / complex float, or
// bfloat16 for real T: rounded once per element, nearest even).
//
// Layout, one per product (G for the first, G^H -- values already conjugated -- for the second), built by kernels
// from the handle's CSR arrays and owned by the plan:
//   slices   64 consecutive rows each, one wave per slice, lane <-> row; rows are not permuted.  Slice s keeps the
//            first width[s] entries of its rows position-major: entry p of the row in lane l lies at
//            off[s] + p * rows(s) + l (rows(s) = 64, fewer in the last slice), so a wave reads consecutive columns and
//            values per position.  A lane stops at its own length rlen[r] <= width[s]: padding slots are never read
//            by a product (they hold column 0 and value 0 so that every slot is defined).
//   width    the largest w with rows(s) * w <= 2 * sum_r min(len_r, w) (2 sum min(len, w) - rows w is concave in w, so
//            those w are an interval from 0 and a bisection finds its end): the slots of the sliced part are at most
//            twice its entries WHATEVER the row lengths, which with the 4 n + 8 (n + 1) + 12 (n / 64 + 2) bytes of
//            rlen, tptr, off and width per layout gives
//              device_bytes <= 2 (nnz(G) + nnz(G^H)) (4 + sizeof V) + 64 n + 4096
//            before the first product (the work block comes on top).  A slice of equal rows stores them whole.
//   tail     what a row has beyond width[s], as CSR (tptr, tcol, tval) in row order: the long rows of G^H (an arrowhead
//            matrix puts n entries into row 0).  After the sliced part the slice's wave takes its tail rows in
//            ascending order: lane q sums entries q, q + 64, .. ascending, the 64 partial sums are added by a butterfly
//            (partners at distance 1, 2, .., 32: the same bits in every lane) and the row's lane adds the total.
//   check    creation ends with fsap_check over the finished arrays: slice offsets and lengths inside the slot arrays,
//            row lengths within their slice, tail offsets inside the tail arrays, every column a product will read in
//            [0, ncol) (ncol = n; on a row shard n + its halo rows), the entries counted.  What it finds is a message
//            of the creating entry point through the status record.
//
// Products: grid = (slices / 4) x column tiles of kVT = 8 vectors, 4 waves (slices) per workgroup.  A lane holds kVT
// accumulators of type T and goes over the positions ascending; a column's sum never sees another column, so the bits
// of column j do not depend on m or on the tile it falls in.  W is [tile][row][kVT] of Wt (kVT * sizeof Wt is a
// multiple of 16 bytes): the first product writes, and the second gathers, whole 16-byte pieces; columns past m in
// the last tile are written as zeros and never stored to Y.  X is gathered and Y written column-major with lanes on
// consecutive rows, at element alignment.  No atomics, no LDS: the order of every sum is fixed by the layout.
//
// New values (rlh_fsvalues_plan): after the handle's values were updated on its kept pattern, fsap_fill runs again on the
// plan's kept layouts, once fsap_same_rows has found every row as long in the layout as in the handle; W and the structure stay.
//
// Row shards (rlh_fsshard_*): the same layout and the same two products on a rank's rows of G and of G^H, as the
// compile-time variant SHARD of fsap_product; the halo rows of W travel between the two products.
//
// New values on a row shard (rlh_shardvalues_*, at the end of the file): the values of both kept layouts from a builder
// handle on the shard's extended block, the own columns that higher ranks computed arriving as a packed block.  The
// plan does NOT keep the row pointers of GH_loc: they are rebuilt from rlen and tptr in scratch at every refill (one
// pass over n_own rows and a scan), so a plan holds the bytes it always held.
#include "fsai.h"
#include "spmm.h"

#include <type_traits>

namespace rlh {
namespace {

constexpr int kVT = 8;                         // vectors per column tile
constexpr int kWaves = kBlock / 64;            // slices per workgroup
constexpr int64_t kMaxTilesY = 65535;          // column tiles per launch (blockIdx.y)
enum { kErrSlice = 1, kErrLength = 2, kErrColumn = 3, kErrTail = 4 };

struct ApplyStatus : BuildStatus {
  unsigned long long entries;                  // entries the check kernel counted
};

struct bf16 { unsigned short u; };

// a stored value or an element of W as T
__device__ __forceinline__ float up(float a, float) { return a; }
__device__ __forceinline__ double up(double a, double) { return a; }
__device__ __forceinline__ double up(float a, double) { return (double)a; }
__device__ __forceinline__ c32 up(c32 a, c32) { return a; }
__device__ __forceinline__ c64 up(c64 a, c64) { return a; }
__device__ __forceinline__ c64 up(c32 a, c64) { return c64{(double)a.re, (double)a.im}; }
__device__ __forceinline__ float up(bf16 a, float) { return bf16_to_f32(a.u); }
__device__ __forceinline__ double up(bf16 a, double) { return (double)bf16_to_f32(a.u); }
// T rounded once to V or Wt (bfloat16: nearest even on the float32 bits, as rlh_bf16_pack)
__device__ __forceinline__ void down(float a, float *o) { *o = a; }
__device__ __forceinline__ void down(double a, double *o) { *o = a; }
__device__ __forceinline__ void down(double a, float *o) { *o = (float)a; }
__device__ __forceinline__ void down(c32 a, c32 *o) { *o = a; }
__device__ __forceinline__ void down(c64 a, c64 *o) { *o = a; }
__device__ __forceinline__ void down(c64 a, c32 *o) { *o = c32{(float)a.re, (float)a.im}; }
__device__ __forceinline__ void down(float a, bf16 *o) { o->u = f32_to_bf16(a); }
__device__ __forceinline__ void down(double a, bf16 *o) { o->u = f32_to_bf16((float)a); }

__device__ __forceinline__ int64_t wave_sum(int64_t v) {
  for (int o = 1; o < 64; o <<= 1) v += (int64_t)__shfl_xor((long long)v, o, 64);
  return v;
}
__device__ __forceinline__ int64_t wave_max(int64_t v) {
  for (int o = 1; o < 64; o <<= 1) {
    const int64_t w = (int64_t)__shfl_xor((long long)v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}
__device__ __forceinline__ int64_t lane_value(int64_t v, int src) { return (int64_t)__shfl((long long)v, src, 64); }

// the sum over the wave's lanes, partners at distance 1, 2, .., 32: the same bits in every lane
__device__ __forceinline__ float wave_total(float v) {
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_total(double v) {
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ c32 wave_total(c32 v) { return c32{wave_total(v.re), wave_total(v.im)}; }
__device__ __forceinline__ c64 wave_total(c64 v) { return c64{wave_total(v.re), wave_total(v.im)}; }

__device__ __forceinline__ int rows_of(int64_t n, int64_t s) { return (int)(n - s * 64 < 64 ? n - s * 64 : 64); }

// ---------------------------------------------------------------- the layout, built from CSR
// per slice its width and slots, per row its sliced length and the entries left to the tail (one wave per slice)
__global__ __launch_bounds__(kBlock) void fsap_widths(int64_t n, int64_t slices, const int64_t *__restrict__ ip,
                                                      int32_t *__restrict__ width, int64_t *__restrict__ slots,
                                                      int32_t *__restrict__ rlen, int64_t *__restrict__ tcnt) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * kWaves;
  for (int64_t s = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); s < slices; s += waves) {
    const int64_t r = s * 64 + lane, rows = rows_of(n, s);
    const int64_t len = r < n ? ip[r + 1] - ip[r] : 0;
    int64_t lo = 0, hi = wave_max(len);
    while (lo < hi) {                                  // (lo, hi are the wave's: every lane takes the same turns)
      const int64_t mid = lo + (hi - lo + 1) / 2;
      if (rows * mid <= 2 * wave_sum(len < mid ? len : mid)) lo = mid; else hi = mid - 1;
    }
    if (r < n) {
      const int64_t kept = len < lo ? len : lo;
      rlen[r] = (int32_t)kept;
      tcnt[r] = len - kept;
    }
    if (lane == 0) {
      width[s] = (int32_t)lo;
      slots[s] = rows * lo;
    }
  }
}

struct LayoutView {
  int64_t n, ncol, slices, slots, tail;  // ncol: the columns a product may read, [0, ncol) (n, or n + halo rows on a shard)
  const int64_t *off;            // slices + 1: where a slice begins in col / val
  const int32_t *width;          // slices
  const int32_t *rlen;           // n: entries of the row in the sliced part
  const int64_t *tptr;           // n + 1: the row's entries in tcol / tval
  const int32_t *col, *tcol;
  const void *val, *tval;
};

template <typename T, typename V>
__global__ __launch_bounds__(kBlock) void fsap_fill(LayoutView L, const int64_t *__restrict__ ip, const int32_t *__restrict__ ix,
                                                    const T *__restrict__ va, int32_t *__restrict__ col, V *__restrict__ val,
                                                    int32_t *__restrict__ tcol, V *__restrict__ tval) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * kWaves;
  for (int64_t s = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); s < L.slices; s += waves) {
    const int64_t r = s * 64 + lane, rows = rows_of(L.n, s), base = L.off[s];
    const bool live = r < L.n;
    const int64_t w = L.width[s], my = live ? L.rlen[r] : 0, k0 = live ? ip[r] : 0;
    if (live) {
      for (int64_t p = 0; p < w; ++p) {
        const int64_t slot = base + p * rows + lane;
        V v{};
        if (p < my) down(va[k0 + p], &v);
        col[slot] = p < my ? ix[k0 + p] : 0;
        val[slot] = v;
      }
    }
    // the tails of the slice's rows, each copied by the whole wave
    const int64_t t0 = live ? L.tptr[r] : 0, tc = live ? ip[r + 1] - k0 - my : 0;
    unsigned long long todo = __ballot(tc > 0);
    while (todo) {
      const int t = __ffsll(todo) - 1;
      todo &= todo - 1;
      const int64_t src = lane_value(k0 + my, t), dst = lane_value(t0, t), cnt = lane_value(tc, t);
      for (int64_t e = lane; e < cnt; e += 64) {
        tcol[dst + e] = ix[src + e];
        down(va[src + e], &tval[dst + e]);
      }
    }
  }
}

// The finished layout as a product will walk it: nothing is read before the offsets that lead to it are known to lie
// inside the arrays (slots and tail are the sizes the arrays were allocated with).
__global__ __launch_bounds__(kBlock) void fsap_check(LayoutView L, ApplyStatus *st) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * kWaves;
  for (int64_t s = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); s < L.slices; s += waves) {
    const int64_t r = s * 64 + lane, rows = rows_of(L.n, s), base = L.off[s], next = L.off[s + 1], w = L.width[s];
    const bool live = r < L.n;
    if (base < 0 || w < 0 || next - base != rows * w || next > L.slots || (s == 0 && base != 0) ||
        (s == L.slices - 1 && next != L.slots)) {
      if (lane == 0) build_error(st, kErrSlice, s);
      continue;                                        // (the wave's decision: the operands are the slice's)
    }
    int64_t my = live ? L.rlen[r] : 0;
    if (my < 0 || my > w) {
      build_error(st, kErrLength, r);
      my = 0;
    }
    for (int64_t p = 0; p < my; ++p) {
      const int64_t c = L.col[base + p * rows + lane];
      if (c < 0 || c >= L.ncol) build_error(st, kErrColumn, r);
    }
    int64_t t0 = live ? L.tptr[r] : 0, tc = live ? L.tptr[r + 1] - t0 : 0;
    if (t0 < 0 || tc < 0 || t0 + tc > L.tail || (r == 0 && t0 != 0) || (r == L.n - 1 && t0 + tc != L.tail)) {
      build_error(st, kErrTail, r);
      tc = 0;
    }
    unsigned long long todo = __ballot(tc > 0);
    while (todo) {
      const int t = __ffsll(todo) - 1;
      todo &= todo - 1;
      const int64_t b = lane_value(t0, t), cnt = lane_value(tc, t);
      for (int64_t e = lane; e < cnt; e += 64) {
        const int64_t c = L.tcol[b + e];
        if (c < 0 || c >= L.ncol) build_error(st, kErrColumn, s * 64 + t);
      }
    }
    const int64_t held = wave_sum(my + tc);
    if (lane == 0) atomicAdd(&st->entries, (unsigned long long)held);
  }
}

// A kept layout against the row pointers of the matrix whose values are to refill it (rlh_fsvalues_plan): row r must
// hold as many entries, sliced part and tail together, as the matrix stores there -- then fsap_fill stays inside both
constexpr int kRefillBlocksPerCu = 8;
__global__ __launch_bounds__(kBlock) void fsap_same_rows(LayoutView L, const int64_t *__restrict__ ip, ApplyStatus *st) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < L.n; r += stride)
    if (ip[r + 1] - ip[r] != (int64_t)L.rlen[r] + (L.tptr[r + 1] - L.tptr[r])) build_error(st, kErrLength, r);
}

// ---------------------------------------------------------------- the products
template <typename Wt> struct alignas(16) WRow { Wt e[kVT]; };

// What a product on a row shard (rlh_fsshard_*) has beyond the whole matrix: columns from L.n on are rows of the
// x-halo block XH (first product), and W has wstride >= L.n rows per tile, the halo rows behind the own ones.
struct ShardView {
  const void *XH;
  int64_t ldxh, wstride;
};

// acc[k] += v * (column j0 + k of the operand at row c): the first product gathers X column-major (SHARD: row c - n_own
// of XH where c >= n_own), the second a row of W
template <typename T, typename Wt, bool FIRST, bool SHARD>
__device__ __forceinline__ void gather(T (&acc)[kVT], T v, int64_t c, int mt, const T *__restrict__ X, int64_t ldx,
                                       const WRow<Wt> *__restrict__ W, int64_t n_own, const T *__restrict__ XH, int64_t ldxh) {
  if constexpr (FIRST && SHARD) {
    const bool own = c < n_own;
    const T *src = own ? X + c : XH + (c - n_own);
    const int64_t ld = own ? ldx : ldxh;
#pragma unroll
    for (int k = 0; k < kVT; ++k)
      if (k < mt) fma_acc(acc[k], v, src[k * ld]);
  } else if constexpr (FIRST) {
#pragma unroll
    for (int k = 0; k < kVT; ++k)
      if (k < mt) fma_acc(acc[k], v, X[c + k * ldx]);
  } else {
    const WRow<Wt> w = W[c];
#pragma unroll
    for (int k = 0; k < kVT; ++k) fma_acc(acc[k], v, up(w.e[k], T()));
  }
}

// FIRST: Wout = G X (X: the block from column tile0 * kVT on, mt valid columns in a tile); else Y = G^H Win.
// Wout / Win: the rows of tile tile0 on.  SHARD: the products of a row shard (ShardView); without it sv is not looked at.
template <typename T, typename V, typename Wt, bool FIRST, bool SHARD = false>
__global__ __launch_bounds__(kBlock) void fsap_product(LayoutView L, int64_t m, const T *__restrict__ X, int64_t ldx,
                                                       const WRow<Wt> *__restrict__ Win, WRow<Wt> *__restrict__ Wout,
                                                       T *__restrict__ Y, int64_t ldy, ShardView sv) {
  const int lane = threadIdx.x & 63;
  const int64_t s = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (s >= L.slices) return;
  const int64_t tile = blockIdx.y, j0 = tile * kVT;
  const int mt = (int)(m - j0 < kVT ? m - j0 : kVT);
  const int64_t r = s * 64 + lane, rows = rows_of(L.n, s);
  const bool live = r < L.n;
  const int w = L.width[s], my = live ? L.rlen[r] : 0;
  const int32_t *col = L.col + L.off[s] + lane;
  const V *val = (const V *)L.val + L.off[s] + lane;
  const T *x = FIRST ? X + j0 * ldx : nullptr;
  const int64_t wstride = SHARD ? sv.wstride : L.n;
  const WRow<Wt> *win = FIRST ? nullptr : Win + tile * wstride;
  const T *xh = SHARD && FIRST && sv.XH ? (const T *)sv.XH + j0 * sv.ldxh : nullptr;
  T acc[kVT];
#pragma unroll
  for (int k = 0; k < kVT; ++k) acc[k] = zero_of(T());
  for (int p = 0; p < w; ++p)
    if (p < my) gather<T, Wt, FIRST, SHARD>(acc, up(val[p * rows], T()), (int64_t)col[p * rows], mt, x, ldx, win, L.n, xh, sv.ldxh);
  // the tail rows of the slice in ascending order, each by the whole wave
  const int64_t t0 = live ? L.tptr[r] : 0, tc = live ? L.tptr[r + 1] - t0 : 0;
  unsigned long long todo = __ballot(tc > 0);
  while (todo) {
    const int t = __ffsll(todo) - 1;
    todo &= todo - 1;
    const int64_t b = lane_value(t0, t), cnt = lane_value(tc, t);
    T part[kVT];
#pragma unroll
    for (int k = 0; k < kVT; ++k) part[k] = zero_of(T());
    for (int64_t e = lane; e < cnt; e += 64)
      gather<T, Wt, FIRST, SHARD>(part, up(((const V *)L.tval)[b + e], T()), (int64_t)L.tcol[b + e], mt, x, ldx, win, L.n, xh,
                                  sv.ldxh);
#pragma unroll
    for (int k = 0; k < kVT; ++k) {
      const T total = wave_total(part[k]);
      if (lane == t) acc[k] = add_of(acc[k], total);
    }
  }
  if (!live) return;
  if constexpr (FIRST) {
    WRow<Wt> out;
#pragma unroll
    for (int k = 0; k < kVT; ++k) down(acc[k], &out.e[k]);
    Wout[tile * wstride + r] = out;
  } else {
#pragma unroll
    for (int k = 0; k < kVT; ++k)
      if (k < mt) Y[r + (j0 + k) * ldy] = acc[k];
  }
}

// ---------------------------------------------------------------- the host side
struct Layout {
  int64_t n = 0, ncol = 0, slices = 0, slots = 0, tail = 0;
  int64_t nnz = 0;                   // entries of the matrix it was built from
  DevBuf<int64_t> off, tptr;
  DevBuf<int32_t> width, rlen, col, tcol;
  DevBuf<void> val, tval;
  LayoutView view() const { return LayoutView{n, ncol, slices, slots, tail, off, width, rlen, tptr, col, tcol, val, tval}; }
  int64_t bytes() const {
    return (int64_t)(off.bytes() + tptr.bytes() + width.bytes() + rlen.bytes() + col.bytes() + tcol.bytes() + val.bytes() +
                     tval.bytes());
  }
};

int report(const ApplyStatus &s, const char *which, int64_t nnz, const char *entry) {
  const int code = (int)(s.err >> 56);
  const long long pos = (long long)(s.err & (((unsigned long long)1 << 56) - 1));
  switch (code) {
    case kErrSlice: set_error("%s: broken layout of %s: slice %lld does not lie inside its array", entry, which, pos); break;
    case kErrLength: set_error("%s: broken layout of %s: row %lld is longer than its slice", entry, which, pos); break;
    case kErrColumn: set_error("%s: broken layout of %s: column index out of range in row %lld", entry, which, pos); break;
    case kErrTail: set_error("%s: broken layout of %s: the tail of row %lld does not lie inside its array", entry, which, pos); break;
    default:
      set_error("%s: broken layout of %s: it holds %llu entries, the matrix %lld", entry, which, s.entries, (long long)nnz);
  }
  return 1;
}

// columns and values (rounded once to V) of the CSR arrays a into the slots and tails of a layout whose structure stands
template <typename T, typename V> void fill_layout(Layout &L, const SpdArrays &a) {
  hipLaunchKernelGGL((fsap_fill<T, V>), dim3(blocks_for(L.slices, kWaves, 1 << 20)), dim3(kBlock), 0, ctx().stream, L.view(), a.indptr,
                     a.idx, (const T *)a.val, L.col.get(), (V *)L.val.get(), L.tcol.get(), (V *)L.tval.get());
}

// The layout of one orientation (a: its CSR arrays in device memory, `which` names it and `entry` the entry point in
// messages).
template <typename T, typename V> int build_layout(Layout &L, const SpdArrays &a, const char *which, const char *entry) {
  hipStream_t st = ctx().stream;
  const dim3 blk(kBlock);
  const int64_t n = a.rows, slices = (n + 63) / 64;
  const unsigned grid = blocks_for(slices, kWaves, 1 << 20);
  L.n = n;
  L.ncol = a.cols;
  L.slices = slices;
  L.nnz = a.nnz;
  if (int rc = L.off.alloc(slices + 1)) return rc;
  if (int rc = L.width.alloc(slices)) return rc;
  if (int rc = L.rlen.alloc(n)) return rc;
  if (int rc = L.tptr.alloc(n + 1)) return rc;
  DevBuf<int64_t> slots, tcnt, bsum;
  DevBuf<ApplyStatus> status;
  if (int rc = slots.alloc(slices)) return rc;
  if (int rc = tcnt.alloc(n)) return rc;
  if (int rc = bsum.alloc((n + kScanTile - 1) / kScanTile + 1)) return rc;
  if (int rc = status.alloc(1)) return rc;
  hipLaunchKernelGGL(fsap_widths, dim3(grid), blk, 0, st, n, slices, a.indptr, L.width.get(), slots.get(), L.rlen.get(), tcnt.get());
  RLH_HIP(hipGetLastError());
  if (int rc = exclusive_scan(slices, slots, bsum, L.off)) return rc;
  if (int rc = exclusive_scan(n, tcnt, bsum, L.tptr)) return rc;
  RLH_HIP(hipMemcpyAsync(&L.slots, L.off + slices, 8, hipMemcpyDeviceToHost, st));
  RLH_HIP(hipMemcpyAsync(&L.tail, L.tptr + n, 8, hipMemcpyDeviceToHost, st));
  RLH_HIP(hipStreamSynchronize(st));
  RLH_REQUIRE(L.slots >= 0 && L.tail >= 0 && L.tail <= a.nnz && L.slots <= 2 * (a.nnz - L.tail),
              "%s: inconsistent slot counts of %s", entry, which);
  if (L.slots) {
    if (int rc = L.col.alloc(L.slots)) return rc;
    if (int rc = L.val.alloc((size_t)L.slots * sizeof(V))) return rc;
  }
  if (L.tail) {
    if (int rc = L.tcol.alloc(L.tail)) return rc;
    if (int rc = L.tval.alloc((size_t)L.tail * sizeof(V))) return rc;
  }
  fill_layout<T, V>(L, a);
  ApplyStatus hs{};
  hs.err = kNoError;
  RLH_HIP(hipMemcpyAsync(status, &hs, sizeof hs, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(fsap_check, dim3(grid), blk, 0, st, L.view(), status.get());
  RLH_HIP(hipGetLastError());
  RLH_HIP(hipMemcpyAsync(&hs, status, sizeof hs, hipMemcpyDeviceToHost, st));
  RLH_HIP(hipStreamSynchronize(st));           // the handle's arrays and the scratch are not referenced after the return
  if (hs.err != kNoError || (int64_t)hs.entries != a.nnz) return report(hs, which, a.nnz, entry);
  return 0;
}

}  // namespace

// The plan behind both families of entry points.  A row shard (rlh_fsshard_*) holds G_loc (the shard's rows of G;
// columns: own rows, then the rows of the x-halo block) and GH_loc (the shard's rows of G^H; columns: own rows, then the
// halo rows of W); W is [tile][n_own + n_whalo][kVT], its halo rows placed between the products from what the owners
// packed.  The whole matrix (rlh_fsapply_*) is the plan with n_own = n and no halo rows: it launches the products
// without SHARD and does not look at m_first / placed.
struct FsPlan {
  int dtype = 0, work = 0;
  int64_t n_own = 0, n_xhalo = 0, n_whalo = 0;
  int64_t m_first = -1, placed = 0;  // the vectors of the last rlh_fsshard_first (-1: none yet), the halo rows placed since
  int64_t refills = 0;               // rlh_shardvalues_refill: the successful ones and the device seconds of the last
  double refill_seconds = 0;
  Layout g, gh;                      // G for the first product, G^H for the second
  DevBuf<char> w;                    // W = G X
  int64_t wrows() const { return n_own + n_whalo; }
};

}  // namespace rlh

struct rlh_fsapply : rlh::FsPlan {};
struct rlh_fsshard : rlh::FsPlan {};

namespace rlh {
namespace {

// f(T(), V(), Wt()) for the types of a plan: the one place that maps (dtype, work) to them
template <typename F> int with_types(int dtype, int work, F f) {
  switch (dtype) {
    case RLH_S: return work == 2 ? f(float(), float(), bf16()) : f(float(), float(), float());
    case RLH_D: return work == 2 ? f(double(), float(), bf16()) : work == 1 ? f(double(), float(), float()) : f(double(), double(), double());
    case RLH_C: return f(c32(), c32(), c32());
    default: return work ? f(c64(), c32(), c32()) : f(c64(), c64(), c64());
  }
}

// bytes of one element of W
int64_t w_elem_bytes(const FsPlan *p) {
  return with_types(p->dtype, p->work, [](auto, auto, auto w) { return (int)sizeof(w); });
}

int check_work(const char *entry, int dtype, int work) {
  RLH_REQUIRE(work >= 0 && work <= 2, "%s: work must be 0 (native), 1 (float32) or 2 (bf16), got %d", entry, work);
  RLH_REQUIRE(work != 2 || dtype == RLH_S || dtype == RLH_D, "%s: bfloat16 work blocks are for real types only", entry);
  return 0;
}

// f(t0, nt) for the column tiles [t0, t0 + nt) of each launch: blockIdx.y takes at most kMaxTilesY of them
template <typename F> void for_tile_chunks(int64_t tiles, F f) {
  for (int64_t t0 = 0; t0 < tiles; t0 += kMaxTilesY) f(t0, tiles - t0 < kMaxTilesY ? tiles - t0 : kMaxTilesY);
}

// One product on all column tiles of m vectors.  FIRST: W = L [X ; XH], else Y = L W; W has wstride rows per tile.  The
// operands of the other product are not looked at, XH and ldxh (null: no halo block) by a SHARD product alone.
template <typename T, typename V, typename Wt, bool FIRST, bool SHARD>
int launch_product(const Layout &L, int64_t m, const T *X, int64_t ldx, WRow<Wt> *W, int64_t wstride, T *Y, int64_t ldy,
                   const T *XH, int64_t ldxh) {
  const unsigned gx = (unsigned)((L.slices + kWaves - 1) / kWaves);
  if (!gx) return 0;                                   // (a shard may own no rows)
  for_tile_chunks((m + kVT - 1) / kVT, [&](int64_t t0, int64_t nt) {
    const int64_t j0 = t0 * kVT;
    WRow<Wt> *w = W + t0 * wstride;
    const ShardView sv = SHARD ? ShardView{XH ? XH + j0 * ldxh : nullptr, ldxh, wstride} : ShardView{};
    if constexpr (FIRST)
      hipLaunchKernelGGL((fsap_product<T, V, Wt, true, SHARD>), dim3(gx, (unsigned)nt), dim3(kBlock), 0, ctx().stream, L.view(),
                         m - j0, X + j0 * ldx, ldx, (const WRow<Wt> *)nullptr, w, (T *)nullptr, (int64_t)0, sv);
    else
      hipLaunchKernelGGL((fsap_product<T, V, Wt, false, SHARD>), dim3(gx, (unsigned)nt), dim3(kBlock), 0, ctx().stream, L.view(),
                         m - j0, (const T *)nullptr, (int64_t)0, (const WRow<Wt> *)w, (WRow<Wt> *)nullptr, Y + j0 * ldy, ldy, sv);
  });
  RLH_HIP(hipGetLastError());
  return 0;
}

// W = G [X ; XH] of the plan, W grown to the block's tiles first
template <bool SHARD> int first_product(FsPlan *p, int64_t m, const void *X, int64_t ldx, const void *XH, int64_t ldxh) {
  return with_types(p->dtype, p->work, [&](auto t, auto v, auto w) {
    using T = decltype(t);
    using Wt = decltype(w);
    const int64_t tiles = (m + kVT - 1) / kVT;
    if (int rc = p->w.reserve((size_t)tiles * (size_t)p->wrows() * sizeof(WRow<Wt>))) return rc;   // grows once per wider block
    return launch_product<T, decltype(v), Wt, true, SHARD>(p->g, m, (const T *)X, ldx, (WRow<Wt> *)p->w.get(), p->wrows(),
                                                           (T *)nullptr, 0, (const T *)XH, ldxh);
  });
}

// Y = G^H W of the plan
template <bool SHARD> int second_product(FsPlan *p, int64_t m, void *Y, int64_t ldy) {
  return with_types(p->dtype, p->work, [&](auto t, auto v, auto w) {
    using T = decltype(t);
    using Wt = decltype(w);
    return launch_product<T, decltype(v), Wt, false, SHARD>(p->gh, m, (const T *)nullptr, 0, (WRow<Wt> *)p->w.get(), p->wrows(),
                                                            (T *)Y, ldy, (const T *)nullptr, 0);
  });
}

template <typename P> int plan_destroy(P *p) {
  if (!p) return 0;
  if (ctx().ready) (void)hipStreamSynchronize(ctx().stream);
  delete p;
  return 0;
}

// A new plan of the handle type P: build(p) makes its layouts; *pp is set when that succeeds
template <typename P, typename Build>
int make_plan(P **pp, int dtype, int work, int64_t n_own, int64_t n_xhalo, int64_t n_whalo, Build build) {
  P *p = new P();
  p->dtype = dtype;
  p->work = work;
  p->n_own = n_own;
  p->n_xhalo = n_xhalo;
  p->n_whalo = n_whalo;
  if (int rc = build(p)) {
    plan_destroy(p);
    return rc;
  }
  *pp = p;
  return 0;
}

int plan_info(const char *entry, const FsPlan *p, int *work, int64_t *stored_slots, int64_t *tail_entries, int64_t *device_bytes) {
  RLH_REQUIRE(p, "%s: null plan", entry);
  if (work) *work = p->work;
  if (stored_slots) *stored_slots = p->g.slots + p->gh.slots;
  if (tail_entries) *tail_entries = p->g.tail + p->gh.tail;
  if (device_bytes) *device_bytes = p->g.bytes() + p->gh.bytes() + (int64_t)p->w.bytes();
  return 0;
}

}  // namespace
}  // namespace rlh

using namespace rlh;

extern "C" int rlh_fsapply_create(rlh_fsapply_t *pp, rlh_fsai_t h, int work) {
  constexpr const char *kEntry = "rlh_fsapply_create";
  if (int rc = require_ready()) return rc;
  RLH_REQUIRE(pp != nullptr, "rlh_fsapply_create: null plan pointer");
  *pp = nullptr;
  RLH_REQUIRE(h != nullptr, "rlh_fsapply_create: null handle");
  if (int rc = check_work(kEntry, h->dtype, work)) return rc;
  return make_plan(pp, h->dtype, work, h->n, 0, 0, [&](FsPlan *p) {
    if (h->n == 0 || !h->spd) return 0;
    return with_types(h->dtype, work, [&](auto t, auto v, auto) {
      using T = decltype(t);
      using V = decltype(v);
      if (int rc = build_layout<T, V>(p->g, spd_arrays(h->spd, 0), "G", kEntry)) return rc;
      return build_layout<T, V>(p->gh, spd_arrays(h->spd, 1), "G^H", kEntry);
    });
  });
}

extern "C" int rlh_fsapply_run(rlh_fsapply_t p, int64_t m, const void *X, int64_t ldx, void *Y, int64_t ldy) {
  if (int rc = require_ready()) return rc;
  RLH_REQUIRE(p, "rlh_fsapply_run: null plan");
  RLH_REQUIRE(m >= 0, "rlh_fsapply_run: negative number of vectors");
  if (m == 0 || p->n_own == 0) return 0;
  RLH_REQUIRE(X && Y, "rlh_fsapply_run: null pointer");
  RLH_REQUIRE(ldx >= p->n_own && ldy >= p->n_own, "rlh_fsapply_run: Matrix and vectors dimensions incompatible");
  if (int rc = first_product<false>(p, m, X, ldx, nullptr, 0)) return rc;
  return second_product<false>(p, m, Y, ldy);
}

extern "C" int rlh_fsapply_info(rlh_fsapply_t p, int *work, int64_t *stored_slots, int64_t *tail_entries, int64_t *device_bytes) {
  return plan_info("rlh_fsapply_info", p, work, stored_slots, tail_entries, device_bytes);
}

extern "C" int rlh_fsapply_destroy(rlh_fsapply_t p) { return plan_destroy(p); }

namespace rlh {
namespace {

// the values of a (and its columns, which are the layout's own) into a layout made from a matrix of the same rows
template <typename T, typename V> int refill_layout(Layout &L, const SpdArrays &a, const char *which, const char *entry) {
  hipStream_t st = ctx().stream;
  DevBuf<ApplyStatus> status;
  if (int rc = status.alloc(1)) return rc;
  ApplyStatus hs{};
  hs.err = kNoError;
  RLH_HIP(hipMemcpyAsync(status, &hs, sizeof hs, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(fsap_same_rows, dim3(blocks_for(L.n, kBlock, (int64_t)ctx().num_cu * kRefillBlocksPerCu)), dim3(kBlock), 0, st,
                     L.view(), a.indptr, status.get());
  RLH_HIP(hipGetLastError());
  RLH_HIP(hipMemcpyAsync(&hs, status, sizeof hs, hipMemcpyDeviceToHost, st));
  RLH_HIP(hipStreamSynchronize(st));
  if (hs.err != kNoError) {
    set_error("%s: row %lld of %s has another length in the plan than in the handle", entry,
              (long long)(hs.err & (((unsigned long long)1 << 56) - 1)), which);
    return 1;
  }
  fill_layout<T, V>(L, a);
  RLH_HIP(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace rlh

extern "C" int rlh_fsvalues_plan(rlh_fsapply_t p, rlh_fsai_t h) {
  constexpr const char *kEntry = "rlh_fsvalues_plan";
  if (int rc = require_ready()) return rc;
  RLH_REQUIRE(p != nullptr, "%s: null plan", kEntry);
  RLH_REQUIRE(h != nullptr, "%s: null handle", kEntry);
  RLH_REQUIRE(p->dtype == h->dtype, "%s: the plan's dtype (%d) is not the handle's (%d)", kEntry, p->dtype, h->dtype);
  RLH_REQUIRE(p->n_own == h->n, "%s: the plan has %lld rows, the handle %lld", kEntry, (long long)p->n_own, (long long)h->n);
  if (h->n == 0 || !h->spd) return 0;
  const SpdArrays g = spd_arrays(h->spd, 0), gh = spd_arrays(h->spd, 1);
  RLH_REQUIRE(p->g.nnz == g.nnz && p->gh.nnz == gh.nnz, "%s: the plan holds %lld entries of G, the handle %lld", kEntry,
              (long long)p->g.nnz, (long long)g.nnz);
  return with_types(p->dtype, p->work, [&](auto t, auto v, auto) {
    using T = decltype(t);
    using V = decltype(v);
    if (int rc = refill_layout<T, V>(p->g, g, "G", kEntry)) return rc;
    return refill_layout<T, V>(p->gh, gh, "G^H", kEntry);
  });
}

// ---------------------------------------------------------------- the application on a row shard (rlh_fsshard_*)
namespace rlh {
namespace {

// dst row (drow0 + i) of tile t <- src row (idx ? idx[i] : i) of tile t, i < nrows, as 16-byte pieces (`pieces` per row;
// the strides count rows).  An index outside [0, bound) is not followed: the row is written as zeros.
__global__ __launch_bounds__(kBlock) void fsap_rows(int64_t nrows, int pieces, const int64_t *__restrict__ idx, int64_t bound,
                                                    const uint4 *__restrict__ src, int64_t sstride, uint4 *__restrict__ dst,
                                                    int64_t dstride, int64_t drow0) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x, tile = blockIdx.y;
  if (e >= nrows * pieces) return;
  const int64_t i = e / pieces, q = e - i * pieces;
  const int64_t r = idx ? idx[i] : i;
  uint4 v = make_uint4(0, 0, 0, 0);
  if (r >= 0 && r < bound) v = src[(tile * sstride + r) * pieces + q];
  dst[(tile * dstride + drow0 + i) * pieces + q] = v;
}

// fsap_rows on the tiles of m vectors of the plan's W
int move_rows(const FsPlan *p, int64_t m, int64_t nrows, const int64_t *idx, int64_t bound, const void *src, int64_t sstride,
              void *dst, int64_t dstride, int64_t drow0) {
  const int pieces = (int)(kVT * w_elem_bytes(p) / 16);
  const unsigned gx = (unsigned)((nrows * pieces + kBlock - 1) / kBlock);
  for_tile_chunks((m + kVT - 1) / kVT, [&](int64_t t0, int64_t nt) {
    hipLaunchKernelGGL(fsap_rows, dim3(gx, (unsigned)nt), dim3(kBlock), 0, ctx().stream, nrows, pieces, idx, bound,
                       (const uint4 *)src + t0 * sstride * pieces, sstride, (uint4 *)dst + t0 * dstride * pieces, dstride, drow0);
  });
  RLH_HIP(hipGetLastError());
  return 0;
}

// one orientation: the host arrays into device memory, then the layout (the uploads go when this returns)
template <typename T, typename V>
int shard_layout(Layout &L, int64_t rows, int64_t cols, const int64_t *ip, const int32_t *ix, const void *va, const char *which) {
  const int64_t nnz = ip[rows];
  DevBuf<int64_t> dip;
  DevBuf<int32_t> dix;
  DevBuf<char> dva;
  if (int rc = dip.upload(ip, (size_t)(rows + 1) * 8)) return rc;
  if (int rc = dix.upload(ix, (size_t)nnz * 4, 16)) return rc;
  if (int rc = dva.upload(va, (size_t)nnz * sizeof(T), 16)) return rc;
  SpdArrays a;
  a.rows = rows; a.cols = cols; a.nnz = nnz;
  a.indptr = dip; a.idx = dix; a.val = dva.get();
  return build_layout<T, V>(L, a, which, "rlh_fsshard_create");
}

// indptr[0] == 0 and non-decreasing
int64_t first_decrease(const int64_t *ip, int64_t rows) {
  if (ip[0] != 0) return 0;
  for (int64_t r = 0; r < rows; ++r)
    if (ip[r + 1] < ip[r]) return r + 1;
  return -1;
}

}  // namespace
}  // namespace rlh

extern "C" int rlh_fsshard_create(rlh_fsshard_t *pp, int dtype, int work, int64_t n_own, int64_t n_xhalo, int64_t n_whalo,
                                  const int64_t *g_indptr, const int32_t *g_indices, const void *g_values,
                                  const int64_t *gh_indptr, const int32_t *gh_indices, const void *gh_values) {
  if (int rc = require_ready()) return rc;
  RLH_REQUIRE(pp != nullptr, "rlh_fsshard_create: null plan pointer");
  *pp = nullptr;
  RLH_REQUIRE(dtype == RLH_S || dtype == RLH_D || dtype == RLH_C || dtype == RLH_Z, "rlh_fsshard_create: unknown dtype %d", dtype);
  if (int rc = check_work("rlh_fsshard_create", dtype, work)) return rc;
  RLH_REQUIRE(n_own >= 0 && n_xhalo >= 0 && n_whalo >= 0, "rlh_fsshard_create: negative size");
  RLH_REQUIRE(n_own + n_xhalo <= INT32_MAX && n_own + n_whalo <= INT32_MAX, "rlh_fsshard_create: more than 2^31 - 1 columns");
  RLH_REQUIRE(g_indptr && gh_indptr, "rlh_fsshard_create: null indptr");
  int64_t bad = first_decrease(g_indptr, n_own);
  RLH_REQUIRE(bad < 0, "rlh_fsshard_create: indptr of G must start at 0 and not decrease (row %lld)", (long long)(bad ? bad - 1 : 0));
  bad = first_decrease(gh_indptr, n_own);
  RLH_REQUIRE(bad < 0, "rlh_fsshard_create: indptr of G^H must start at 0 and not decrease (row %lld)", (long long)(bad ? bad - 1 : 0));
  RLH_REQUIRE((g_indptr[n_own] == 0 || (g_indices && g_values)) && (gh_indptr[n_own] == 0 || (gh_indices && gh_values)),
              "rlh_fsshard_create: null indices or values");
  return make_plan(pp, dtype, work, n_own, n_xhalo, n_whalo, [&](FsPlan *p) {
    if (n_own == 0) return 0;
    return with_types(dtype, work, [&](auto t, auto v, auto) {
      using T = decltype(t);
      using V = decltype(v);
      if (int rc = shard_layout<T, V>(p->g, n_own, n_own + n_xhalo, g_indptr, g_indices, g_values, "G")) return rc;
      return shard_layout<T, V>(p->gh, n_own, n_own + n_whalo, gh_indptr, gh_indices, gh_values, "G^H");
    });
  });
}

extern "C" int rlh_fsshard_first(rlh_fsshard_t p, int64_t m, const void *X, int64_t ldx, const void *XH, int64_t ldxh) {
  if (int rc = require_ready()) return rc;
  RLH_REQUIRE(p, "rlh_fsshard_first: null plan");
  RLH_REQUIRE(m >= 0, "rlh_fsshard_first: negative number of vectors");
  if (m > 0 && p->n_own > 0) {
    RLH_REQUIRE(X, "rlh_fsshard_first: null pointer");
    RLH_REQUIRE(XH || p->n_xhalo == 0, "rlh_fsshard_first: null halo block with %lld halo rows", (long long)p->n_xhalo);
    RLH_REQUIRE(ldx >= p->n_own && (!XH || ldxh >= p->n_xhalo), "rlh_fsshard_first: Matrix and vectors dimensions incompatible");
  }
  p->m_first = -1;
  p->placed = 0;
  if (m > 0)
    if (int rc = first_product<true>(p, m, X, ldx, p->n_xhalo ? XH : nullptr, ldxh)) return rc;
  p->m_first = m;
  return 0;
}

extern "C" int rlh_fsshard_pack(rlh_fsshard_t p, int64_t m, int64_t nidx, const int64_t *d_idx, void *out) {
  if (int rc = require_ready()) return rc;
  RLH_REQUIRE(p, "rlh_fsshard_pack: null plan");
  RLH_REQUIRE(m >= 0 && nidx >= 0, "rlh_fsshard_pack: negative size");
  RLH_REQUIRE(nidx <= p->n_own, "rlh_fsshard_pack: %lld rows asked of %lld own rows", (long long)nidx, (long long)p->n_own);
  RLH_REQUIRE(p->m_first == m, "rlh_fsshard_pack: no rlh_fsshard_first with %lld vectors came before", (long long)m);
  if (m == 0 || nidx == 0) return 0;
  RLH_REQUIRE(d_idx && out, "rlh_fsshard_pack: null pointer");
  return move_rows(p, m, nidx, d_idx, p->n_own, p->w.get(), p->wrows(), out, nidx, 0);
}

extern "C" int rlh_fsshard_halo(rlh_fsshard_t p, int64_t m, int64_t first, int64_t count, const void *src) {
  if (int rc = require_ready()) return rc;
  RLH_REQUIRE(p, "rlh_fsshard_halo: null plan");
  RLH_REQUIRE(m >= 0 && first >= 0 && count >= 0, "rlh_fsshard_halo: negative size");
  RLH_REQUIRE(first + count <= p->n_whalo, "rlh_fsshard_halo: rows %lld .. %lld of %lld halo rows", (long long)first,
              (long long)(first + count), (long long)p->n_whalo);
  RLH_REQUIRE(p->m_first == m, "rlh_fsshard_halo: no rlh_fsshard_first with %lld vectors came before", (long long)m);
  if (m > 0 && count > 0) {
    RLH_REQUIRE(src, "rlh_fsshard_halo: null pointer");
    if (int rc = move_rows(p, m, count, nullptr, count, src, count, p->w.get(), p->wrows(), p->n_own + first)) return rc;
  }
  p->placed += count;
  return 0;
}

extern "C" int rlh_fsshard_second(rlh_fsshard_t p, int64_t m, void *Y, int64_t ldy) {
  if (int rc = require_ready()) return rc;
  RLH_REQUIRE(p, "rlh_fsshard_second: null plan");
  RLH_REQUIRE(m >= 0, "rlh_fsshard_second: negative number of vectors");
  RLH_REQUIRE(p->m_first >= 0, "rlh_fsshard_second: no rlh_fsshard_first came before");
  RLH_REQUIRE(p->m_first == m, "rlh_fsshard_second: the last rlh_fsshard_first had %lld vectors, not %lld", (long long)p->m_first,
              (long long)m);
  RLH_REQUIRE(p->placed >= p->n_whalo, "rlh_fsshard_second: halo rows missing (%lld of %lld placed)", (long long)p->placed,
              (long long)p->n_whalo);
  if (m == 0 || p->n_own == 0) return 0;
  RLH_REQUIRE(Y, "rlh_fsshard_second: null pointer");
  RLH_REQUIRE(ldy >= p->n_own, "rlh_fsshard_second: Matrix and vectors dimensions incompatible");
  return second_product<true>(p, m, Y, ldy);
}

extern "C" int rlh_fsshard_info(rlh_fsshard_t p, int *work, int64_t *stored_slots, int64_t *tail_entries, int64_t *device_bytes,
                                int64_t *w_row_bytes) {
  if (int rc = plan_info("rlh_fsshard_info", p, work, stored_slots, tail_entries, device_bytes)) return rc;
  if (w_row_bytes) *w_row_bytes = kVT * w_elem_bytes(p);
  return 0;
}

extern "C" int rlh_fsshard_destroy(rlh_fsshard_t p) { return plan_destroy(p); }

// ---------------------------------------------------------------- new values on a row shard (rlh_shardvalues_*)
namespace rlh {
namespace {

enum { kErrSource = 5 };                      // (after kErrLength: a row of another length is reported first)

// out[i] = the handle's value at entry ip[0] + pos[i] (ip: the handle's row pointers from first_row on, `rows` rows); a
// position outside those rows' entries is not followed
template <typename T>
__global__ __launch_bounds__(kBlock) void shv_pack(int64_t count, int64_t rows, const int64_t *__restrict__ ip,
                                                   const int64_t *__restrict__ pos, const T *__restrict__ va, T *__restrict__ out) {
  const int64_t base = ip[0], entries = ip[rows] - base, stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += stride) {
    const int64_t q = pos[i];
    T v = zero_of(T());
    if (q >= 0 && q < entries) v = va[base + q];
    out[i] = v;
  }
}

// What a refill checks before it writes (one launch, one status record): the entries of the handle's rows (st->nnz),
// every row of G_loc as long in the layout as in the handle (fsap_same_rows from an offset), every source of GH_loc in
// [-n_recv, entries)
__global__ __launch_bounds__(kBlock) void shv_check(LayoutView G, const int64_t *__restrict__ ip, int64_t nsrc,
                                                    const int64_t *__restrict__ src, int64_t n_recv, ApplyStatus *st) {
  const int64_t stride = (int64_t)gridDim.x * kBlock, first = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t entries = ip[G.n] - ip[0];
  if (first == 0) st->nnz = entries;
  for (int64_t r = first; r < G.n; r += stride)
    if (ip[r + 1] - ip[r] != (int64_t)G.rlen[r] + (G.tptr[r + 1] - G.tptr[r])) build_error(st, kErrLength, r);
  for (int64_t k = first; k < nsrc; k += stride) {
    const int64_t s = src[k];
    if (s < -n_recv || s >= entries) build_error(st, kErrSource, k);
  }
}

// the entries of every row of a layout, sliced part and tail together (their scan: the row pointers of the CSR arrays
// the layout was made from)
__global__ __launch_bounds__(kBlock) void shv_row_lengths(LayoutView L, int64_t *__restrict__ len) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < L.n; r += stride)
    len[r] = (int64_t)L.rlen[r] + (L.tptr[r + 1] - L.tptr[r]);
}

// The value of entry k of the CSR arrays a layout was made from (va: the handle's values, ip: its row pointers from
// first_row on).  G_loc: the handle's entry ip[0] + k.  GH_loc: the conjugate of the handle's entry ip[0] + src[k], or of
// recv[-1 - src[k]] for a negative source -- the select and the conjugation happen on the way into the slot.
template <typename T> struct OwnValues {
  const T *va;
  const int64_t *ip;
  __device__ __forceinline__ T operator()(int64_t k) const { return va[ip[0] + k]; }
};
template <typename T> struct SourcedValues {
  const T *va;
  const int64_t *ip;
  const T *recv;
  const int64_t *src;
  __device__ __forceinline__ T operator()(int64_t k) const {
    const int64_t s = src[k];
    return dev_conj(s >= 0 ? va[ip[0] + s] : recv[-1 - s]);
  }
};

// fsap_fill for the values alone: the slots position-major within the slice, then the tails of the slice's rows by the
// whole wave; columns, padding slots and the structure are not touched.  rp: the row pointers of the CSR order (those of
// the handle from first_row on for G_loc, the scan of shv_row_lengths for GH_loc); entry k of row r is rp[r] - rp[0] + k.
template <typename T, typename V, typename F>
__global__ __launch_bounds__(kBlock) void shv_fill(LayoutView L, const int64_t *__restrict__ rp, F value, V *__restrict__ val,
                                                   V *__restrict__ tval) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * kWaves, e0 = rp[0];
  for (int64_t s = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); s < L.slices; s += waves) {
    const int64_t r = s * 64 + lane, rows = rows_of(L.n, s), base = L.off[s];
    const bool live = r < L.n;
    const int64_t my = live ? L.rlen[r] : 0, k0 = live ? rp[r] - e0 : 0;
    for (int64_t p = 0; p < my; ++p) down(value(k0 + p), &val[base + p * rows + lane]);
    const int64_t t0 = live ? L.tptr[r] : 0, tc = live ? L.tptr[r + 1] - t0 : 0;
    unsigned long long todo = __ballot(tc > 0);
    while (todo) {
      const int t = __ffsll(todo) - 1;
      todo &= todo - 1;
      const int64_t from = lane_value(k0 + my, t), dst = lane_value(t0, t), cnt = lane_value(tc, t);
      for (int64_t e = lane; e < cnt; e += 64) down(value(from + e), &tval[dst + e]);
    }
  }
}

// the grid of a refill's kernels: at most kRefillBlocksPerCu workgroups per CU, as refill_layout
unsigned refill_grid(int64_t items, int64_t per) { return blocks_for(items, per, (int64_t)ctx().num_cu * kRefillBlocksPerCu); }

}  // namespace
}  // namespace rlh

extern "C" int rlh_shardvalues_pack(rlh_fsai_t h, int64_t first_row, int64_t count, const int64_t *d_pos, void *d_out) {
  constexpr const char *kEntry = "rlh_shardvalues_pack";
  if (int rc = require_ready()) return rc;
  RLH_REQUIRE(h != nullptr, "%s: null handle", kEntry);
  RLH_REQUIRE(count >= 0, "%s: negative size", kEntry);
  RLH_REQUIRE(first_row >= 0 && first_row <= h->n, "%s: first row %lld of a handle of %lld rows", kEntry, (long long)first_row,
              (long long)h->n);
  if (count == 0) return 0;
  RLH_REQUIRE(d_pos && d_out, "%s: null pointer", kEntry);
  const int64_t room_p = bytes_from(d_pos), room_o = bytes_from(d_out);
  const int64_t es = h->dtype == RLH_S ? 4 : h->dtype == RLH_Z ? 16 : 8;
  RLH_REQUIRE((room_p < 0 || room_p >= 8 * count) && (room_o < 0 || room_o >= es * count), "%s: an array holds fewer than %lld entries",
              kEntry, (long long)count);
  if (h->n == 0 || !h->spd) {                          // no entries: every position lies outside
    RLH_HIP(hipMemsetAsync(d_out, 0, (size_t)(es * count), ctx().stream));
    return 0;
  }
  const SpdArrays g = spd_arrays(h->spd, 0);
  return with_types(h->dtype, 0, [&](auto t, auto, auto) {
    using T = decltype(t);
    hipLaunchKernelGGL(shv_pack<T>, dim3(refill_grid(count, kBlock)), dim3(kBlock), 0, ctx().stream, count, h->n - first_row,
                       g.indptr + first_row, d_pos, (const T *)g.val, (T *)d_out);
    RLH_HIP(hipGetLastError());
    return 0;
  });
}

extern "C" int rlh_shardvalues_refill(rlh_fsshard_t p, rlh_fsai_t h, int64_t first_row, const int64_t *d_src, int64_t n_recv,
                                      const void *d_recv) {
  constexpr const char *kEntry = "rlh_shardvalues_refill";
  if (int rc = require_ready()) return rc;
  RLH_REQUIRE(p != nullptr, "%s: null plan", kEntry);
  RLH_REQUIRE(h != nullptr, "%s: null handle", kEntry);
  RLH_REQUIRE(p->dtype == h->dtype, "%s: the plan's dtype (%d) is not the handle's (%d)", kEntry, p->dtype, h->dtype);
  RLH_REQUIRE(n_recv >= 0, "%s: negative size", kEntry);
  RLH_REQUIRE(first_row >= 0 && h->n - first_row == p->n_own, "%s: the plan has %lld own rows, the handle %lld from row %lld on", kEntry,
              (long long)p->n_own, (long long)(h->n - first_row), (long long)first_row);
  if (p->n_own == 0) {                                 // nothing to fill: a valid refill
    p->refill_seconds = 0;
    ++p->refills;
    return 0;
  }
  RLH_REQUIRE(h->spd != nullptr, "%s: the handle holds no matrix", kEntry);
  RLH_REQUIRE(d_src || p->gh.nnz == 0, "%s: null source list", kEntry);
  RLH_REQUIRE(d_recv || n_recv == 0, "%s: null block of received values", kEntry);
  const int64_t es = h->dtype == RLH_S ? 4 : h->dtype == RLH_Z ? 16 : 8;
  const int64_t room_s = bytes_from(d_src), room_r = bytes_from(d_recv);
  RLH_REQUIRE(room_s < 0 || room_s >= 8 * p->gh.nnz, "%s: the source list holds fewer than the %lld entries of G^H", kEntry,
              (long long)p->gh.nnz);
  RLH_REQUIRE(room_r < 0 || room_r >= es * n_recv, "%s: the block of received values holds fewer than %lld", kEntry, (long long)n_recv);
  const SpdArrays g = spd_arrays(h->spd, 0);
  const int64_t *ip = g.indptr + first_row;            // rows first_row .. n of the handle's G: the plan's G_loc
  hipStream_t st = ctx().stream;
  const int64_t n = p->n_own;
  StreamTimer timer;
  if (int rc = timer.start()) return rc;
  DevBuf<ApplyStatus> status;
  DevBuf<int64_t> len, bsum, hp;
  if (int rc = status.alloc(1)) return rc;
  if (int rc = len.alloc(n)) return rc;
  if (int rc = bsum.alloc((n + kScanTile - 1) / kScanTile + 1)) return rc;
  if (int rc = hp.alloc(n + 1)) return rc;
  // ---- every check before any write to the plan; the one synchronisation for the status
  ApplyStatus hs{};
  hs.err = kNoError;
  RLH_HIP(hipMemcpyAsync(status, &hs, sizeof hs, hipMemcpyHostToDevice, st));
  const int64_t most = n > p->gh.nnz ? n : p->gh.nnz;
  hipLaunchKernelGGL(shv_check, dim3(refill_grid(most, kBlock)), dim3(kBlock), 0, st, p->g.view(), ip, p->gh.nnz, d_src, n_recv,
                     status.get());
  RLH_HIP(hipGetLastError());
  RLH_HIP(hipMemcpyAsync(&hs, status, sizeof hs, hipMemcpyDeviceToHost, st));
  RLH_HIP(hipStreamSynchronize(st));
  RLH_REQUIRE((int64_t)hs.nnz == p->g.nnz, "%s: the plan holds %lld entries of G, the handle %lld from row %lld on", kEntry,
              (long long)p->g.nnz, (long long)hs.nnz, (long long)first_row);
  if (hs.err != kNoError) {
    const long long pos = (long long)(hs.err & kPosMask);
    if ((int)(hs.err >> 56) == kErrLength)
      set_error("%s: row %lld of G has another length in the plan than in the handle", kEntry, pos);
    else
      set_error("%s: entry %lld of G^H has its source outside [-%lld, %lld)", kEntry, pos, (long long)n_recv, (long long)hs.nnz);
    return 1;
  }
  // ---- the row pointers of GH_loc, then the values of both layouts
  hipLaunchKernelGGL(shv_row_lengths, dim3(refill_grid(n, kBlock)), dim3(kBlock), 0, st, p->gh.view(), len.get());
  RLH_HIP(hipGetLastError());
  if (int rc = exclusive_scan(n, len, bsum, hp)) return rc;
  if (int rc = with_types(p->dtype, p->work, [&](auto t, auto v, auto) {
        using T = decltype(t);
        using V = decltype(v);
        const T *va = (const T *)g.val;
        const dim3 grid(refill_grid(p->g.slices, kWaves));
        hipLaunchKernelGGL((shv_fill<T, V, OwnValues<T>>), grid, dim3(kBlock), 0, st, p->g.view(), ip, OwnValues<T>{va, ip}, (V *)p->g.val.get(),
                           (V *)p->g.tval.get());
        hipLaunchKernelGGL((shv_fill<T, V, SourcedValues<T>>), grid, dim3(kBlock), 0, st, p->gh.view(), (const int64_t *)hp.get(),
                           SourcedValues<T>{va, ip, (const T *)d_recv, d_src}, (V *)p->gh.val.get(), (V *)p->gh.tval.get());
        RLH_HIP(hipGetLastError());
        return 0;
      }))
    return rc;
  if (int rc = timer.stop()) return rc;                // the handle's arrays, the caller's and the scratch are not referenced after the return
  p->refill_seconds = timer.seconds();
  ++p->refills;
  return 0;
}

extern "C" int rlh_shardvalues_info(rlh_fsshard_t p, int64_t *updates, double *seconds) {
  RLH_REQUIRE(p != nullptr, "rlh_shardvalues_info: null plan");
  if (updates) *updates = p->refills;
  if (seconds) *seconds = p->refill_seconds;
  return 0;
}
