// Pieces shared by everything that is built by kernels from CSR arrays already in device memory (rlh_spd_create_device:
// spmm_data.hip, rlh_csr_create_device: spmm_build_device.hip, the approximate inverse and its updates: fsai.hip).
// The checked input: the status record the host fetches once, the checks of indptr and of the columns, the messages of
// what they find, and indptr / columns as int64 / int32 -- as separate steps, so that a builder can enqueue checks of
// its own on the same record before the one synchronisation.  Then the exclusive scan, the timing events of a build and
// two host helpers.  The kernels sit in an unnamed namespace: every translation unit that includes this file gets its
// own copies.
#pragma once

#include "common.h"

#include <algorithm>
#include <type_traits>

namespace rlh {
namespace {

constexpr int kBlock = 256;

struct BuildStatus {
  unsigned long long err;         // ~0: none; else (code << 56) | position, the smallest of all found
  long long nnz;                  // indptr[n_rows]
};
// the record of a builder that can report an entry without its partner on the other side of the diagonal
struct PartnerStatus : BuildStatus {
  long long row, col;             // row and column of that entry (resolve_partner)
};
// The smallest code wins (build_error), so the order of the codes is behaviour.  6 is left to a check of a builder's own
// that has to win over a missing partner (the approximate inverse: a row without its diagonal); a builder's other codes
// come after kErrPartner.
enum { kErrFirst = 1, kErrDecreasing = 2, kErrLast = 3, kErrRange = 4, kErrOrder = 5, kErrPartner = 7 };
constexpr unsigned long long kNoError = ~0ull;
constexpr unsigned long long kPosMask = ((unsigned long long)1 << 56) - 1;

__device__ __forceinline__ void build_error(BuildStatus *st, int code, int64_t pos) {
  atomicMin(&st->err, ((unsigned long long)code << 56) | (unsigned long long)pos);
}

// a kernel after the first returns at once when the record already holds an error: none reads through an index that
// failed its check
__device__ __forceinline__ bool failed(const BuildStatus *st) { return *(const volatile unsigned long long *)&st->err != kNoError; }

// The same for a kernel that records errors itself, `first` being the smallest code it records: only a smaller code, that
// of an earlier check, ends it.  What another workgroup of its own launch has found meanwhile must not end a workgroup
// that starts later: the record is to hold the smallest of all findings, whatever the order in which the workgroups run.
__device__ __forceinline__ bool failed_before(const BuildStatus *st, int first) {
  return (int)(*(const volatile unsigned long long *)&st->err >> 56) < first;
}

// indptr[0] == 0, non-decreasing, the last entry within [0, cap] (cap: the entries the index and value arrays
// can hold): then every indptr[r] lies in [0, cap] and the kernels below stay inside the arrays
template <typename I>
__global__ __launch_bounds__(kBlock) void spd_check_indptr(int64_t M, const I *__restrict__ ip, int64_t cap, BuildStatus *st) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r <= M; r += stride) {
    if (r == 0 && ip[0] != 0) build_error(st, kErrFirst, 0);
    if (r < M && ip[r + 1] < ip[r]) build_error(st, kErrDecreasing, r);
    if (r == M) {
      const long long last = (long long)ip[M];
      st->nnz = last;
      if (last < 0 || last > cap) build_error(st, kErrLast, 0);
    }
  }
}

// columns inside [0, N) and strictly ascending within each row: one wave per row.  The position of what it finds is the
// row, or (BY_ENTRY) the entry.
template <bool BY_ENTRY, typename P, typename I>
__global__ __launch_bounds__(kBlock) void check_columns(int64_t M, int64_t N, const P *__restrict__ ip, const I *__restrict__ ix,
                                                        BuildStatus *st) {
  if (failed_before(st, kErrRange)) return;
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * (kBlock / 64);
  for (int64_t r = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); r < M; r += waves) {
    const int64_t kb = (int64_t)ip[r], ke = (int64_t)ip[r + 1];
    for (int64_t k = kb + lane; k < ke; k += 64) {
      const int64_t c = (int64_t)ix[k];
      if (c < 0 || c >= N) build_error(st, kErrRange, BY_ENTRY ? k : r);
      else if (k > kb && (int64_t)ix[k - 1] >= c) build_error(st, kErrOrder, BY_ENTRY ? k : r);
    }
  }
}

// the first entry of [lo, hi) whose column is not below c (rows are sorted)
template <typename I>
__device__ __forceinline__ int64_t lower_bound_col(const I *__restrict__ ix, int64_t lo, int64_t hi, int64_t c) {
  while (lo < hi) {
    const int64_t mid = (lo + hi) / 2;
    if ((int64_t)ix[mid] < c) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the entry of row j with column i: its index, or -1
template <typename P, typename I>
__device__ __forceinline__ int64_t find_entry(const P *__restrict__ ip, const I *__restrict__ ix, int64_t j, int64_t i) {
  const int64_t end = (int64_t)ip[j + 1], f = lower_bound_col(ix, (int64_t)ip[j], end, i);
  return (f < end && (int64_t)ix[f] == i) ? f : -1;
}

// row and column of the entry a partner error points at (one thread)
template <typename P, typename I>
__global__ void resolve_partner(int64_t M, const P *__restrict__ ip, const I *__restrict__ ix, PartnerStatus *st) {
  if (st->err == kNoError || (int)(st->err >> 56) != kErrPartner) return;
  const int64_t k = (int64_t)(st->err & kPosMask);
  int64_t lo = 0, hi = M;                  // the last row with ip[row] <= k (ip[0] = 0 <= k < ip[M])
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) / 2;
    if ((int64_t)ip[mid] <= k) lo = mid; else hi = mid;
  }
  st->row = lo;
  st->col = (long long)ix[k];
}

template <typename I, typename O>
__global__ __launch_bounds__(kBlock) void spd_convert_index(int64_t n, const I *__restrict__ in, O *__restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) out[i] = (O)in[i];
}

// exclusive scan of n int64 into out[0 .. n] (out[n] = the sum): tile sums, one workgroup over the tile sums,
// tiles again with their offsets
constexpr int kScanPer = 4;
constexpr int kScanTile = kBlock * kScanPer;

__device__ __forceinline__ int64_t block_scan_exclusive(int64_t v, int64_t *sh, int64_t *total) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int o = 1; o < kBlock; o <<= 1) {
    const int64_t a = t >= o ? sh[t - o] : 0;
    __syncthreads();
    sh[t] += a;
    __syncthreads();
  }
  const int64_t incl = sh[t];
  *total = sh[kBlock - 1];
  __syncthreads();
  return incl - v;
}

__global__ __launch_bounds__(kBlock) void scan_tile_sums(int64_t n, const int64_t *__restrict__ in, int64_t *__restrict__ bsum) {
  __shared__ int64_t sh[kBlock];
  const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanPer;
  int64_t s = 0;
  for (int e = 0; e < kScanPer; ++e)
    if (base + e < n) s += in[base + e];
  int64_t total;
  block_scan_exclusive(s, sh, &total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(kBlock) void scan_of_sums(int64_t nb, int64_t *__restrict__ bsum) {
  __shared__ int64_t sh[kBlock];
  int64_t carry = 0;
  for (int64_t base = 0; base < nb; base += kBlock) {
    const int64_t i = base + threadIdx.x;
    const int64_t v = i < nb ? bsum[i] : 0;
    int64_t total;
    const int64_t ex = block_scan_exclusive(v, sh, &total);
    if (i < nb) bsum[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) bsum[nb] = carry;
}

__global__ __launch_bounds__(kBlock) void scan_tiles(int64_t n, int64_t nb, const int64_t *__restrict__ in,
                                                     const int64_t *__restrict__ bsum, int64_t *__restrict__ out) {
  __shared__ int64_t sh[kBlock];
  const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanPer;
  int64_t v[kScanPer], s = 0;
  for (int e = 0; e < kScanPer; ++e) {
    v[e] = base + e < n ? in[base + e] : 0;
    s += v[e];
  }
  int64_t total;
  int64_t run = block_scan_exclusive(s, sh, &total) + bsum[blockIdx.x];
  for (int e = 0; e < kScanPer; ++e) {
    if (base + e < n) out[base + e] = run;
    run += v[e];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = bsum[nb];
}

__device__ __forceinline__ float dev_conj(float a) { return a; }
__device__ __forceinline__ double dev_conj(double a) { return a; }
__device__ __forceinline__ c32 dev_conj(c32 a) { return c32{a.re, -a.im}; }
__device__ __forceinline__ c64 dev_conj(c64 a) { return c64{a.re, -a.im}; }

static inline unsigned blocks_for(int64_t n, int64_t per, int64_t most) {
  int64_t nb = (n + per - 1) / per;
  if (nb > most) nb = most;
  return (unsigned)(nb < 1 ? 1 : nb);
}

// bytes that can be read from p on inside its allocation (-1: the runtime does not know the pointer)
static inline int64_t bytes_from(const void *p) {
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (!p || hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) {
    (void)hipGetLastError();
    return -1;
  }
  return (int64_t)size - (int64_t)((const char *)p - (const char *)base);
}

// out[0 .. n] = exclusive scan of in[0 .. n) on the library stream (n = 0: out[0] = 0); bsum: (n + kScanTile - 1) /
// kScanTile + 1 entries
static inline int exclusive_scan(int64_t n, const int64_t *in, int64_t *bsum, int64_t *out) {
  hipStream_t st = ctx().stream;
  const int64_t nb = (n + kScanTile - 1) / kScanTile;
  if (nb) hipLaunchKernelGGL(scan_tile_sums, dim3((unsigned)nb), dim3(kBlock), 0, st, n, in, bsum);
  hipLaunchKernelGGL(scan_of_sums, dim3(1), dim3(kBlock), 0, st, nb, bsum);
  if (nb) hipLaunchKernelGGL(scan_tiles, dim3((unsigned)nb), dim3(kBlock), 0, st, n, nb, in, bsum, out);
  else RLH_HIP(hipMemsetAsync(out, 0, sizeof(int64_t), st));
  RLH_HIP(hipGetLastError());
  return 0;
}

// Device seconds between two points of the library stream; the events go when the timer does, however a build returns.
class StreamTimer {
 public:
  StreamTimer() = default;
  StreamTimer(const StreamTimer &) = delete;
  StreamTimer &operator=(const StreamTimer &) = delete;
  ~StreamTimer() {
    if (e0_) (void)hipEventDestroy(e0_);
    if (e1_) (void)hipEventDestroy(e1_);
  }
  int start() {
    RLH_HIP(hipEventCreate(&e0_));
    RLH_HIP(hipEventCreate(&e1_));
    RLH_HIP(hipEventRecord(e0_, ctx().stream));
    return 0;
  }
  int stop() {                             // returns when the stream has reached this point
    RLH_HIP(hipEventRecord(e1_, ctx().stream));
    RLH_HIP(hipEventSynchronize(e1_));
    float ms = 0.f;
    RLH_HIP(hipEventElapsedTime(&ms, e0_, e1_));
    seconds_ = 1e-3 * ms;
    return 0;
  }
  double seconds() const { return seconds_; }

 private:
  hipEvent_t e0_ = nullptr, e1_ = nullptr;
  double seconds_ = 0;
};

// ---------------------------------------------------------------- the checked input, step by step
// The caller's arrays once they have passed the checks on them as they came: indptr as int64 and columns as int32 (the
// caller's own arrays where they already are, else converted copies that live as long as this record).  cap: the
// entries the index and value arrays can hold; nnz: indptr's last entry.
struct CsrInput {
  const int64_t *ip64 = nullptr;
  const int32_t *ix32 = nullptr;
  DevBuf<int64_t> indptr;
  DevBuf<int32_t> cols;
  int64_t cap = INT64_MAX, nnz = 0;
};

// Step 1: *cap from what the runtime knows of the three allocations; an indptr array of fewer than M + 1 entries is
// refused (`rows`: what the entry point calls M in that message)
template <typename T, typename P, typename I>
int input_cap(const char *name, const char *rows, int64_t M, const P *ip, const I *ix, const T *va, int64_t *cap) {
  const int64_t room_p = bytes_from(ip), room_i = bytes_from(ix), room_v = bytes_from(va);
  RLH_REQUIRE(room_p < 0 || room_p >= (int64_t)sizeof(P) * (M + 1), "%s: the indptr array holds fewer than %s + 1 entries", name, rows);
  *cap = (!ix || !va) ? 0 : INT64_MAX;
  if (room_i >= 0) *cap = std::min<int64_t>(*cap, room_i / (int64_t)sizeof(I));
  if (room_v >= 0) *cap = std::min<int64_t>(*cap, room_v / (int64_t)sizeof(T));
  return 0;
}

// Step 2: a fresh status record (*hs on the host, `status` on the device) and the checks of indptr and of the columns
// on the library stream.  The caller may launch checks of its own behind them; nothing waits here.
template <bool BY_ENTRY, typename S, typename P, typename I>
int launch_input_checks(int64_t M, int64_t N, const P *ip, const I *ix, int64_t cap, DevBuf<S> &status, S *hs) {
  hipStream_t st = ctx().stream;
  if (int rc = status.alloc(1)) return rc;
  *hs = S{};
  hs->err = kNoError;
  RLH_HIP(hipMemcpyAsync(status, hs, sizeof *hs, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(spd_check_indptr<P>, dim3(blocks_for(M + 1, kBlock, 4096)), dim3(kBlock), 0, st, M, ip, cap, status.get());
  hipLaunchKernelGGL((check_columns<BY_ENTRY, P, I>), dim3(blocks_for(M, kBlock / 64, 8192)), dim3(kBlock), 0, st, M, N, ip, ix,
                     status.get());
  RLH_HIP(hipGetLastError());
  return 0;
}

// What the shared checks found, as the message of `name`; false: the code is not one of theirs.  by_entry: the
// position of a column out of range or out of order is an entry, as check_columns<true> records it.
template <typename S> bool report_input(const char *name, const S &s, int64_t cap, bool by_entry = false) {
  const long long pos = (long long)(s.err & kPosMask);
  switch ((int)(s.err >> 56)) {
    case kErrFirst: set_error("%s: indptr[0] must be 0", name); return true;
    case kErrDecreasing: set_error("%s: indptr decreases at row %lld", name, pos); return true;
    case kErrLast:
      set_error("%s: indptr's last entry (%lld) is not the number of stored entries (the index and value arrays "
                "hold at most %lld)", name, s.nnz, (long long)cap);
      return true;
    case kErrRange:
      set_error(by_entry ? "%s: column index out of range at entry %lld" : "%s: column index out of range in row %lld", name, pos);
      return true;
    case kErrOrder:
      set_error(by_entry ? "%s: the columns of a row must ascend strictly (no duplicates): entry %lld"
                         : "%s: the columns of row %lld must ascend strictly (no duplicates)", name, pos);
      return true;
    case kErrPartner:
      if constexpr (std::is_base_of<PartnerStatus, S>::value) {
        set_error("%s: the stored structure is not symmetric: entry (%lld, %lld) has no partner (%lld, %lld); the "
                  "device build creates no entries", name, s.row, s.col, s.col, s.row);
        return true;
      }
  }
  return false;
}

// Step 3: the record comes back (the one synchronisation of the checks); non-zero with the message when it holds an error
template <typename S> int fetch_input_status(const char *name, const S *status, S *hs, int64_t cap, bool by_entry = false) {
  hipStream_t st = ctx().stream;
  RLH_HIP(hipMemcpyAsync(hs, status, sizeof *hs, hipMemcpyDeviceToHost, st));
  RLH_HIP(hipStreamSynchronize(st));
  if (hs->err == kNoError) return 0;
  if (!report_input(name, *hs, cap, by_entry)) set_error("%s: unknown error code in the status record", name);
  return 1;
}

// Step 4: in->ip64 and in->ix32 (in->nnz and in->cap are the caller's to set)
template <typename P, typename I> int normalise_indices(int64_t M, const P *ip, const I *ix, CsrInput *in) {
  hipStream_t st = ctx().stream;
  const int64_t nnz = in->nnz;
  if constexpr (std::is_same<P, int64_t>::value) {
    in->ip64 = ip;
  } else {
    if (int rc = in->indptr.alloc(M + 1)) return rc;
    hipLaunchKernelGGL((spd_convert_index<P, int64_t>), dim3(blocks_for(M + 1, kBlock, 4096)), dim3(kBlock), 0, st, M + 1, ip,
                       in->indptr.get());
    in->ip64 = in->indptr;
  }
  if constexpr (std::is_same<I, int32_t>::value) {
    in->ix32 = ix;
  } else {
    if (int rc = in->cols.alloc(std::max<int64_t>(nnz, 1))) return rc;
    if (nnz) hipLaunchKernelGGL((spd_convert_index<I, int32_t>), dim3(blocks_for(nnz, kBlock, 8192)), dim3(kBlock), 0, st, nnz, ix,
                                in->cols.get());
    in->ix32 = in->cols;
  }
  RLH_HIP(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace rlh
