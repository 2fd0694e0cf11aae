// Pieces shared by the operators that are built by kernels from CSR arrays already in device memory
// (rlh_spd_create_device: spmm_data.hip, rlh_csr_create_device: spmm_build_device.hip): the status record the host
// fetches once, the indptr check, the index conversion, the exclusive scan and two host helpers.  The kernels sit in
// an unnamed namespace: every translation unit that includes this file gets its own copies.
#pragma once

#include "common.h"

#include <algorithm>

namespace rlh {
namespace {

constexpr int kBlock = 256;

struct BuildStatus {
  unsigned long long err;         // ~0: none; else (code << 56) | position, the smallest of all found
  long long nnz;                  // indptr[n_rows]
};
enum { kErrFirst = 1, kErrDecreasing = 2, kErrLast = 3, kErrRange = 4, kErrOrder = 5 };
constexpr unsigned long long kNoError = ~0ull;

__device__ __forceinline__ void build_error(BuildStatus *st, int code, int64_t pos) {
  atomicMin(&st->err, ((unsigned long long)code << 56) | (unsigned long long)pos);
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

}  // namespace
}  // namespace rlh
