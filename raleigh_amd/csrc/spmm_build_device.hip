// rlh_csr_create_device: the sparse operator (K13) built by kernels from a full CSR matrix that already lies in
// device memory.  No entry, index or value visits the host; what does is a status record (fetched once), 8 bytes
// per 256-row block and the list of the blocks' staging groups (4 bytes per 16 staged columns).
//
// Built here: the 256-row interleaved windowed layout (spmm_wide.inc; rows of any length, all four types) and,
// where that one does not qualify, sliced ELL.  The 1024-row windowed layout and its stacks stay host-built
// (rlh_csr_create): their window and stack analysis is host code.
//
// The checks run first, on the caller's arrays as they are: indptr (device_build.h), then the columns of every
// row, then -- mirror_upper -- that every entry (i, j) has its partner (j, i), then the pair test of the
// interleaved layout.  Every kernel after the first returns at once when the status record already holds an error,
// so none of them reads through an index that failed its check.
//
// Interleaved layout:
//   wide_collect   one workgroup per block: the distinct 16-column staging groups (column >> 4) its rows reference,
//                  collected in an LDS hash set, compacted and sorted in LDS; the block's width
//   (host)         the qualification rules of wide_build, the offsets of the blocks, K
//   wide_place     the groups' first columns into their final place (a group that would reach past the last column
//                  is moved left to end on it, as find_windows_of does)
//   (host)         runs of consecutive groups are the windows: well_schedule, stage_inbounds, stage_aligned
//   wide_fill      positions and values in the storage order of wide_build (spmm_wide_build.hip)
// A window here is a run of referenced 16-aligned groups, not find_windows_of's hole-bridging merge: windows decide
// staging positions, not sums.  Slot order (a row's stored order), padding slots (value 0, position of the row's
// first entry in rows with at least one entry; position / column 0 in an empty row, which is then 0 * x[there]), rows past the end and the pairing rule are those of wide_build: they decide result bits.
//
// mirror_upper: the value of an entry (i, j), j < i, is the conjugate of the stored (j, i), found by binary search
// in row j inside the fill kernels (no second copy of the values).
//
// No kernel waits on another workgroup; the only atomics in global memory are those on the status record.
#include "device_build.h"
#include "spmm.h"

#include <type_traits>

namespace rlh {
namespace {

// A qualifying block stages at most (kWideLdsBytes - 2 kWideHeader) / (kWideGroup * wide_stride(8, 4)) = 210 groups
// (float32, the smallest stride: 48 bytes per column) and its group list must fit the header: kWideHeader / 4 = 256.
// The set takes 256 distinct groups; one more is "does not qualify".  256 threads insert one group at a time and
// look at the overflow flag before each, so at most 512 of the 1024 slots are ever taken and a probe always ends.
constexpr int kGroupCap = kWideHeader / 4;
constexpr int kHashSlots = 4 * kGroupCap;
constexpr int32_t kOverflow = 1 << 20;          // groups recorded for a block whose set overflowed
static_assert(kGroupCap == kWideRows, "one thread per group of a block");

struct BlockRec { int32_t width, ng; };

// the status record of this build: the shared one with the partner's place (device_build.h) and what only this build reports
struct CsrStatus : PartnerStatus {
  int differ;                     // some pair of rows (2 i, 2 i + 1) differs in its columns
};

// mirror_upper: every entry off the diagonal has its partner on the other side
template <typename I>
__global__ __launch_bounds__(kBlock) void csr_check_partners(int64_t M, const I *__restrict__ ip, const I *__restrict__ ix,
                                                             BuildStatus *st) {
  if (failed_before(st, kErrPartner)) return;
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * (kBlock / 64);
  for (int64_t r = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); r < M; r += waves) {
    const int64_t kb = (int64_t)ip[r], ke = (int64_t)ip[r + 1];
    for (int64_t k = kb + lane; k < ke; k += 64) {
      const int64_t j = (int64_t)ix[k];
      if (j != r && find_entry(ip, ix, j, r) < 0) build_error(st, kErrPartner, k);
    }
  }
}

// the pairing rule of wide_build: rows 2 q and 2 q + 1 hold the same columns, for every complete pair
template <typename I>
__global__ __launch_bounds__(kBlock) void csr_pair_test(int64_t pairs, const I *__restrict__ ip, const I *__restrict__ ix,
                                                        CsrStatus *st) {
  if (failed(st)) return;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < pairs; q += stride) {
    const int64_t a = (int64_t)ip[2 * q], b = (int64_t)ip[2 * q + 1], c = (int64_t)ip[2 * q + 2];
    bool same = (b - a) == (c - b);
    for (int64_t t = 0; same && t < b - a; ++t) same = ix[a + t] == ix[b + t];
    if (!same) { atomicOr(&st->differ, 1); return; }
  }
}

// the stored value of entry k = (i, j); mirror: below the diagonal the conjugate of the stored (j, i)
template <typename T>
__device__ __forceinline__ T entry_value(bool mirror, int64_t i, int64_t j, int64_t k, const int64_t *__restrict__ ip,
                                         const int32_t *__restrict__ ix, const T *__restrict__ va) {
  if (mirror && j < i) {
    const int64_t f = find_entry(ip, ix, j, i);       // (checked: it is there)
    return f >= 0 ? dev_conj(va[f]) : zero_of(T());
  }
  return va[k];
}

// ---------------------------------------------------------------- sliced ELL (storage order of csr_build, spmm_build.hip)
__global__ __launch_bounds__(kBlock) void sell_widths(int64_t n, int64_t ns, const int64_t *__restrict__ ip, int64_t *__restrict__ out) {
  const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (s >= ns) return;
  int64_t w = 0;
  for (int64_t r = s * 64; r < n && r < (s + 1) * 64; ++r) w = std::max<int64_t>(w, ip[r + 1] - ip[r]);
  out[s] = w * 64;
}

template <typename T>
__global__ __launch_bounds__(64) void sell_fill(int64_t n, bool mirror, const int64_t *__restrict__ ip, const int32_t *__restrict__ ix,
                                                const T *__restrict__ va, const int64_t *__restrict__ sp,
                                                int32_t *__restrict__ cols, T *__restrict__ vals) {
  const int64_t s = blockIdx.x, r = s * 64 + threadIdx.x;
  const int64_t w = (sp[s + 1] - sp[s]) / 64;
  const int64_t b = r < n ? ip[r] : 0, len = r < n ? ip[r + 1] - b : 0;
  const int32_t padcol = len > 0 ? ix[b] : 0;      // padding: value 0 and the row's first column (else 0)
  for (int64_t t = 0; t < w; ++t) {
    const int64_t e = sp[s] + t * 64 + threadIdx.x;
    if (t < len) {
      const int32_t c = ix[b + t];
      cols[e] = c;
      vals[e] = entry_value<T>(mirror, r, c, b + t, ip, ix, va);
    } else {
      cols[e] = padcol;
      vals[e] = zero_of(T());
    }
  }
}

// ---------------------------------------------------------------- the interleaved layout
__global__ __launch_bounds__(kWideRows) void wide_collect(int64_t n, const int64_t *__restrict__ ip, const int32_t *__restrict__ ix,
                                                          BlockRec *__restrict__ rec, int32_t *__restrict__ groups) {
  __shared__ int32_t tab[kHashSlots];
  __shared__ int32_t list[kGroupCap], sorted[kGroupCap];
  __shared__ int cnt, over, wmax, nlist;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x, r0 = b * kWideRows, r1 = std::min<int64_t>(r0 + kWideRows, n);
  for (int s = tid; s < kHashSlots; s += kWideRows) tab[s] = -1;
  if (tid == 0) { cnt = 0; over = 0; wmax = 0; nlist = 0; }
  __syncthreads();
  if (r0 + tid < r1) atomicMax(&wmax, (int)std::min<int64_t>(ip[r0 + tid + 1] - ip[r0 + tid], (int64_t)1 << 20));
  // the block's entries are one contiguous range: all threads walk it together (coalesced)
  const int64_t kb = ip[r0], ke = ip[r1];
  for (int64_t k = kb + tid; k < ke; k += kWideRows) {
    if (*(volatile int *)&over) break;
    const int32_t c = ix[k];
    const int32_t g = c >> kWideGroupShift;
    unsigned hs = ((unsigned)g * 2654435761u) >> 22;            // 10 bits
    for (;;) {
      const int32_t old = atomicCAS(&tab[hs], -1, g);
      if (old == -1) {
        if (atomicAdd(&cnt, 1) >= kGroupCap) over = 1;
        break;
      }
      if (old == g) break;
      hs = (hs + 1) & (kHashSlots - 1);
    }
  }
  __syncthreads();
  if (over) {                                // does not qualify: never an error, never a wrong window
    if (tid == 0) rec[b] = BlockRec{wmax, kOverflow};
    return;
  }
  for (int s = tid; s < kHashSlots; s += kWideRows)
    if (tab[s] >= 0) list[atomicAdd(&nlist, 1)] = tab[s];
  __syncthreads();
  int ng = nlist;                            // <= kGroupCap
  if (tid < ng) {                            // distinct keys: the rank of a key is its place
    const int32_t g = list[tid];
    int rank = 0;
    for (int q = 0; q < ng; ++q) rank += list[q] < g;
    sorted[rank] = g;
  }
  __syncthreads();
  if (ng == 0) {                             // a block of empty rows still stages one group
    ng = 1;
    if (tid == 0) groups[b * kGroupCap] = 0;
  } else if (tid < ng) {
    groups[b * kGroupCap + tid] = sorted[tid];
  }
  if (tid == 0) rec[b] = BlockRec{wmax, ng};
}

__global__ __launch_bounds__(kWideRows) void wide_place(int64_t n_cols, const WideMeta *__restrict__ meta,
                                                        const int32_t *__restrict__ groups, int32_t *__restrict__ gsrc) {
  const int64_t b = blockIdx.x;
  const WideMeta mt = meta[b];
  if ((int)threadIdx.x >= mt.ng) return;
  int64_t src = (int64_t)groups[b * kGroupCap + threadIdx.x] * kWideGroup;
  if (src + kWideGroup > n_cols && n_cols >= kWideGroup) src = n_cols - kWideGroup;
  gsrc[mt.goff + threadIdx.x] = (int32_t)src;
}

template <typename T, int K>
__global__ __launch_bounds__(kWideRows) void wide_fill(int64_t n, bool mirror, const int64_t *__restrict__ ip,
                                                       const int32_t *__restrict__ ix, const T *__restrict__ va,
                                                       const WideMeta *__restrict__ meta, const int32_t *__restrict__ gsrc,
                                                       rlh_u32x4e *__restrict__ idx, rlh_u32x4e *__restrict__ vals) {
  constexpr int ES = sizeof(T), VP = ES / 2, VPG = 16 / ES, TPS = kWideRows / K;
  __shared__ int32_t gs[kGroupCap];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const WideMeta mt = meta[b];
  const int ng = mt.ng;
  if (tid < ng) gs[tid] = gsrc[mt.goff + tid];
  __syncthreads();
  // position of column c in the staged image: the last group that starts at or before c (staged_position)
  auto position = [&](int32_t c) -> unsigned {
    int lo = 0, hi = ng;
    while (hi - lo > 1) {
      const int mid = (lo + hi) / 2;
      if (gs[mid] <= c) lo = mid; else hi = mid;
    }
    return (unsigned)(lo * kWideGroup + (c - gs[lo]));
  };
  const int64_t r = b * kWideRows + tid;
  const int lt = tid / K, lk = tid % K;
  const int64_t p = r < n ? ip[r] : 0, len = r < n ? ip[r + 1] - p : 0;
  // padding slots carry value 0 and the position of the row's own first entry (a row past the end: position 0)
  const unsigned padpos = len > 0 ? position(ix[p]) : 0u;
  for (int q = 0; q < mt.nchunks; ++q) {
    const int64_t ch = mt.eoff + q;
    union { rlh_u32x4e v; unsigned short s[8]; } pos;
    int32_t col[8];
#pragma unroll
    for (int tt = 0; tt < 8; ++tt) {
      const int64_t t = (int64_t)q * 8 + tt;
      col[tt] = t < len ? ix[p + t] : -1;
      pos.s[tt] = (unsigned short)(t < len ? position(col[tt]) : padpos);
    }
    if (lk == 0) idx[ch * TPS + lt] = pos.v;
#pragma unroll
    for (int k = 0; k < VP; ++k) {
      union { rlh_u32x4e v; T e[VPG]; } piece;
#pragma unroll
      for (int e = 0; e < VPG; ++e) {
        const int tt = k * VPG + e;
        const int64_t t = (int64_t)q * 8 + tt;
        piece.e[e] = t < len ? entry_value<T>(mirror, r, col[tt], p + t, ip, ix, va) : zero_of(T());
      }
      vals[((ch * K + lk) * VP + k) * TPS + lt] = piece.v;
    }
  }
}

struct CsrScratch {                 // released when the build returns, however it returns
  DevBuf<CsrStatus> status;
  CsrInput in;
  DevBuf<int64_t> widths, bsum;
  DevBuf<int32_t> groups;
  DevBuf<BlockRec> rec;
};

struct Lap {                        // RLH_SPMM_VERBOSE=1: the kernels of a phase have run before its time is taken
  PhaseClock clk;
  int operator()(const char *what) {
    if (clk.on) {
      RLH_HIP(hipStreamSynchronize(ctx().stream));
      clk.lap(what);
    }
    return 0;
  }
};

template <typename T>
int sell_build_device(rlh_csr *h, CsrScratch &w, bool mirror, const int64_t *ip, const int32_t *ix, const T *va) {
  hipStream_t st = ctx().stream;
  const int64_t n = h->n_rows, ns = (n + 63) / 64;
  const int64_t nb = (ns + kScanTile - 1) / kScanTile;
  if (int rc = h->slice_ptr.alloc((size_t)(ns + 1))) return rc;
  int64_t padded = 0;
  if (ns > 0) {
    if (int rc = w.widths.alloc((size_t)ns)) return rc;
    if (int rc = w.bsum.alloc((size_t)(nb + 1))) return rc;
    hipLaunchKernelGGL(sell_widths, dim3(blocks_for(ns, kBlock, INT32_MAX)), dim3(kBlock), 0, st, n, ns, ip, w.widths);
    if (int rc = exclusive_scan(ns, w.widths, w.bsum, h->slice_ptr)) return rc;
    RLH_HIP(hipMemcpyAsync(&padded, h->slice_ptr + ns, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    RLH_HIP(hipStreamSynchronize(st));
  } else {
    RLH_HIP(hipMemsetAsync(h->slice_ptr, 0, sizeof(int64_t), st));
  }
  h->n_slices = ns;
  h->padded = padded;
  if (padded > 0) {
    if (int rc = h->cols.alloc((size_t)padded)) return rc;
    if (int rc = h->vals.alloc((size_t)padded * sizeof(T))) return rc;
    hipLaunchKernelGGL(sell_fill<T>, dim3((unsigned)ns), dim3(64), 0, st, n, mirror, ip, ix, va, h->slice_ptr, h->cols, (T *)h->vals);
    RLH_HIP(hipGetLastError());
  }
  h->device_bytes = (ns + 1) * 8 + padded * (4 + (int64_t)sizeof(T));
  return 0;
}

// wide_build (spmm_wide_build.hip) with the per-block analysis and the fill done by kernels; the rules in between
// are the host's, line by line.  h->wide_blocks stays 0 where the layout does not qualify.
template <typename T>
int wide_build_device(rlh_csr *h, CsrScratch &w, Lap &lap, bool mirror, bool force, bool paired, const int64_t *ip,
                      const int32_t *ix, const T *va) {
  hipStream_t st = ctx().stream;
  const int es = (int)sizeof(T), VP = es / 2;
  const int64_t n = h->n_rows;
  const int64_t nblocks = (n + kWideRows - 1) / kWideRows;
  h->wide_blocks = 0;
  if (nblocks == 0 || h->nnz == 0) return 0;
  if (int rc = w.rec.alloc((size_t)nblocks)) return rc;
  if (int rc = w.groups.alloc((size_t)nblocks * kGroupCap)) return rc;
  hipLaunchKernelGGL(wide_collect, dim3((unsigned)nblocks), dim3(kWideRows), 0, st, n, ip, ix, w.rec, w.groups);
  RLH_HIP(hipGetLastError());
  std::vector<BlockRec> rec((size_t)nblocks);
  RLH_HIP(hipMemcpyAsync(rec.data(), w.rec, (size_t)nblocks * sizeof(BlockRec), hipMemcpyDeviceToHost, st));
  RLH_HIP(hipStreamSynchronize(st));
  if (int rc = lap("staging groups of the blocks")) return rc;
  int32_t wmax = 0, gmax = 0;
  int64_t staged = 0, slots = 0;
  for (int64_t b = 0; b < nblocks; ++b) {
    wmax = std::max(wmax, rec[b].width);
    gmax = std::max(gmax, rec[b].ng);
    staged += (int64_t)rec[b].ng * kWideGroup;
    slots += (int64_t)rec[b].width * kWideRows;
  }
  h->stage_ratio = slots > 0 ? (double)staged / (double)slots : 0.0;
  if ((int64_t)gmax * kWideGroup * wide_stride(wide_min_nv(h->dtype), es) + 2 * kWideHeader > kWideLdsBytes) return 0;
  if (gmax * 4 > kWideHeader || wmax > 8 * 32767) return 0;
  if (!force && staged * 10 > slots * 9) return 0;
  const int K = paired ? 2 : 1;
  h->wide_k = K;
  const int TPS = kWideRows / K;
  std::vector<WideMeta> meta((size_t)nblocks);
  int64_t eoff = 0, goff = 0;
  for (int64_t b = 0; b < nblocks; ++b) {
    const int nch = std::max(1, (rec[b].width + 7) / 8);
    meta[b] = WideMeta{eoff, (int32_t)goff, (int16_t)nch, (int16_t)rec[b].ng};
    eoff += nch;
    goff += rec[b].ng;
  }
  RLH_REQUIRE(goff < ((int64_t)1 << 31), "rlh_csr_create_device: too many staging groups");
  const int64_t nchunks = eoff + kWidePadChunks;  // padding: the kernel's prefetch runs ahead of the last block's chunks
  const size_t idx_bytes = (size_t)nchunks * TPS * 16, val_bytes = (size_t)nchunks * VP * kWideRows * 16;
  if (int rc = h->wide_meta.alloc((size_t)nblocks)) return rc;
  if (int rc = h->wide_gsrc.alloc((size_t)goff)) return rc;
  if (int rc = h->wide_idx.alloc(idx_bytes)) return rc;
  if (int rc = h->wide_vals.alloc(val_bytes)) return rc;
  RLH_HIP(hipMemcpyAsync(h->wide_meta, meta.data(), (size_t)nblocks * sizeof(WideMeta), hipMemcpyHostToDevice, st));
  // (the fill writes every slot of every block: what is zeroed here is the padding behind the last block)
  RLH_HIP(hipMemsetAsync((char *)h->wide_idx + (size_t)eoff * TPS * 16, 0, idx_bytes - (size_t)eoff * TPS * 16, st));
  RLH_HIP(hipMemsetAsync((char *)h->wide_vals + (size_t)eoff * VP * kWideRows * 16, 0,
                         val_bytes - (size_t)eoff * VP * kWideRows * 16, st));
  hipLaunchKernelGGL(wide_place, dim3((unsigned)nblocks), dim3(kWideRows), 0, st, h->n_cols, h->wide_meta, w.groups, h->wide_gsrc);
  if (K == 2)
    hipLaunchKernelGGL((wide_fill<T, 2>), dim3((unsigned)nblocks), dim3(kWideRows), 0, st, n, mirror, ip, ix, va, h->wide_meta,
                       h->wide_gsrc, (rlh_u32x4e *)h->wide_idx, (rlh_u32x4e *)h->wide_vals);
  else
    hipLaunchKernelGGL((wide_fill<T, 1>), dim3((unsigned)nblocks), dim3(kWideRows), 0, st, n, mirror, ip, ix, va, h->wide_meta,
                       h->wide_gsrc, (rlh_u32x4e *)h->wide_idx, (rlh_u32x4e *)h->wide_vals);
  RLH_HIP(hipGetLastError());
  std::vector<int32_t> gsrc((size_t)goff);
  RLH_HIP(hipMemcpyAsync(gsrc.data(), h->wide_gsrc, (size_t)goff * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  RLH_HIP(hipStreamSynchronize(st));          // (meta and rec are read by the copies above until here)
  if (int rc = lap("positions and values")) return rc;
  // the windows of a block: its runs of consecutive groups
  std::vector<std::vector<Win>> wins((size_t)nblocks);
  stage_flags(gsrc.data(), goff, kWideGroup, h->n_cols, &h->stage_inbounds, &h->stage_aligned);
  for (int64_t b = 0; b < nblocks; ++b) {
    std::vector<Win> &ws = wins[(size_t)b];
    for (int32_t g = 0; g < rec[b].ng; ++g) {
      const int32_t src = gsrc[(size_t)meta[b].goff + g];
      if (!ws.empty() && ws.back().start + ws.back().len == src) ws.back().len += kWideGroup;
      else ws.push_back(Win{src, kWideGroup, g * kWideGroup});
    }
  }
  well_schedule(wins, nblocks, n, kWideRows, ctx().num_cu * 2, h->wide_order);
  h->wide_maxcol.resize((size_t)nblocks);
  // the last STAGED column of a block (wide_sched: a block is interior when it stages nothing at or past n_own)
  for (int64_t b = 0; b < nblocks; ++b) {
    const Win &last = wins[(size_t)b].back();
    h->wide_maxcol[(size_t)b] = (int32_t)std::min<int64_t>((int64_t)last.start + last.len - 1, h->n_cols - 1);
  }
  h->wide_gmax = gmax;
  h->padded = eoff * 8 * kWideRows;
  h->device_bytes = nblocks * (int64_t)sizeof(WideMeta) + goff * 4 + (int64_t)idx_bytes + (int64_t)val_bytes;
  h->wide_blocks = nblocks;
  if (int rc = lap("launch order")) return rc;
  return 0;
}

template <typename T, typename I>
int csr_create_device_impl(rlh_csr *h, const I *ip, const I *ix, const T *va, bool mirror, bool want_sell, bool force_wide) {
  constexpr const char *name = "rlh_csr_create_device";
  const int64_t M = h->n_rows, N = h->n_cols;
  hipStream_t st = ctx().stream;
  const dim3 blk(kBlock);
  CsrScratch w;
  Lap lap;
  // ---- the checks: the shared ones (device_build.h), then this build's own on the same record; one record comes back
  CsrInput &in = w.in;
  CsrStatus hs;
  if (int rc = input_cap(name, "n_rows", M, ip, ix, va, &in.cap)) return rc;
  const bool real = std::is_same<T, float>::value || std::is_same<T, double>::value;
  const bool pair_test = real && env_int("RLH_WIDE_PAIR", 1) != 0 && !want_sell;
  if (int rc = launch_input_checks<false>(M, N, ip, ix, in.cap, w.status, &hs)) return rc;
  if (mirror) {
    hipLaunchKernelGGL(csr_check_partners<I>, dim3(blocks_for(M, kBlock / 64, 8192)), blk, 0, st, M, ip, ix, w.status);
    hipLaunchKernelGGL((resolve_partner<I, I>), dim3(1), dim3(1), 0, st, M, ip, ix, w.status);
  }
  if (pair_test) hipLaunchKernelGGL(csr_pair_test<I>, dim3(blocks_for(M / 2, kBlock, 8192)), blk, 0, st, M / 2, ip, ix, w.status);
  RLH_HIP(hipGetLastError());
  if (int rc = fetch_input_status(name, w.status.get(), &hs, in.cap)) return rc;
  h->nnz = in.nnz = hs.nnz;
  if (int rc = lap("argument checks")) return rc;
  // ---- indptr as int64 and columns as int32 (the caller's own arrays where they already are)
  if (int rc = normalise_indices(M, ip, ix, &in)) return rc;
  const int64_t *ip64 = in.ip64;
  const int32_t *ix32 = in.ix32;
  if (!want_sell) {
    const bool paired = pair_test && !hs.differ && h->nnz >= 16 * M;
    if (int rc = wide_build_device<T>(h, w, lap, mirror, force_wide, paired, ip64, ix32, va)) return rc;
  }
  if (h->wide_blocks == 0) {
    h->wide_k = 1;
    if (int rc = sell_build_device<T>(h, w, mirror, ip64, ix32, va)) return rc;
    if (int rc = lap("sliced ELL")) return rc;
  }
  RLH_HIP(hipStreamSynchronize(st));         // the caller's arrays and the scratch are not referenced after the return
  return 0;
}

}  // namespace
}  // namespace rlh

using namespace rlh;

extern "C" int rlh_csr_create_device(rlh_csr_t *out, int dtype, int64_t n_rows, int64_t n_cols, int index_bits,
                                     const void *d_indptr, const void *d_indices, const void *d_values, int mirror_upper) {
  if (int rc = require_ready()) return rc;
  RLH_REQUIRE(out != nullptr, "rlh_csr_create_device: null handle pointer");
  *out = nullptr;
  RLH_REQUIRE(dtype_valid(dtype), "rlh_csr_create_device: unknown dtype %d", dtype);
  RLH_REQUIRE(index_bits == 32 || index_bits == 64, "rlh_csr_create_device: index_bits must be 32 or 64, got %d", index_bits);
  RLH_REQUIRE(n_rows >= 0 && n_cols >= 0 && n_rows < INT32_MAX && n_cols < INT32_MAX,
              "rlh_csr_create_device: sizes must lie in [0, 2^31 - 1)");
  RLH_REQUIRE(!mirror_upper || n_rows == n_cols, "rlh_csr_create_device: mirror_upper needs a square matrix, got %lld x %lld",
              (long long)n_rows, (long long)n_cols);
  RLH_REQUIRE(d_indptr, "rlh_csr_create_device: null indptr");
  const char *fmt = getenv("RLH_SPMM_FORMAT");
  const bool want_sell = fmt && !strcmp(fmt, "sell"), force_wide = fmt && !strcmp(fmt, "wide");
  RLH_REQUIRE(!(fmt && !strcmp(fmt, "well")),
              "rlh_csr_create_device: RLH_SPMM_FORMAT=well: the 1024-row windowed layout is not built on the device "
              "(interleaved or sliced ELL only; rlh_csr_create builds it from host arrays)");
  rlh_csr *h = new rlh_csr();                 // (every member at its "nothing built" default)
  h->dtype = dtype; h->n_rows = n_rows; h->n_cols = n_cols;
  int rc = 1;
#define RLH_CSR_BUILD(T)                                                                                              \
  rc = index_bits == 32 ? csr_create_device_impl<T, int32_t>(h, (const int32_t *)d_indptr, (const int32_t *)d_indices,  \
                                                             (const T *)d_values, mirror_upper != 0, want_sell, force_wide) \
                        : csr_create_device_impl<T, int64_t>(h, (const int64_t *)d_indptr, (const int64_t *)d_indices,  \
                                                             (const T *)d_values, mirror_upper != 0, want_sell, force_wide)
  switch (dtype) {
    case RLH_S: RLH_CSR_BUILD(float); break;
    case RLH_D: RLH_CSR_BUILD(double); break;
    case RLH_C: RLH_CSR_BUILD(c32); break;
    case RLH_Z: RLH_CSR_BUILD(c64); break;
  }
#undef RLH_CSR_BUILD
  if (rc) {
    rlh_csr_destroy(h);
    return rc;
  }
  *out = h;
  return 0;
}
