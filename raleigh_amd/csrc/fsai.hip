// Factorised sparse approximate inverse (Kolotilina-Yeremin): T = G^H G ~ A^-1 for a Hermitian positive definite A
// given as a full CSR matrix in device memory (rlh_fsai_*, include/rlhip.h).  The UPPER triangle defines A: no value
// stored below the diagonal is ever read.
//
// Row i of G lives on P_i, the (at most max_row, the largest) columns of the level pattern of row i: with L(i) the
// stored columns j <= i of row i of A, P_1(i) = L(i) and P_{l+1}(i) is the union of L(j) over j in P_l(i) -- the
// pattern of tril(A)^levels, nested because j lies in L(j).  With S =
// A[P_i, P_i] = R^H R (R upper triangular, positive diagonal) the row is g = conj(u), R u = e_k: then
// S g^H = e_k / g_kk and g_kk = 1 / R_kk > 0.  Every local system is solved in double / complex double whatever the
// storage type; G is rounded to it once, at the store.
//
// The build, all on the library stream:
//   checks          indptr (device_build.h), the columns of every row, then per row: the diagonal is stored and every
//                   entry below it has its partner above (fsai_count)
//   prefiltration   (the rlh_fsthreshold_* entry points only, between the checks and the pattern) fsai_diagonal, then
//                   fsai_strong<T, false>, 8 lanes per row: the lower entries whose partner above the diagonal is large
//                   against prefilter in a scaling-invariant measure are counted per row; one scan, one wait for the
//                   size and for what the checks found, and fsai_strong<T, true> writes the strong lower structure
//                   (a CSR of the strong entries, the diagonal last in each row).  The pattern kernels of every level,
//                   1 included, walk it in place of A; everything after the pattern reads the caller's arrays.
//   pattern         kept entries per row, exclusive scans, columns of G and the rows of the bins.  Level 1: a slice
//                   of A's row (fsai_count, fsai_fill).  Higher levels: one wave per row (fsai_pattern_count, then
//                   fsai_pattern_fill, which forms the row again).  Lane q walks L(P[q]) downwards from its diagonal;
//                   the wave's maximum of the lanes' current columns is the next member, every lane that shows it
//                   steps on: a descending selection without a sort, at most max_row + 1 steps per level.  Capping
//                   to the max_row largest after every level gives the capped final pattern: what a dropped column
//                   j reaches is <= j, below every kept column, and the kept ones are in the next union themselves.
//   enrichment      (the _adaptive entry points only) fsai_enrich<T, LANES>: `steps` times per row, solve on the pattern
//                   and take the (at most step_size) columns below i, stored in a member's row, that lower the row's
//                   Kaporin functional most.  The rows are binned by their capacity min(max_row, k + steps *
//                   step_size) with the keys and scans of the set-up's bins, one lane group per row from the first
//                   solve to the last selection; pattern and packed triangle in the LDS (the set-up's 40 KB), g in
//                   the lanes' registers.  The patterns go to a slab at the scanned capacities and are compacted
//                   (fsai_fill again) with new counts, keys and scans; from there on the build is the one below.
//   set-up          fsai_setup<T, LANES>: LANES = 8, 16, 32 or 64 lanes per row for k <= LANES (RLH_FSAI_BINS=0: 8
//                   and 64 only), 256 threads per workgroup (128 for 32 lanes in complex, 64 for 64 lanes).  The
//                   packed upper triangle of S (then R) lies in the LDS: at most 40 KB per workgroup, so four
//                   workgroups fit the 160 KB of a CU.  Lane q owns column q and every sum runs over t in order, so
//                   a row's bits do not depend on its bin.  The pattern is read from G's own column array;
//                   S is gathered by a binary search for column P[q] in the sorted row P[p], p <= q.
//   post-filtration (the rlh_fsfilter_* entry points only) fsai_filter<T>, 8 lanes per row: the entries of the computed G
//                   that are small against drop in a scaling-invariant measure leave the row; the kept columns go to
//                   a slab at the row's old offset, counts, keys and scans are made again, fsai_fill compacts and
//                   fsai_setup solves every row once more in the bin of its new length.
//   operators       G and G^H as the two orientations of one sparse data operator (rlh_spd_create_device), which
//                   copies G's arrays; the build's own are scratch and released.
// A row is one lane group's work from the gather to the store: no floating-point atomics, no order that depends on
// scheduling, G is the same bits in every run.  Lanes of a group exchange data through the LDS and shuffles only
// within their own wave, at points every lane of the group reaches together (the trip counts are the group's k).
// What a kernel finds wrong goes to the status record (code and the smallest position), never to a trap.
//
// The host side follows the kernels.  An entry point makes an FsaiPlan from its named makers (what the build is asked
// to do, and so which arguments are checked); create_host and create_device check it and run fsai_build inside
// make_handle.  fsai_build is the one build path and reads as the list above: the stages are the members of FsaiBuild,
// the state that owns every array one stage hands to the next -- checks, strong_structure (if prefilter), level_pattern,
// enrich (if steps), solve, post_filter (if drop), make_operator.  Whether the level pattern is a slice of A's row or
// the wave-per-row walk is decided once (FsaiBuild::slice).  pattern_totals is the scan-fetch-wait-check sequence on
// the counts and keys in FsaiScratch; new_columns follows it with the column array of that size, and compact copies the
// rows into it (fsai_fill): from A's rows at level 1, from the slab of the enrichment, from that of the filter.
// for_each_bin with launch_bin launches the enrichment and the set-up kernels bin by bin.
//
// New values on the kept pattern (rlh_fsvalues_update*, fsai_update): the numeric phase alone, from the pieces the
// stages are made of.  checked_input (the checks on the arrays as they came), fsai_kept_rows (a stored diagonal, the
// rows' lengths from the handle's G, the keys of the bins), pattern_totals, fsai_bin_rows, then solve_rows (fsai_setup
// bin by bin, as in the stage solve) into a scratch value array, the pattern read from the operator's own arrays of G.
// Only when every row succeeded do the values go to G and, conjugated, to G^H (spd_set_values, spmm_data.h); structure
// and partitions stay.
#include "fsai.h"

#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include <vector>

namespace rlh {
namespace {

constexpr int kShort = 8;                      // rows of at most kShort kept entries: kShort lanes per row
constexpr int kMaxRow = 64;
constexpr int kMaxLevels = 8;
constexpr int kSetupBlocksPerCu = 8;           // grid of a set-up kernel: at most this many workgroups per CU
enum { kErrDiag = 6, kErrNotPd = 8 };          // beside the shared codes (device_build.h): a missing diagonal wins over a missing partner

struct FsaiStatus : PartnerStatus {
  unsigned long long truncated;                // rows cut to max_row
  int longest;                                 // longest row of G
  unsigned long long limited;                  // adaptive build: rows max_row held back (those cut are among them)
  unsigned long long removed;                  // post-filtration: entries of G dropped
  int kept_longest;                            // post-filtration: longest row of the filtered G
  unsigned long long weak;                     // prefiltration: stored entries below the diagonal that are not strong
};

// The rows of a build go to bins by their kept entries k: 8, 16, 32 or 64 lanes per row (two bins: 8 or 64).  Two
// scans carry the three running counts of rows with k <= 8, k <= 16 (high half of the first key) and k <= 32; with two
// bins all three count k <= 8.  n < 2^31, so the halves do not meet.
__device__ __forceinline__ void bin_keys(int64_t k, int four, int64_t *ka, int64_t *kb) {
  const int64_t a = k <= kShort ? 1 : 0, b = four ? (k <= 16 ? 1 : 0) : a, c = four ? (k <= 32 ? 1 : 0) : a;
  *ka = a | (b << 32);
  *kb = c;
}

struct Bins {
  const int64_t *sa, *sb;        // exclusive scans of the two keys
  int64_t c8, c16, c32;          // their totals: rows with k <= 8, <= 16, <= 32
  int32_t *rows;                 // the rows of bin 8, then 16, 32 and 64, each in ascending order
};

// (the row's own keys are the steps of the scans at i)
__device__ __forceinline__ void put_row(const Bins &b, int64_t i) {
  const int64_t a = b.sa[i], p8 = a & 0xffffffff, p16 = a >> 32, p32 = b.sb[i];
  int64_t at;
  if (p8 + 1 == (b.sa[i + 1] & 0xffffffff)) at = p8;
  else if (p16 + 1 == (b.sa[i + 1] >> 32)) at = b.c8 + (p16 - p8);
  else if (p32 + 1 == b.sb[i + 1]) at = b.c16 + (p32 - p16);
  else at = b.c32 + (i - p32);
  b.rows[at] = (int32_t)i;
}

// per row: the diagonal is stored, every entry below it has its partner; at level 1 (tally) the kept entries (the
// last min(lower, max_row) up to the diagonal), where they begin in A's row, and the keys of the row's bin (that of
// its capacity min(max_row, k + grow); grow = 0 unless the pattern is enriched)
__global__ __launch_bounds__(kBlock) void fsai_count(int64_t n, int max_row, int tally, int four, int grow,
                                                     const int64_t *__restrict__ ip,
                                                     const int32_t *__restrict__ ix, int64_t *__restrict__ cnt,
                                                     int64_t *__restrict__ keya, int64_t *__restrict__ keyb,
                                                     int64_t *__restrict__ start, FsaiStatus *st) {
  if (failed_before(st, kErrDiag)) return;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const int64_t kb = ip[i], ke = ip[i + 1];
    const int64_t d = lower_bound_col(ix, kb, ke, i);
    int64_t k = 0;
    if (d == ke || (int64_t)ix[d] != i) {
      build_error(st, kErrDiag, i);
    } else {
      for (int64_t e = kb; e < d; ++e) {
        const int64_t j = ix[e];
        const int64_t je = ip[j + 1], f = lower_bound_col(ix, ip[j], je, i);
        if (f == je || (int64_t)ix[f] != i) build_error(st, kErrPartner, e);
      }
      const int64_t lower = d + 1 - kb;
      k = lower < max_row ? lower : max_row;
      if (tally) {
        if (lower > max_row) atomicAdd(&st->truncated, 1ull);
        atomicMax(&st->longest, (int)k);
      }
      start[i] = d + 1 - k;
    }
    if (tally) {
      cnt[i] = k;
      bin_keys(k + grow < max_row ? k + grow : max_row, four, &keya[i], &keyb[i]);
    }
  }
}

// level 1: the columns of G (a slice of A's row) and the rows of the bins
__global__ __launch_bounds__(kBlock) void fsai_fill(int64_t n, const int32_t *__restrict__ ix, const int64_t *__restrict__ start,
                                                    const int64_t *__restrict__ gp, int32_t *__restrict__ gi, Bins bins) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const int64_t g0 = gp[i], k = gp[i + 1] - g0, a0 = start[i];
    for (int64_t t = 0; t < k; ++t) gi[g0 + t] = ix[a0 + t];
    put_row(bins, i);
  }
}

// An update of the values (rlh_fsvalues_update*) keeps the pattern: per row the new matrix must store its diagonal
// (nothing else is asked of its structure: the solve reads entries on or above the diagonal and takes a missing one
// as zero); the kept entries of the row are those of the handle's G (gp: its row pointers), the keys those of its bin
__global__ __launch_bounds__(kBlock) void fsai_kept_rows(int64_t n, int four, const int64_t *__restrict__ ip,
                                                         const int32_t *__restrict__ ix, const int64_t *__restrict__ gp,
                                                         int64_t *__restrict__ cnt, int64_t *__restrict__ keya,
                                                         int64_t *__restrict__ keyb, FsaiStatus *st) {
  if (failed_before(st, kErrDiag)) return;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const int64_t ke = ip[i + 1], d = lower_bound_col(ix, ip[i], ke, i);
    if (d == ke || (int64_t)ix[d] != i) build_error(st, kErrDiag, i);
    const int64_t k = gp[i + 1] - gp[i];
    cnt[i] = k;
    bin_keys(k, four, &keya[i], &keyb[i]);
  }
}

// the rows of the bins alone (an update: the columns of G stay where they are)
__global__ __launch_bounds__(kBlock) void fsai_bin_rows(int64_t n, Bins bins) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) put_row(bins, i);
}

// lanes of one wave that exchange data through the LDS: the LDS serves a wave's accesses in order; this keeps the
// compiler from moving one across
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// the largest value among the LANES lanes of a group (64: the wave), the same in each of them
template <int LANES> __device__ __forceinline__ int group_max(int v) {
  for (int o = LANES / 2; o; o >>= 1) {
    const int w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

// The level pattern of row i by one wave: its (at most max_row, the largest) columns ascending in cur[0 .. k), k
// returned in every lane; *over: the full pattern has more than max_row members.  Every lane of the wave gets here
// together; the trip counts are the wave's.
__device__ __forceinline__ int row_pattern(int64_t i, int max_row, int levels, const int64_t *__restrict__ ip,
                                           const int32_t *__restrict__ ix, int32_t *cur, int lane, bool *over) {
  const int64_t kb = ip[i], ke = ip[i + 1], d = lower_bound_col(ix, kb, ke, i);
  const int64_t lower = d - kb + ((d < ke && (int64_t)ix[d] == i) ? 1 : 0);
  int k = (int)(lower < max_row ? lower : max_row);
  *over = lower > max_row;
  wave_sync();                                       // (the row before this one is done with the LDS)
  if (lane < k) cur[lane] = ix[kb + lower - k + lane];
  wave_sync();
  for (int l = 1; l < levels; ++l) {
    // lane q < k walks L(cur[q]) downwards: pos is the entry it shows, from the diagonal of that row on
    int64_t beg = 0, pos = -1;
    if (lane < k) {
      const int64_t j = cur[lane], je = ip[j + 1];
      beg = ip[j];
      const int64_t f = lower_bound_col(ix, beg, je, j);
      pos = (f < je && (int64_t)ix[f] == j) ? f : f - 1;
    }
    int cand = pos >= beg ? ix[pos] : -1, mine = -1, kn = 0;
    for (;;) {
      const int m = group_max<64>(cand);                  // the largest column not yet taken: the same in every lane
      if (m < 0) break;
      if (kn == max_row) {
        *over = true;
        break;
      }
      if (lane == kn) mine = m;
      ++kn;
      if (cand == m) {
        --pos;
        cand = pos >= beg ? ix[pos] : -1;
      }
    }
    wave_sync();
    if (lane < kn) cur[kn - 1 - lane] = mine;
    wave_sync();
    k = kn;
  }
  return k;
}

// levels > 1: the kept entries per row and the keys of its bin (one wave per row)
__global__ __launch_bounds__(kBlock) void fsai_pattern_count(int64_t n, int max_row, int levels, int four, int grow,
                                                             const int64_t *__restrict__ ip, const int32_t *__restrict__ ix,
                                                             int64_t *__restrict__ cnt, int64_t *__restrict__ ka,
                                                             int64_t *__restrict__ kb, FsaiStatus *st) {
  if (failed(st)) return;
  __shared__ int32_t cur[kBlock / 64][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * (kBlock / 64);
  for (int64_t i = (int64_t)blockIdx.x * (kBlock / 64) + wave; i < n; i += waves) {
    bool over;
    const int k = row_pattern(i, max_row, levels, ip, ix, cur[wave], lane, &over);
    if (lane == 0) {
      cnt[i] = k;
      bin_keys(k + grow < max_row ? k + grow : max_row, four, &ka[i], &kb[i]);
      if (over) atomicAdd(&st->truncated, 1ull);
      atomicMax(&st->longest, k);
    }
  }
}

// levels > 1: the columns of G and the rows of the bins (the same walk again: nothing but the counts is kept between)
__global__ __launch_bounds__(kBlock) void fsai_pattern_fill(int64_t n, int max_row, int levels, const int64_t *__restrict__ ip,
                                                            const int32_t *__restrict__ ix, const int64_t *__restrict__ gp,
                                                            int32_t *__restrict__ gi, Bins bins) {
  __shared__ int32_t cur[kBlock / 64][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * (kBlock / 64);
  for (int64_t i = (int64_t)blockIdx.x * (kBlock / 64) + wave; i < n; i += waves) {
    bool over;
    const int64_t g0 = gp[i];
    int k = row_pattern(i, max_row, levels, ip, ix, cur[wave], lane, &over);
    if ((int64_t)k > gp[i + 1] - g0) k = (int)(gp[i + 1] - g0);      // (equal: the walk is the counting kernel's)
    if (lane < k) gi[g0 + lane] = cur[wave][lane];
    if (lane == 0) put_row(bins, i);
  }
}

// ---------------------------------------------------------------- the local solves, in double / complex double
template <typename T> struct Wide { using type = double; };
template <> struct Wide<c32> { using type = c64; };
template <> struct Wide<c64> { using type = c64; };

__device__ __forceinline__ double widen(float a) { return (double)a; }
__device__ __forceinline__ double widen(double a) { return a; }
__device__ __forceinline__ c64 widen(c32 a) { return c64{(double)a.re, (double)a.im}; }
__device__ __forceinline__ c64 widen(c64 a) { return a; }
__device__ __forceinline__ void narrow(double a, float *out) { *out = (float)a; }
__device__ __forceinline__ void narrow(double a, double *out) { *out = a; }
__device__ __forceinline__ void narrow(c64 a, c32 *out) { *out = c32{(float)a.re, (float)a.im}; }
__device__ __forceinline__ void narrow(c64 a, c64 *out) { *out = a; }
__device__ __forceinline__ double real_of(double a) { return a; }
__device__ __forceinline__ double real_of(c64 a) { return a.re; }
__device__ __forceinline__ double from_real(double r, double) { return r; }
__device__ __forceinline__ c64 from_real(double r, c64) { return c64{r, 0.0}; }
__device__ __forceinline__ double neg_of(double a) { return -a; }
__device__ __forceinline__ c64 neg_of(c64 a) { return c64{-a.re, -a.im}; }
__device__ __forceinline__ double div_real(double a, double r) { return a / r; }
__device__ __forceinline__ c64 div_real(c64 a, double r) { return c64{a.re / r, a.im / r}; }
__device__ __forceinline__ double shfl_of(double a, int src, int width) { return __shfl(a, src, width); }
__device__ __forceinline__ c64 shfl_of(c64 a, int src, int width) { return c64{__shfl(a.re, src, width), __shfl(a.im, src, width)}; }

// d^(-1/2), correctly rounded up to the rarest of ties: 1 / sqrt(d) (two roundings) and one Newton step whose
// residual 1 - d g^2 is formed without rounding d g (its low part comes from a fused multiply-add)
__device__ __forceinline__ double inv_sqrt(double d) {
  const double g = 1.0 / sqrt(d);
  const double h = d * g, hl = fma(d, g, -h);
  double e = fma(-h, g, 1.0);
  e = fma(-hl, g, e);
  return fma(0.5 * g, e, g);
}

__device__ __forceinline__ int tri_at(int p, int q) { return q * (q + 1) / 2 + p; }     // p <= q, packed by columns

// threads of a set-up workgroup: the packed triangles of its rows stay within 40 KB of LDS
template <typename T, int LANES> constexpr int setup_threads() {
  return LANES == 64 ? 64 : (LANES == 32 && sizeof(typename Wide<T>::type) == 16) ? 128 : kBlock;
}

// The local system of one row by its lane group (the set-up and every enrichment step): the columns of the pattern
// ascend in pcol[0 .. k), the rows they name begin and end at pbeg / pend, all three in the LDS and visible to the
// group.  S = A[P, P] is gathered into the packed triangle R, factorised S = R^H R and R u = e_k is solved: lane q
// returns u_q (row q of G is conj(u)).  false: S is not positive definite (the same answer in every lane).
template <typename T, int LANES>
__device__ __forceinline__ bool local_solve(int k, int lane, const int32_t *pcol, const int64_t *pbeg, const int64_t *pend,
                                            typename Wide<T>::type *R, const int32_t *__restrict__ ix,
                                            const T *__restrict__ va, typename Wide<T>::type *out) {
  using D = typename Wide<T>::type;
  // S[p, q], p <= q: the stored entry (P[p], P[q]) -- on or above the diagonal -- or 0
  const int pairs = k * (k + 1) / 2;
  for (int e = lane; e < pairs; e += LANES) {
    int q = (int)((sqrtf(8.f * (float)e + 1.f) - 1.f) * 0.5f);
    while (q * (q + 1) / 2 > e) --q;
    while ((q + 1) * (q + 2) / 2 <= e) ++q;
    const int p = e - q * (q + 1) / 2;
    const int64_t c = pcol[q], hi = pend[p];
    const int64_t f = lower_bound_col(ix, pbeg[p], hi, c);
    R[e] = (f < hi && (int64_t)ix[f] == c) ? widen(va[f]) : from_real(0.0, D());
  }
  wave_sync();
  // S = R^H R row by row: lane q holds column q; R[p, q] = (S[p, q] - sum_{t < p} conj(R[t, p]) R[t, q]) / R[p, p]
  double last = 1.0;
  for (int p = 0; p < k; ++p) {
    D acc = from_real(0.0, D());
    const bool mine = lane >= p && lane < k;
    if (mine) {
      acc = R[tri_at(p, lane)];
      for (int t = 0; t < p; ++t) fma_conj_acc(acc, R[tri_at(t, p)], neg_of(R[tri_at(t, lane)]));
    }
    const double d = __shfl(real_of(acc), p, LANES);
    if (!(d > 0.0) || !(d < INFINITY)) return false;                     // (the same decision in every lane of the group)
    last = d;
    const double r = sqrt(d);
    if (mine) R[tri_at(p, lane)] = lane == p ? from_real(r, D()) : div_real(acc, r);
    wave_sync();
  }
  // R u = e_k from the last column back; lane p carries the right-hand side of row p
  D rhs = from_real(0.0, D()), u = from_real(0.0, D());
  for (int q = k - 1; q >= 0; --q) {
    const D cand = q == k - 1 ? from_real(inv_sqrt(last), D()) : div_real(rhs, real_of(R[tri_at(q, q)]));
    const D uq = shfl_of(cand, q, LANES);
    if (lane == q) u = uq;
    if (lane < q) fma_acc(rhs, R[tri_at(lane, q)], neg_of(uq));
  }
  *out = u;
  return true;
}

template <typename T, int LANES>
__global__ __launch_bounds__((setup_threads<T, LANES>())) void fsai_setup(int64_t nlist, const int32_t *__restrict__ list,
                                                                        const int64_t *__restrict__ ip,
                                                                        const int32_t *__restrict__ ix, const T *__restrict__ va,
                                                                        const int64_t *__restrict__ gp,
                                                                        const int32_t *__restrict__ gi, T *__restrict__ gv,
                                                                        FsaiStatus *st) {
  using D = typename Wide<T>::type;
  constexpr int kThreads = setup_threads<T, LANES>(), kGroups = kThreads / LANES, kTri = LANES * (LANES + 1) / 2;
  __shared__ D tri[kGroups][kTri];
  __shared__ int32_t pcol[kGroups][LANES];
  __shared__ int64_t pbeg[kGroups][LANES], pend[kGroups][LANES];
  const int grp = threadIdx.x / LANES, lane = threadIdx.x % LANES;
  for (int64_t s = (int64_t)blockIdx.x * kGroups + grp; s < nlist; s += (int64_t)gridDim.x * kGroups) {
    const int64_t i = list[s];
    const int64_t g0 = gp[i];
    const int k = (int)(gp[i + 1] - g0);             // 1 <= k <= LANES: the bins are made from these counts
    wave_sync();                                     // (the row before this one is done with the LDS)
    if (lane < k) {
      const int32_t c = gi[g0 + lane];
      pcol[grp][lane] = c;
      pbeg[grp][lane] = ip[c];
      pend[grp][lane] = ip[c + 1];
    }
    wave_sync();
    D u;
    if (!local_solve<T, LANES>(k, lane, pcol[grp], pbeg[grp], pend[grp], tri[grp], ix, va, &u)) {
      if (lane == 0) build_error(st, kErrNotPd, i);
      continue;
    }
    if (lane < k) narrow(dev_conj(u), &gv[g0 + lane]);
  }
}

// ---------------------------------------------------------------- adaptive patterns: enrichment by Kaporin gradient

// The sum over the lanes of a group, the same bits in every lane.  Partners at distance 1, 2, 4, ..: a row of k
// members leaves exact zeros in the lanes from k on, so the rounded partial sums -- and the result -- are those of
// every group width that holds the row: the sum does not depend on the row's bin.
template <int LANES> __device__ __forceinline__ double group_sum(double v) {
  for (int o = 1; o < LANES; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <int LANES> __device__ __forceinline__ c64 group_sum(c64 v) { return c64{group_sum<LANES>(v.re), group_sum<LANES>(v.im)}; }

__device__ __forceinline__ double abs2_of(double a) { return a * a; }
__device__ __forceinline__ double abs2_of(c64 a) { return fma(a.re, a.re, a.im * a.im); }

// `steps` enrichment steps on the level pattern of every row of one bin (LANES lanes per row: the row's capacity
// min(max_row, k0 + steps * step_size) is at most LANES).  One step on the pattern P (ascending in the LDS, i its last
// member): solve S y = e_last (local_solve: g = conj(u) is a positive multiple of y^H, lane q keeps g_q in a register);
// then lane q walks the stored entries of row P[q] downwards from column i - 1, the group's maximum of the columns the
// lanes show is the next candidate j (descending, each once; members of P are passed over), the lanes that show it
// contribute g_p a_pj -- a_pj read at (p, j) for j > p, as conj of (j, p) for j < p: never below the diagonal -- and
// r_j is their group_sum.  score_j = |r_j|^2 / a_jj; lane t holds the t-th best (score, column) so far, a new one goes
// behind those that are not smaller (they have larger columns).  The taken columns are appended and the pattern is
// sorted by ranks.  The final pattern goes to slab[sp[i] ..), its length and the keys of its bin to cnt, ka, kb.
// Every decision is the group's (the same in each of its lanes); st->limited counts rows max_row held back.
template <typename T, int LANES>
__global__ __launch_bounds__((setup_threads<T, LANES>())) void fsai_enrich(
    int64_t nlist, const int32_t *__restrict__ list, int max_row, int steps, int step_size, int four,
    const int64_t *__restrict__ ip, const int32_t *__restrict__ ix, const T *__restrict__ va, const int64_t *__restrict__ gp0,
    const int32_t *__restrict__ gi0, const int64_t *__restrict__ sp, int32_t *__restrict__ slab, int64_t *__restrict__ cnt,
    int64_t *__restrict__ ka, int64_t *__restrict__ kb, FsaiStatus *st) {
  using D = typename Wide<T>::type;
  constexpr int kThreads = setup_threads<T, LANES>(), kGroups = kThreads / LANES, kTri = LANES * (LANES + 1) / 2;
  __shared__ D tri[kGroups][kTri];
  __shared__ int32_t pcol[kGroups][LANES];
  __shared__ int64_t pbeg[kGroups][LANES], pend[kGroups][LANES];
  static_assert(sizeof(D) * kGroups * kTri + 20 * kThreads <= 40 * 1024, "the LDS of a workgroup");
  const int grp = threadIdx.x / LANES, lane = threadIdx.x % LANES;
  const int base = (threadIdx.x & 63) - lane;          // the group's first lane within its wave
  constexpr unsigned long long kGroupMask = LANES == 64 ? ~0ull : ((1ull << (LANES & 63)) - 1);
  int32_t *P = pcol[grp];
  for (int64_t s = (int64_t)blockIdx.x * kGroups + grp; s < nlist; s += (int64_t)gridDim.x * kGroups) {
    const int64_t i = list[s];
    const int64_t g0 = gp0[i], s0 = sp[i];
    int k = (int)(gp0[i + 1] - g0);                    // 1 <= k <= capacity <= LANES
    const int room = (int)(sp[i + 1] - s0);            // the row's capacity
    wave_sync();                                       // (the row before this one is done with the LDS)
    if (lane < k) P[lane] = gi0[g0 + lane];
    bool limited = false, bad = false;
    for (int step = 0; step < steps; ++step) {
      if (k >= max_row) { limited = true; break; }     // full before this step begins
      if (k >= room) break;                            // (k < max_row: capacity left for every step; never taken)
      wave_sync();
      if (lane < k) {
        const int32_t c = P[lane];
        pbeg[grp][lane] = ip[c];
        pend[grp][lane] = ip[c + 1];
      }
      wave_sync();
      D u;
      if (!local_solve<T, LANES>(k, lane, P, pbeg[grp], pend[grp], tri[grp], ix, va, &u)) { bad = true; break; }
      const D g = dev_conj(u);
      const int take = min(step_size, room - k);                    // = min(step_size, max_row - k); 1 <= take < LANES
      int64_t beg = 0, pos = -1, own = -1;
      if (lane < k) {
        own = P[lane];
        beg = pbeg[grp][lane];
        pos = lower_bound_col(ix, beg, pend[grp][lane], i) - 1;     // the last stored column below i
      }
      int cand = pos >= beg ? ix[pos] : -1;
      int member = k - 1, held = 0, positive = 0, my_col = -1;
      double my_score = 0.0;
      for (;;) {
        const int j = group_max<LANES>(cand);          // the largest column not yet seen: the same in every lane
        if (j < 0) break;
        while (member >= 0 && P[member] > j) --member;
        const bool show = cand == j;
        if (member < 0 || P[member] != j) {
          const int64_t jb = ip[j], je = ip[j + 1];
          D term = from_real(0.0, D());
          if (show) {
            D a = from_real(0.0, D());
            if ((int64_t)j > own) {
              a = widen(va[pos]);
            } else {                                   // the partner (j, own) above the diagonal (fsai_count saw it)
              const int64_t f = lower_bound_col(ix, jb, je, own);
              if (f < je && (int64_t)ix[f] == own) a = dev_conj(widen(va[f]));
            }
            fma_acc(term, g, a);
          }
          const D r = group_sum<LANES>(term);
          const int64_t fd = lower_bound_col(ix, jb, je, j);
          const double ajj = (fd < je && ix[fd] == j) ? real_of(widen(va[fd])) : 0.0;
          const double score = abs2_of(r) / ajj;
          if (score > 0.0 && score < INFINITY) {
            ++positive;
            const unsigned long long ahead = __ballot(lane < held && my_score >= score);
            const int at = __popcll((ahead >> base) & kGroupMask);
            if (at < take) {
              const double up_score = __shfl_up(my_score, 1, LANES);
              const int up_col = __shfl_up(my_col, 1, LANES);
              if (lane == at) {
                my_score = score;
                my_col = j;
              } else if (lane > at) {
                my_score = up_score;
                my_col = up_col;
              }
              if (held < take) ++held;
            }
          }
        }
        if (show) {
          --pos;
          cand = pos >= beg ? ix[pos] : -1;
        }
      }
      if (max_row - k < min(step_size, positive)) limited = true;    // fewer taken than offered, for lack of room
      if (!held) break;                                // nothing to take: the row stops
      // the taken columns behind the pattern, then every member to its rank
      wave_sync();
      if (lane < held) P[k + lane] = my_col;
      wave_sync();
      k += held;
      int32_t v = 0;
      int rank = 0;
      if (lane < k) {
        v = P[lane];
        for (int t = 0; t < k; ++t) rank += P[t] < v ? 1 : 0;
      }
      wave_sync();
      if (lane < k) P[rank] = v;
    }
    wave_sync();
    if (lane < k) slab[s0 + lane] = P[lane];
    if (lane == 0) {
      cnt[i] = k;
      bin_keys(k, four, &ka[i], &kb[i]);
      if (limited) atomicAdd(&st->limited, 1ull);
      atomicMax(&st->longest, k);
      if (bad) build_error(st, kErrNotPd, i);
    }
  }
}

// per row the capacity min(max_row, k + grow) of an enriched pattern
__global__ __launch_bounds__(kBlock) void fsai_capacity(int64_t n, int max_row, int grow, const int64_t *__restrict__ cnt,
                                                        int64_t *__restrict__ cap) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
    cap[i] = cnt[i] + grow < max_row ? cnt[i] + grow : max_row;
}

// ---------------------------------------------------------------- post-filtration by value
constexpr int kFilterLanes = 8;                // lanes per row of fsai_filter: 32 rows per workgroup

// the real diagonal of A in double (fsai_count saw it stored)
template <typename T>
__global__ __launch_bounds__(kBlock) void fsai_diagonal(int64_t n, const int64_t *__restrict__ ip, const int32_t *__restrict__ ix,
                                                        const T *__restrict__ va, double *__restrict__ diag) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const int64_t ke = ip[i + 1], d = lower_bound_col(ix, ip[i], ke, i);
    diag[i] = (d < ke && (int64_t)ix[d] == i) ? real_of(widen(va[d])) : 0.0;
  }
}

// Row i of the computed G (k entries from gp[i] on, the diagonal last) by a group of kFilterLanes lanes: entry (i, j)
// stays iff |g_ij|^2 a_jj >= drop^2 g_ii^2 a_ii -- drop2 = drop * drop, the right-hand side formed as (drop2 * (g_ii *
// g_ii)) * a_ii, the left as |g_ij|^2 * a_jj, all in double, no division and no square root; the diagonal always stays.
// The kept columns go to slab[gp[i] ..) in their order (ranks from the group's ballot), their number and the keys of its
// bin to cnt, ka, kb.  The decision reads row i of G and the diagonal of A only.  The groups of a wave run different
// trip counts: nothing but the ballot crosses lanes, and a group reads only its own bits of it.
template <typename T>
__global__ __launch_bounds__(kBlock) void fsai_filter(int64_t n, double drop2, int four, const int64_t *__restrict__ gp,
                                                      const int32_t *__restrict__ gi, const T *__restrict__ gv,
                                                      const double *__restrict__ diag, int32_t *__restrict__ slab,
                                                      int64_t *__restrict__ cnt, int64_t *__restrict__ ka,
                                                      int64_t *__restrict__ kb, FsaiStatus *st) {
  constexpr int kRows = kBlock / kFilterLanes;
  const int lane = threadIdx.x % kFilterLanes;
  const int base = (threadIdx.x & 63) - lane;          // the group's first lane within its wave
  for (int64_t i = (int64_t)blockIdx.x * kRows + threadIdx.x / kFilterLanes; i < n; i += (int64_t)gridDim.x * kRows) {
    const int64_t g0 = gp[i];
    const int k = (int)(gp[i + 1] - g0);               // 1 <= k <= max_row
    const double gii = k > 0 ? real_of(widen(gv[g0 + k - 1])) : 0.0;
    const double bar = (drop2 * (gii * gii)) * diag[i];
    int kept = 0;
    for (int t0 = 0; t0 < k; t0 += kFilterLanes) {
      const int t = t0 + lane;
      bool keep = false;
      int32_t c = 0;
      if (t < k) {
        c = gi[g0 + t];
        keep = t == k - 1 || abs2_of(widen(gv[g0 + t])) * diag[c] >= bar;
      }
      const unsigned mine = (unsigned)(__ballot(keep) >> base) & ((1u << kFilterLanes) - 1);
      if (keep) slab[g0 + kept + __popc(mine & ((1u << lane) - 1))] = c;
      kept += __popc(mine);
    }
    if (lane == 0) {
      cnt[i] = kept;
      bin_keys(kept, four, &ka[i], &kb[i]);
      if (kept < k) atomicAdd(&st->removed, (unsigned long long)(k - kept));
      atomicMax(&st->kept_longest, kept);
    }
  }
}

// ---------------------------------------------------------------- prefiltration: the strong lower structure
constexpr int kStrongLanes = 8;                // lanes per row of fsai_strong: 32 rows per workgroup

// |a|^2 as re^2 + im^2, each product and the sum rounded on its own
__device__ __forceinline__ double abs2_plain(double a) { return a * a; }
__device__ __forceinline__ double abs2_plain(c64 a) {
#pragma clang fp contract(off)
  const double r = a.re * a.re, s = a.im * a.im;
  return r + s;
}

// Row i of A by a group of kStrongLanes lanes: the stored entry (i, j), j < i, is strong iff its partner a_ji (row j,
// above the diagonal: nothing below it is read) has |a_ji|^2 >= (tau2 * a_ii) * a_jj -- tau2 = prefilter * prefilter,
// all in double, no division and no square root; false where a NaN takes part, and where the partner is missing (then
// fsai_count has recorded the error).  FILL = false: cnt[i] = the members of L_tau(i), the strong columns and the
// diagonal; the weak entries go to st->weak.  FILL = true (the same decisions again, after the scan sp of the counts):
// the strong columns in their order (ranks from the group's ballot) and then i go to six[sp[i] ..): the CSR of the
// strong lower triangle, the diagonal last in each row, which the pattern kernels walk in place of A.  The groups of
// a wave run different trip counts: nothing but the ballot crosses lanes, and a group reads only its own bits of it.
template <typename T, bool FILL>
__global__ __launch_bounds__(kBlock) void fsai_strong(int64_t n, double tau2, const int64_t *__restrict__ ip,
                                                      const int32_t *__restrict__ ix, const T *__restrict__ va,
                                                      const double *__restrict__ diag, int64_t *__restrict__ cnt,
                                                      const int64_t *__restrict__ sp, int32_t *__restrict__ six, FsaiStatus *st) {
  if (!FILL && failed(st)) return;
  constexpr int kRows = kBlock / kStrongLanes;
  const int lane = threadIdx.x % kStrongLanes;
  const int base = (threadIdx.x & 63) - lane;          // the group's first lane within its wave
  for (int64_t i = (int64_t)blockIdx.x * kRows + threadIdx.x / kStrongLanes; i < n; i += (int64_t)gridDim.x * kRows) {
    const int64_t kb = ip[i], d = lower_bound_col(ix, kb, ip[i + 1], i);      // [kb, d): the entries below the diagonal
    const double bar = tau2 * diag[i];
    const int64_t s0 = FILL ? sp[i] : 0, room = FILL ? sp[i + 1] - s0 : 0;
    int64_t kept = 0;
    for (int64_t e0 = kb; e0 < d; e0 += kStrongLanes) {
      const int64_t e = e0 + lane;
      bool strong = false;
      int32_t j = 0;
      if (e < d) {
        j = ix[e];
        const int64_t je = ip[j + 1], f = lower_bound_col(ix, ip[j], je, i);
        strong = f < je && (int64_t)ix[f] == i && abs2_plain(widen(va[f])) >= bar * diag[j];
      }
      const unsigned mine = (unsigned)(__ballot(strong) >> base) & ((1u << kStrongLanes) - 1);
      if (FILL && strong) {
        const int64_t at = kept + __popc(mine & ((1u << lane) - 1));
        if (at < room) six[s0 + at] = j;               // (always: the decisions are the counting pass's)
      }
      kept += __popc(mine);
    }
    if (lane == 0) {
      if (FILL) {
        if (kept < room) six[s0 + kept] = (int32_t)i;
      } else {
        cnt[i] = kept + 1;
        if (kept < d - kb) atomicAdd(&st->weak, (unsigned long long)(d - kb - kept));
      }
    }
  }
}

// ---------------------------------------------------------------- the host side
// RLH_FSAI_BINS=0: the two bins of 8 and 64 lanes per row
int four_bins() {
  const char *e = getenv("RLH_FSAI_BINS");
  return (e && e[0] == '0' && e[1] == 0) ? 0 : 1;
}

// What a build is asked to do, made by the entry points from the makers below: an entry point names the arguments it
// has, and those are the ones check_create_args checks (adaptive: steps and step_size; filtered: drop; thresholded:
// prefilter).  What an entry point does not have stays 0.  four: read from the environment by every create call.
struct FsaiPlan {
  int max_row = 0, levels = 1;
  bool adaptive = false;
  int steps = 0, step_size = 0;
  double drop = 0.0;
  bool filtered = false;
  double prefilter = 0.0;
  bool thresholded = false;
  int four = four_bins();
  int grow() const { return steps * step_size; }       // what enrichment can add to a row

  static FsaiPlan of_levels(int max_row, int levels) { FsaiPlan p; p.max_row = max_row; p.levels = levels; return p; }
  FsaiPlan enriched(int s, int size) const { FsaiPlan p = *this; p.adaptive = true; p.steps = s; p.step_size = size; return p; }
  FsaiPlan filtered_by(double d) const { FsaiPlan p = *this; p.filtered = true; p.drop = d; return p; }
  FsaiPlan thresholded_by(double tau) const { FsaiPlan p = *this; p.thresholded = true; p.prefilter = tau; return p; }
  // steps == 0: no enrichment, step_size is not looked at
  FsaiPlan enriched_unless_0(int s, int size) const { return s != 0 ? enriched(s, size) : *this; }
  // drop == 0: no post-filtration (anything else, a NaN included, is checked as a drop)
  FsaiPlan filtered_unless_0(double d) const { return d == 0.0 ? *this : filtered_by(d); }
};

// The device arrays that pattern_totals works on and the events of one build or update: released when it returns,
// however it returns.
struct FsaiScratch {
  DevBuf<FsaiStatus> status;
  DevBuf<int64_t> cnt, ka, kb;            // per row: kept entries and the keys of the bin,
  DevBuf<int64_t> gp, sa, sb, bsum;       // their exclusive scans and the scans' tile sums
  StreamTimer timer;
  int alloc_rows(int64_t n) {             // everything above but the status record, for n rows
    for (DevBuf<int64_t> *p : {&cnt, &ka, &kb})
      if (int rc = p->alloc(n)) return rc;
    for (DevBuf<int64_t> *p : {&gp, &sa, &sb})
      if (int rc = p->alloc(n + 1)) return rc;
    return bsum.alloc((n + kScanTile - 1) / kScanTile + 1);
  }
};

// What the kernels found wrong, as the message of `name`: this build's own codes here, the shared ones by report_input
// (device_build.h).  cap: the entries the index and value arrays can hold.
int report(const char *name, const FsaiStatus &s, int64_t cap) {
  if (report_input(name, s, cap)) return 1;
  const long long pos = (long long)(s.err & kPosMask);
  if ((int)(s.err >> 56) == kErrDiag) set_error("%s: row %lld does not store its diagonal entry", name, pos);
  else set_error("%s: local block of row %lld is not positive definite", name, pos);
  return 1;
}

// One kernel over the rows of one bin, a group of LANES lanes per row: kernel(count, list, args...)
template <typename T, int LANES, typename Kernel, typename... Args>
void launch_bin(Kernel kernel, int64_t count, const int32_t *list, Args... args) {
  if (!count) return;
  constexpr int kThreads = setup_threads<T, LANES>();
  const int64_t most = (int64_t)ctx().num_cu * kSetupBlocksPerCu;
  hipLaunchKernelGGL(kernel, dim3(blocks_for(count, kThreads / LANES, most)), dim3(kThreads), 0, ctx().stream, count, list, args...);
}

// visit(lanes, count, list) for the bins of 8, 16, 32 and 64 lanes per row in turn; lanes is a std::integral_constant
template <typename Visit> void for_each_bin(const Bins &b, int64_t n, Visit visit) {
  visit(std::integral_constant<int, kShort>(), b.c8, b.rows);
  visit(std::integral_constant<int, 16>(), b.c16 - b.c8, b.rows + b.c8);
  visit(std::integral_constant<int, 32>(), b.c32 - b.c16, b.rows + b.c16);
  visit(std::integral_constant<int, kMaxRow>(), n - b.c32, b.rows + b.c32);
}

// The counts and keys of the rows (w.cnt, w.ka, w.kb) are scanned into w.gp, w.sa, w.sb; the host waits for the stream
// and reports what the kernels found so far.  *hs: the status record; *gnnz: the entries of the pattern, which must lie
// in [lo, hi]; bins: the scans and the totals of the keys.
int pattern_totals(const char *name, int64_t n, const FsaiScratch &w, int64_t cap, int64_t lo, int64_t hi, FsaiStatus *hs,
                   int64_t *gnnz, Bins *bins) {
  hipStream_t st = ctx().stream;
  if (int rc = exclusive_scan(n, w.cnt, w.bsum, w.gp)) return rc;
  if (int rc = exclusive_scan(n, w.ka, w.bsum, w.sa)) return rc;
  if (int rc = exclusive_scan(n, w.kb, w.bsum, w.sb)) return rc;
  int64_t tot[3] = {0, 0, 0};
  RLH_HIP(hipMemcpyAsync(hs, w.status, sizeof *hs, hipMemcpyDeviceToHost, st));
  RLH_HIP(hipMemcpyAsync(&tot[0], w.gp + n, 8, hipMemcpyDeviceToHost, st));
  RLH_HIP(hipMemcpyAsync(&tot[1], w.sa + n, 8, hipMemcpyDeviceToHost, st));
  RLH_HIP(hipMemcpyAsync(&tot[2], w.sb + n, 8, hipMemcpyDeviceToHost, st));
  RLH_HIP(hipStreamSynchronize(st));
  if (hs->err != kNoError) return report(name, *hs, cap);
  const int64_t c8 = tot[1] & 0xffffffff, c16 = tot[1] >> 32, c32 = tot[2];
  RLH_REQUIRE(tot[0] >= lo && tot[0] <= hi && c8 >= 0 && c8 <= c16 && c16 <= c32 && c32 <= n,
              "%s: inconsistent row counts of the pattern", name);
  *gnnz = tot[0];
  *bins = Bins{w.sa, w.sb, c8, c16, c32, bins->rows};
  return 0;
}

// The checks of a build and of an update on ip, ix, va (device arrays, n >= 1) and the arrays as the kernels read them:
// the four steps of device_build.h in a row.  *hs is the record as the host saw it last.
template <typename T, typename P, typename I>
int checked_input(const char *name, int64_t n, const P *ip, const I *ix, const T *va, FsaiScratch &w, FsaiStatus *hs, CsrInput *in) {
  if (int rc = input_cap(name, "n", n, ip, ix, va, &in->cap)) return rc;
  if (int rc = launch_input_checks<false>(n, n, ip, ix, in->cap, w.status, hs)) return rc;
  if (int rc = fetch_input_status(name, w.status.get(), hs, in->cap)) return rc;
  in->nnz = hs->nnz;
  return normalise_indices(n, ip, ix, in);
}

// Every row solved on its pattern, bin by bin (the pattern of gp and `columns`, the bins as they stand, the values to
// `values`); the host waits and reports what the kernels found.
template <typename T>
int solve_rows(const char *name, int64_t n, const Bins &bins, const CsrInput &in, const T *va, const int64_t *gp, const int32_t *columns,
               T *values, const FsaiScratch &w, FsaiStatus *hs) {
  hipStream_t st = ctx().stream;
  for_each_bin(bins, n, [&](auto lanes, int64_t count, const int32_t *list) {
    constexpr int kLanes = decltype(lanes)::value;
    launch_bin<T, kLanes>(fsai_setup<T, kLanes>, count, list, in.ip64, in.ix32, va, gp, columns, values, w.status.get());
  });
  RLH_HIP(hipGetLastError());
  RLH_HIP(hipMemcpyAsync(hs, w.status, sizeof *hs, hipMemcpyDeviceToHost, st));
  RLH_HIP(hipStreamSynchronize(st));
  return hs->err != kNoError ? report(name, *hs, in.cap) : 0;
}

// One build: the arrays its stages hand to each other, and the stages in the order fsai_build runs them.  The state
// owns every array until the build returns, however it returns (device_release waits for the device); the two releases
// before that are named where they happen (post_filter, make_operator).  ip, ix, va: device arrays, n >= 1.
template <typename T> struct FsaiBuild {
  rlh_fsai *const h;
  const char *const name;                  // the entry point the messages speak for
  const T *const va;
  const FsaiPlan &plan;
  const int64_t n = h->n;
  // decided once: the level pattern is a slice of A's row (fsai_count tallies, fsai_fill copies from `start` on), or
  // one wave per row walks pat_ip / pat_ix (fsai_pattern_count, fsai_pattern_fill)
  const bool slice = plan.levels == 1 && !(plan.prefilter > 0);
  const hipStream_t st = ctx().stream;
  const dim3 blk{kBlock};
  const int64_t most = (int64_t)ctx().num_cu * kSetupBlocksPerCu;
  FsaiScratch w;                           // counts, keys, scans (w.gp: G's row pointers), the status record on the device
  FsaiStatus hs{};                         // the status record as last fetched
  CsrInput in;
  DevBuf<int64_t> start;
  DevBuf<double> strong_diag;              // prefiltration: A's diagonal and the strong lower structure (a CSR)
  DevBuf<int64_t> strong_ip;
  DevBuf<int32_t> strong_ix;
  const int64_t *pat_ip = nullptr;         // the structure the pattern is the power of: A's own arrays (checks) or the
  const int32_t *pat_ix = nullptr;         // strong lower structure (strong_structure)
  DevBuf<int32_t> gi, bin_rows;            // G's columns; the rows of the bins
  DevBuf<T> gv;
  Bins bins{};
  int64_t gnnz = 0;                        // the entries of the pattern as it stands
  DevBuf<int64_t> capacity, sp;            // enrichment: the rows' capacities, their scan, the slab of the enriched
  DevBuf<int32_t> slab, level;             // patterns and the level patterns the rows grew from

  dim3 by_row() const { return dim3(blocks_for(n, kBlock, 8192)); }

  // ---- checks: the arrays as they came, then per row the diagonal and the partners (fsai_count; for a slice also the
  // counts, the keys and where the slice begins)
  template <typename P, typename I> int checks(const P *ip, const I *ix) {
    if (int rc = checked_input(name, n, ip, ix, va, w, &hs, &in)) return rc;
    if (int rc = w.alloc_rows(n)) return rc;
    if (int rc = start.alloc(n)) return rc;
    if (int rc = bin_rows.alloc(n)) return rc;
    hipLaunchKernelGGL(fsai_count, by_row(), blk, 0, st, n, plan.max_row, slice ? 1 : 0, plan.four, plan.grow(), in.ip64, in.ix32,
                       w.cnt, w.ka, w.kb, start, w.status);
    hipLaunchKernelGGL((resolve_partner<int64_t, int32_t>), dim3(1), dim3(1), 0, st, n, in.ip64, in.ix32, w.status);
    pat_ip = in.ip64;
    pat_ix = in.ix32;
    return 0;
  }

  // ---- prefiltration: every lower entry is decided by value (counts in w.cnt, which the pattern overwrites later), the
  // counts are scanned, the host waits once for the size and for what the checks found, and the strong lower structure
  // is filled.  The pattern kernels of every level, 1 included, walk it in place of A.
  int strong_structure() {
    const double tau2 = plan.prefilter * plan.prefilter;
    const dim3 grid(blocks_for(n, kBlock / kStrongLanes, most));
    if (int rc = strong_diag.alloc(n)) return rc;
    if (int rc = strong_ip.alloc(n + 1)) return rc;
    hipLaunchKernelGGL(fsai_diagonal<T>, by_row(), blk, 0, st, n, in.ip64, in.ix32, va, strong_diag.get());
    hipLaunchKernelGGL((fsai_strong<T, false>), grid, blk, 0, st, n, tau2, in.ip64, in.ix32, va, (const double *)strong_diag,
                       w.cnt.get(), (const int64_t *)nullptr, (int32_t *)nullptr, w.status.get());
    RLH_HIP(hipGetLastError());
    if (int rc = exclusive_scan(n, w.cnt, w.bsum, strong_ip)) return rc;
    int64_t members = 0;
    RLH_HIP(hipMemcpyAsync(&hs, w.status, sizeof hs, hipMemcpyDeviceToHost, st));
    RLH_HIP(hipMemcpyAsync(&members, strong_ip + n, 8, hipMemcpyDeviceToHost, st));
    RLH_HIP(hipStreamSynchronize(st));
    if (hs.err != kNoError) return report(name, hs, in.cap);
    RLH_REQUIRE(members >= n && members <= in.nnz && (int64_t)hs.weak + members <= in.nnz, "%s: inconsistent row counts of the pattern", name);
    if (int rc = strong_ix.alloc(members)) return rc;
    hipLaunchKernelGGL((fsai_strong<T, true>), grid, blk, 0, st, n, tau2, in.ip64, in.ix32, va, (const double *)strong_diag,
                       (int64_t *)nullptr, (const int64_t *)strong_ip, strong_ix.get(), w.status.get());
    RLH_HIP(hipGetLastError());
    pat_ip = strong_ip;
    pat_ix = strong_ix;
    h->weak = (int64_t)hs.weak;
    return 0;
  }

  // The counts and keys in w become a pattern (pattern_totals: one wait; its entries must lie in [lo, hi]) with a column
  // array of its size
  int new_columns(int64_t lo, int64_t hi) {
    bins.rows = bin_rows;
    if (int rc = pattern_totals(name, n, w, in.cap, lo, hi, &hs, &gnnz, &bins)) return rc;
    return gi.alloc(gnnz);
  }

  // ... and row i of it is copied from src[src_start[i] ..): from A's own rows, from the slab of the enrichment and from
  // that of the filter (fsai_fill, which also writes the rows of the bins)
  int compact(const int32_t *src, const int64_t *src_start, int64_t lo, int64_t hi) {
    if (int rc = new_columns(lo, hi)) return rc;
    hipLaunchKernelGGL(fsai_fill, by_row(), blk, 0, st, n, src, src_start, w.gp.get(), gi.get(), bins);
    return 0;
  }

  // ---- the level pattern: counts, scans, the columns of G and the rows of the bins (a slice: fsai_count has made the
  // counts and keys)
  int level_pattern() {
    const int64_t hi = n * (int64_t)plan.max_row;
    const dim3 grid(blocks_for(n, kBlock / 64, most));
    if (!slice)
      hipLaunchKernelGGL(fsai_pattern_count, grid, blk, 0, st, n, plan.max_row, plan.levels, plan.four, plan.grow(), pat_ip, pat_ix,
                         w.cnt, w.ka, w.kb, w.status);
    if (int rc = slice ? compact(in.ix32, start, n, hi) : new_columns(n, hi)) return rc;
    if (!slice) hipLaunchKernelGGL(fsai_pattern_fill, grid, blk, 0, st, n, plan.max_row, plan.levels, pat_ip, pat_ix, w.gp, gi, bins);
    h->truncated = (int64_t)hs.truncated;
    h->longest = hs.longest;
    return 0;
  }

  // ---- enrichment: so far the bins are those of the capacities and gi holds the level patterns.  The enriched patterns
  // go to a slab at the scanned capacities (one wait, for their total); counts, keys and scans are then made again for
  // the final rows and the slab is compacted.
  int enrich() {
    if (int rc = capacity.alloc(n)) return rc;
    if (int rc = sp.alloc(n + 1)) return rc;
    hipLaunchKernelGGL(fsai_capacity, by_row(), blk, 0, st, n, plan.max_row, plan.grow(), w.cnt, capacity);
    if (int rc = exclusive_scan(n, capacity, w.bsum, sp)) return rc;
    int64_t room = 0;
    RLH_HIP(hipMemcpyAsync(&room, sp + n, 8, hipMemcpyDeviceToHost, st));
    RLH_HIP(hipStreamSynchronize(st));
    RLH_REQUIRE(room >= gnnz && room <= n * (int64_t)plan.max_row, "%s: inconsistent row counts of the pattern", name);
    if (int rc = slab.alloc(room)) return rc;
    level = std::move(gi);                 // the level patterns the rows grow from
    for_each_bin(bins, n, [&](auto lanes, int64_t count, const int32_t *list) {
      constexpr int kLanes = decltype(lanes)::value;
      launch_bin<T, kLanes>(fsai_enrich<T, kLanes>, count, list, plan.max_row, plan.steps, plan.step_size, plan.four, in.ip64, in.ix32, va,
                            w.gp.get(), (const int32_t *)level, sp.get(), slab.get(), w.cnt.get(), w.ka.get(), w.kb.get(),
                            w.status.get());
    });
    RLH_HIP(hipGetLastError());
    if (int rc = compact(slab, sp, gnnz, room)) return rc;      // (the kernels above are done with w.gp when the scans write it)
    h->truncated = (int64_t)hs.limited;    // of an enriched build: the rows max_row held back
    h->longest = hs.longest;
    return 0;
  }

  // ---- the rows, bin by bin (the pattern of w.gp and gi, the bins as they stand): one wait
  int solve() {
    if (int rc = gv.alloc(gnnz)) return rc;
    return solve_rows<T>(name, n, bins, in, va, w.gp, gi, gv, w, &hs);
  }

  // ---- post-filtration: the kept columns of every row go to a slab at the row's old offset; counts, keys and scans are
  // made again, the slab is compacted and every row is solved once more on what is left, in the bin of its new length.
  // A principal sub-block of a positive definite block is positive definite.  The unfiltered G and the stage's own
  // arrays are released when the stage returns: the second solve has waited then, the stream is idle.
  int post_filter() {
    DevBuf<double> diag;
    DevBuf<int32_t> kept_cols;
    if (int rc = diag.alloc(n)) return rc;
    if (int rc = kept_cols.alloc(gnnz)) return rc;
    hipLaunchKernelGGL(fsai_diagonal<T>, by_row(), blk, 0, st, n, in.ip64, in.ix32, va, diag.get());
    hipLaunchKernelGGL(fsai_filter<T>, dim3(blocks_for(n, kBlock / kFilterLanes, most)), blk, 0, st, n, plan.drop * plan.drop, plan.four,
                       (const int64_t *)w.gp, (const int32_t *)gi, (const T *)gv, (const double *)diag, kept_cols.get(),
                       w.cnt.get(), w.ka.get(), w.kb.get(), w.status.get());
    RLH_HIP(hipGetLastError());
    const DevBuf<int64_t> old_gp = std::move(w.gp);      // (where the rows lie in the slab; the scans write a new w.gp)
    const DevBuf<int32_t> old_gi = std::move(gi);
    const DevBuf<T> old_gv = std::move(gv);
    if (int rc = w.gp.alloc(n + 1)) return rc;
    const int64_t before = gnnz;
    if (int rc = compact(kept_cols, old_gp, n, before)) return rc;
    RLH_REQUIRE((int64_t)hs.removed == before - gnnz, "%s: inconsistent row counts of the pattern", name);
    h->removed = (int64_t)hs.removed;
    h->longest = hs.kept_longest;
    return solve();
  }

  // ---- G and G^H as one sparse data operator (it copies the arrays: 32-bit row pointers where they can hold nnz).  What
  // else the handle reports, each stage has written when it made it.
  int make_operator() {
    int rc;
    DevBuf<int32_t> gp32;
    DevBuf<int64_t> gi64;
    if (gnnz < INT32_MAX) {
      if (int rc2 = gp32.alloc(n + 1)) return rc2;
      hipLaunchKernelGGL((spd_convert_index<int64_t, int32_t>), dim3(blocks_for(n + 1, kBlock, 4096)), blk, 0, st, n + 1, w.gp, gp32);
      RLH_HIP(hipGetLastError());
      rc = rlh_spd_create_device(&h->spd, h->dtype, n, n, 32, gp32, gi, gv);
    } else {
      in.cols.reset();                  // (the set-up was the last to read the converted columns)
      if (int rc2 = gi64.alloc(gnnz)) return rc2;
      hipLaunchKernelGGL((spd_convert_index<int32_t, int64_t>), dim3(blocks_for(gnnz, kBlock, 8192)), blk, 0, st, gnnz, gi, gi64);
      rc = rlh_spd_create_device(&h->spd, h->dtype, n, n, 64, w.gp, gi64, gv);
    }
    if (rc) return rc;
    if (int rc2 = w.timer.stop()) return rc2;   // the caller's arrays and the scratch are not referenced after the return
    h->setup_seconds = w.timer.seconds();
    h->nnz = gnnz;
    return 0;
  }
};

template <typename T, typename P, typename I>
int fsai_build(rlh_fsai *h, const char *name, const P *ip, const I *ix, const T *va, const FsaiPlan &plan) {
  FsaiBuild<T> b{h, name, va, plan};
  if (int rc = b.w.timer.start()) return rc;
  if (int rc = b.checks(ip, ix)) return rc;
  if (plan.prefilter > 0)
    if (int rc = b.strong_structure()) return rc;
  if (int rc = b.level_pattern()) return rc;
  if (plan.steps > 0)
    if (int rc = b.enrich()) return rc;
  if (int rc = b.solve()) return rc;
  if (plan.drop > 0)
    if (int rc = b.post_filter()) return rc;
  return b.make_operator();
}

// f(values as const T *) for the T of `dtype`
template <typename F> int with_values(int dtype, const void *va, F f) {
  switch (dtype) {
    case RLH_S: return f((const float *)va);
    case RLH_D: return f((const double *)va);
    case RLH_C: return f((const c32 *)va);
    case RLH_Z: return f((const c64 *)va);
  }
  return 1;
}

// New values on the pattern the handle has (rlh_fsvalues_update*): the checks of a build on the new arrays (no partner
// check: nothing below the diagonal is read), the bins of the rows' lengths, every row solved into scratch by the
// build's own fsai_setup and, when all succeeded, the values committed to G and G^H of the handle's operator.  What
// the update allocates is released when it returns; the handle's index arrays and partitions are not touched.
template <typename T, typename P, typename I>
int fsai_update(rlh_fsai *h, const char *name, const P *ip, const I *ix, const T *va) {
  const int64_t n = h->n;
  const int four = four_bins();
  hipStream_t st = ctx().stream;
  const dim3 blk(kBlock);
  FsaiScratch w;
  if (int rc = w.timer.start()) return rc;
  FsaiStatus hs{};
  CsrInput in;
  if (int rc = checked_input(name, n, ip, ix, va, w, &hs, &in)) return rc;
  const SpdArrays g = spd_arrays(h->spd, 0);
  const unsigned grid = blocks_for(n, kBlock, (int64_t)ctx().num_cu * kSetupBlocksPerCu);
  if (int rc = w.alloc_rows(n)) return rc;
  hipLaunchKernelGGL(fsai_kept_rows, dim3(grid), blk, 0, st, n, four, in.ip64, in.ix32, g.indptr, w.cnt.get(), w.ka.get(), w.kb.get(),
                     w.status.get());
  int64_t gnnz = 0;
  Bins bins{};
  if (int rc = pattern_totals(name, n, w, in.cap, g.nnz, g.nnz, &hs, &gnnz, &bins)) return rc;
  DevBuf<int32_t> bin_rows;
  DevBuf<T> gv;
  if (int rc = bin_rows.alloc(n)) return rc;
  if (int rc = gv.alloc(gnnz)) return rc;
  bins.rows = bin_rows;
  hipLaunchKernelGGL(fsai_bin_rows, dim3(grid), blk, 0, st, n, bins);
  if (int rc = solve_rows<T>(name, n, bins, in, va, g.indptr, g.idx, gv, w, &hs)) return rc;
  // ---- every row succeeded: the new values go to the operator
  if (int rc = spd_set_values(h->spd, gv)) return rc;
  if (int rc = w.timer.stop()) return rc;    // the caller's arrays and the scratch are not referenced after the return
  h->update_seconds = w.timer.seconds();
  ++h->updates;
  return 0;
}

template <typename P, typename I>
int update_as(rlh_fsai *h, const char *name, const void *ip, const void *ix, const void *va) {
  if (h->n == 0 || !h->spd) {               // nothing to solve: a valid update
    h->update_seconds = 0;
    ++h->updates;
    return 0;
  }
  return with_values(h->dtype, va, [&](auto *v) { return fsai_update(h, name, (const P *)ip, (const I *)ix, v); });
}

constexpr int kMaxSteps = 63, kMaxStepSize = 16;

int check_create_args(const char *name, rlh_fsai_t *ph, int dtype, int64_t n, const void *indptr, const FsaiPlan &plan) {
  RLH_REQUIRE(ph != nullptr, "%s: null handle pointer", name);
  *ph = nullptr;
  RLH_REQUIRE(dtype_valid(dtype), "%s: unknown dtype %d", name, dtype);
  RLH_REQUIRE(n >= 0 && n < INT32_MAX, "%s: the size must lie in [0, 2^31 - 1)", name);
  RLH_REQUIRE(plan.max_row >= 1 && plan.max_row <= kMaxRow, "%s: max_row must lie in [1, %d], got %d", name, kMaxRow, plan.max_row);
  RLH_REQUIRE(plan.levels >= 1 && plan.levels <= kMaxLevels, "%s: levels must lie in [1, %d], got %d", name, kMaxLevels, plan.levels);
  if (plan.adaptive) {
    RLH_REQUIRE(plan.steps >= 1 && plan.steps <= kMaxSteps, "%s: steps must lie in [1, %d], got %d", name, kMaxSteps, plan.steps);
    RLH_REQUIRE(plan.step_size >= 1 && plan.step_size <= kMaxStepSize, "%s: step_size must lie in [1, %d], got %d", name,
                kMaxStepSize, plan.step_size);
  }
  if (plan.filtered) RLH_REQUIRE(plan.drop > 0.0 && plan.drop < 1.0, "%s: drop must lie in (0, 1), got %g", name, plan.drop);
  if (plan.thresholded)
    RLH_REQUIRE(plan.prefilter > 0.0 && plan.prefilter < 1.0, "%s: prefilter must lie in (0, 1), got %g", name, plan.prefilter);
  RLH_REQUIRE(indptr, "%s: null indptr", name);
  return 0;
}

// The handle of a build: build(h) runs for n > 0; *ph is set when it succeeds
template <typename Build> int make_handle(rlh_fsai_t *ph, int dtype, int64_t n, const FsaiPlan &plan, Build build) {
  rlh_fsai *h = new rlh_fsai();
  h->dtype = dtype;
  h->n = n;
  h->levels = plan.levels;
  h->steps = plan.steps;
  h->step_size = plan.step_size;
  h->drop = plan.drop;
  h->prefilter = plan.prefilter;
  if (int rc = n > 0 ? build(h) : 0) {
    rlh_fsai_destroy(h);
    return rc;
  }
  *ph = h;
  return 0;
}

int create_device(const char *name, rlh_fsai_t *ph, int dtype, int64_t n, int index_bits, const void *d_indptr,
                  const void *d_indices, const void *d_values, const FsaiPlan &plan) {
  if (int rc = require_ready()) return rc;
  if (int rc = check_create_args(name, ph, dtype, n, d_indptr, plan)) return rc;
  RLH_REQUIRE(index_bits == 32 || index_bits == 64, "%s: index_bits must be 32 or 64, got %d", name, index_bits);
  return make_handle(ph, dtype, n, plan, [&](rlh_fsai *h) {
    return with_values(dtype, d_values, [&](auto *va) {
      return index_bits == 32 ? fsai_build(h, name, (const int32_t *)d_indptr, (const int32_t *)d_indices, va, plan)
                              : fsai_build(h, name, (const int64_t *)d_indptr, (const int64_t *)d_indices, va, plan);
    });
  });
}

// Host arrays (indptr not null): what decides how much is uploaded is checked here, everything else by the kernels, as
// for device arrays; then the three arrays go to the device (n == 0: nothing to upload)
struct UploadedCsr {
  DevBuf<int64_t> ip;
  DevBuf<int32_t> ix;
  DevBuf<void> va;
};
int upload_csr(const char *name, int dtype, int64_t n, const int64_t *indptr, const int32_t *indices, const void *values, UploadedCsr *d) {
  RLH_REQUIRE(indptr[0] == 0, "%s: indptr[0] must be 0", name);
  for (int64_t r = 0; r < n; ++r) RLH_REQUIRE(indptr[r + 1] >= indptr[r], "%s: indptr decreases at row %lld", name, (long long)r);
  const int64_t nnz = indptr[n], es = dtype_size(dtype);
  RLH_REQUIRE(nnz == 0 || (indices && values), "%s: null indices or values", name);
  if (n == 0) return 0;
  if (int rc = d->ip.upload(indptr, (size_t)(n + 1) * 8)) return rc;
  if (int rc = d->ix.upload(indices, (size_t)nnz * 4, 4)) return rc;
  return d->va.upload(values, (size_t)(nnz * es), 16);
}

int create_host(const char *name, rlh_fsai_t *ph, int dtype, int64_t n, const int64_t *indptr, const int32_t *indices,
                const void *values, const FsaiPlan &plan) {
  if (int rc = require_ready()) return rc;
  if (int rc = check_create_args(name, ph, dtype, n, indptr, plan)) return rc;
  UploadedCsr d;
  if (int rc = upload_csr(name, dtype, n, indptr, indices, values, &d)) return rc;
  return make_handle(ph, dtype, n, plan, [&](rlh_fsai *h) {
    return with_values(dtype, d.va, [&](auto *va) { return fsai_build(h, name, d.ip.get(), d.ix.get(), va, plan); });
  });
}

}  // namespace
}  // namespace rlh

using namespace rlh;

extern "C" int rlh_fsai_create_device(rlh_fsai_t *ph, int dtype, int64_t n, int index_bits, const void *d_indptr,
                                      const void *d_indices, const void *d_values, int max_row) {
  return create_device("rlh_fsai_create_device", ph, dtype, n, index_bits, d_indptr, d_indices, d_values, FsaiPlan::of_levels(max_row, 1));
}

extern "C" int rlh_fsai_create_levels_device(rlh_fsai_t *ph, int dtype, int64_t n, int index_bits, const void *d_indptr,
                                             const void *d_indices, const void *d_values, int max_row, int levels) {
  return create_device("rlh_fsai_create_levels_device", ph, dtype, n, index_bits, d_indptr, d_indices, d_values,
                       FsaiPlan::of_levels(max_row, levels));
}

extern "C" int rlh_fsai_create(rlh_fsai_t *ph, int dtype, int64_t n, const int64_t *indptr, const int32_t *indices,
                               const void *values, int max_row) {
  return create_host("rlh_fsai_create", ph, dtype, n, indptr, indices, values, FsaiPlan::of_levels(max_row, 1));
}

extern "C" int rlh_fsai_create_levels(rlh_fsai_t *ph, int dtype, int64_t n, const int64_t *indptr, const int32_t *indices,
                                      const void *values, int max_row, int levels) {
  return create_host("rlh_fsai_create_levels", ph, dtype, n, indptr, indices, values, FsaiPlan::of_levels(max_row, levels));
}

extern "C" int rlh_fsai_create_adaptive_device(rlh_fsai_t *ph, int dtype, int64_t n, int index_bits, const void *d_indptr,
                                               const void *d_indices, const void *d_values, int max_row, int levels, int steps,
                                               int step_size) {
  return create_device("rlh_fsai_create_adaptive_device", ph, dtype, n, index_bits, d_indptr, d_indices, d_values,
                       FsaiPlan::of_levels(max_row, levels).enriched(steps, step_size));
}

extern "C" int rlh_fsai_create_adaptive(rlh_fsai_t *ph, int dtype, int64_t n, const int64_t *indptr, const int32_t *indices,
                                        const void *values, int max_row, int levels, int steps, int step_size) {
  return create_host("rlh_fsai_create_adaptive", ph, dtype, n, indptr, indices, values,
                     FsaiPlan::of_levels(max_row, levels).enriched(steps, step_size));
}

extern "C" int rlh_fsfilter_create_device(rlh_fsai_t *ph, int dtype, int64_t n, int index_bits, const void *d_indptr,
                                               const void *d_indices, const void *d_values, int max_row, int levels, int steps,
                                               int step_size, double drop) {
  return create_device("rlh_fsfilter_create_device", ph, dtype, n, index_bits, d_indptr, d_indices, d_values,
                       FsaiPlan::of_levels(max_row, levels).enriched_unless_0(steps, step_size).filtered_by(drop));
}

extern "C" int rlh_fsfilter_create(rlh_fsai_t *ph, int dtype, int64_t n, const int64_t *indptr, const int32_t *indices,
                                        const void *values, int max_row, int levels, int steps, int step_size, double drop) {
  return create_host("rlh_fsfilter_create", ph, dtype, n, indptr, indices, values,
                     FsaiPlan::of_levels(max_row, levels).enriched_unless_0(steps, step_size).filtered_by(drop));
}

extern "C" int rlh_fsfilter_info(rlh_fsai_t h, double *drop, int64_t *removed) {
  RLH_REQUIRE(h && drop && removed, "rlh_fsfilter_info: null handle or output");
  *drop = h->drop;
  *removed = h->removed;
  return 0;
}

static FsaiPlan thresholded_plan(int max_row, int levels, int steps, int step_size, double drop, double prefilter) {
  return FsaiPlan::of_levels(max_row, levels).enriched_unless_0(steps, step_size).filtered_unless_0(drop).thresholded_by(prefilter);
}

extern "C" int rlh_fsthreshold_create_device(rlh_fsai_t *ph, int dtype, int64_t n, int index_bits, const void *d_indptr,
                                             const void *d_indices, const void *d_values, int max_row, int levels, int steps,
                                             int step_size, double drop, double prefilter) {
  return create_device("rlh_fsthreshold_create_device", ph, dtype, n, index_bits, d_indptr, d_indices, d_values,
                       thresholded_plan(max_row, levels, steps, step_size, drop, prefilter));
}

extern "C" int rlh_fsthreshold_create(rlh_fsai_t *ph, int dtype, int64_t n, const int64_t *indptr, const int32_t *indices,
                                      const void *values, int max_row, int levels, int steps, int step_size, double drop,
                                      double prefilter) {
  return create_host("rlh_fsthreshold_create", ph, dtype, n, indptr, indices, values,
                     thresholded_plan(max_row, levels, steps, step_size, drop, prefilter));
}

extern "C" int rlh_fsthreshold_info(rlh_fsai_t h, double *prefilter, int64_t *weak_entries) {
  RLH_REQUIRE(h && prefilter && weak_entries, "rlh_fsthreshold_info: null handle or output");
  *prefilter = h->prefilter;
  *weak_entries = h->weak;
  return 0;
}

extern "C" int rlh_fsvalues_update_device(rlh_fsai_t h, int index_bits, const void *d_indptr, const void *d_indices,
                                          const void *d_values) {
  constexpr const char *name = "rlh_fsvalues_update_device";
  if (int rc = require_ready()) return rc;
  RLH_REQUIRE(h != nullptr, "%s: null handle", name);
  RLH_REQUIRE(d_indptr, "%s: null indptr", name);
  RLH_REQUIRE(index_bits == 32 || index_bits == 64, "%s: index_bits must be 32 or 64, got %d", name, index_bits);
  return index_bits == 32 ? update_as<int32_t, int32_t>(h, name, d_indptr, d_indices, d_values)
                          : update_as<int64_t, int64_t>(h, name, d_indptr, d_indices, d_values);
}

extern "C" int rlh_fsvalues_update(rlh_fsai_t h, const int64_t *indptr, const int32_t *indices, const void *values) {
  constexpr const char *name = "rlh_fsvalues_update";
  if (int rc = require_ready()) return rc;
  RLH_REQUIRE(h != nullptr, "%s: null handle", name);
  RLH_REQUIRE(indptr, "%s: null indptr", name);
  UploadedCsr d;
  if (int rc = upload_csr(name, h->dtype, h->n, indptr, indices, values, &d)) return rc;
  return update_as<int64_t, int32_t>(h, name, d.ip, d.ix, d.va);     // (n == 0: a valid update that reads nothing)
}

extern "C" int rlh_fsvalues_info(rlh_fsai_t h, int64_t *updates, double *seconds) {
  RLH_REQUIRE(h, "rlh_fsvalues_info: null handle");
  if (updates) *updates = h->updates;
  if (seconds) *seconds = h->update_seconds;
  return 0;
}

extern "C" int rlh_fsai_adaptive(rlh_fsai_t h, int *steps, int *step_size) {
  RLH_REQUIRE(h && steps && step_size, "rlh_fsai_adaptive: null handle or output");
  *steps = h->steps;
  *step_size = h->step_size;
  return 0;
}

extern "C" int rlh_fsai_levels(rlh_fsai_t h, int *levels) {
  RLH_REQUIRE(h && levels, "rlh_fsai_levels: null handle or output");
  *levels = h->levels;
  return 0;
}

extern "C" int rlh_fsai_destroy(rlh_fsai_t h) {
  if (!h) return 0;
  if (ctx().ready) (void)hipStreamSynchronize(ctx().stream);
  if (h->spd) rlh_spd_destroy(h->spd);
  delete h;
  return 0;
}

extern "C" int rlh_fsai_info(rlh_fsai_t h, int64_t *n, int64_t *nnz, int64_t *longest_row, int64_t *truncated_rows,
                             int64_t *device_bytes, double *setup_seconds) {
  RLH_REQUIRE(h, "rlh_fsai_info: null handle");
  if (n) *n = h->n;
  if (nnz) *nnz = h->nnz;
  if (longest_row) *longest_row = h->longest;
  if (truncated_rows) *truncated_rows = h->truncated;
  if (device_bytes) {
    int64_t held = 0;
    if (h->spd)
      if (int rc = rlh_spd_info(h->spd, nullptr, nullptr, nullptr, &held)) return rc;
    *device_bytes = held + (int64_t)h->work.bytes();
  }
  if (setup_seconds) *setup_seconds = h->setup_seconds;
  return 0;
}

extern "C" int rlh_fsai_get(rlh_fsai_t h, int64_t *indptr, int32_t *indices, void *values) {
  if (int rc = require_ready()) return rc;
  RLH_REQUIRE(h, "rlh_fsai_get: null handle");
  RLH_REQUIRE(indptr && (h->nnz == 0 || (indices && values)), "rlh_fsai_get: null output");
  if (!h->spd) {
    indptr[0] = 0;
    return 0;
  }
  const SpdArrays g = spd_arrays(h->spd, 0);
  RLH_HIP(hipStreamSynchronize(ctx().stream));
  RLH_HIP(hipMemcpy(indptr, g.indptr, (size_t)(g.rows + 1) * 8, hipMemcpyDeviceToHost));
  if (g.nnz) {
    RLH_HIP(hipMemcpy(indices, g.idx, (size_t)g.nnz * 4, hipMemcpyDeviceToHost));
    RLH_HIP(hipMemcpy(values, g.val, (size_t)(g.nnz * dtype_size(h->dtype)), hipMemcpyDeviceToHost));
  }
  return 0;
}

extern "C" int rlh_fsai_apply(rlh_fsai_t h, int64_t m, const void *X, int64_t ldx, void *Y, int64_t ldy) {
  if (int rc = require_ready()) return rc;
  RLH_REQUIRE(h, "rlh_fsai_apply: null handle");
  RLH_REQUIRE(m >= 0, "rlh_fsai_apply: negative number of vectors");
  if (m == 0 || h->n == 0) return 0;
  RLH_REQUIRE(X && Y, "rlh_fsai_apply: null pointer");
  RLH_REQUIRE(ldx >= h->n && ldy >= h->n, "rlh_fsai_apply: Matrix and vectors dimensions incompatible");
  const int64_t ldw = (h->n + 15) & ~(int64_t)15;
  const int64_t need = ldw * m * dtype_size(h->dtype);
  if (int rc = h->work.reserve((size_t)need)) return rc;      // grows once per wider block, then reused without allocation
  if (int rc = rlh_spd_apply(h->spd, 0, m, X, ldx, h->work, ldw, nullptr, nullptr)) return rc;
  return rlh_spd_apply(h->spd, 1, m, h->work, ldw, Y, ldy, nullptr, nullptr);
}
