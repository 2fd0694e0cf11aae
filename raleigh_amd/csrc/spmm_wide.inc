// K13, interleaved windowed layout: Y = A X (or the fused Chebyshev step) for rows of ANY length and
// any element type.  Included by spmm_wide_{s,d,c,z}.hip, which define RLH_WIDE_DT / RLH_WIDE_FN.
//
// Reference semantics: mkl_?csrmm on triu(A) with the 'SUNF' / 'HUNF' descriptor
// (raleigh/algebra/sparse_mkl.py:42-48 -> mkl_wrap.py:246-276); the layout is built from the full
// CSR by spmm_wide_build.hip.
//
// One 256-thread workgroup per block of 256 rows, one row per thread.  Per PASS over NV vectors of
// the block of vectors:
//  * stage: the block's column windows of the NV vectors go to the LDS as an image [column][vector]
//    (row stride S = NV elements + 16 bytes, an odd number of 16-byte slots).  A lane loads 16-byte
//    pieces (EPL consecutive columns) of EPL vectors and writes the EPL x EPL transposed tile as EPL
//    ds_write_b128, so both sides move 16 bytes per lane;
//  * multiply: the row's entries stream through registers in chunks of 8 (four register sets: the
//    loads of three chunks are in flight during the arithmetic of one).  Per entry ONE address
//    (position * S) serves all NV vectors: NV / EPL ds_read_b128 at immediate offsets feed NV FMAs
//    into NV accumulators.  Nothing but the accumulators lives across chunks, so the register need
//    does not depend on the row length (the 1024-row kernel of spmm.hip keeps the whole row in
//    registers and spills beyond 8 entries);
//  * store: Y (or the fused three-term update of P) straight from the accumulators, 64 rows of one
//    vector per wave store.
// Passes re-read the entries (from L2 / Infinity Cache) and re-stage the windows; the launcher picks
// the largest NV whose image fits the LDS.
#include <type_traits>

#include "spmm.h"

namespace rlh {

template <typename T>
struct WideArgs {
  const WideMeta *meta;
  const int32_t *gsrc;
  const rlh_u32x4e *idx;         // [chunk][row]: 8 positions
  const rlh_u32x4e *vals;        // [chunk][piece][row]
  int64_t n_rows, n_cols;
  const int32_t *sched;
  int64_t sched_len;
  const T *X; int64_t ldx;
  int64_t n_own;
  const T *H; int64_t ldh;
  T *Y; int64_t ldy;
  int m;
  int vec;                       // 16-byte staging loads allowed (groups in range, pieces on one side of n_own)
  ChebArgs<T> cheb;
};

template <int NV, int ES> struct WideStride {
  static constexpr int raw = NV * ES + 16;
  static constexpr int value = ((raw / 16) & 1) ? raw : raw + 16;
};

// VS: waves 0-3 and (VS = 2) waves 4-7 work on the SAME 256 rows and different halves of the NV
// vectors of a pass -- twice the waves per SIMD to hide the LDS and memory latencies of the chunk
// loop, no reduction between them (both halves stream the row's entries, the second from L1 / L2).
// K: rows per thread.  K = 2 (real types, rows that share their column pattern pairwise: the unknowns of a finite-element
// node): a thread owns the row pair (2 r, 2 r + 1) of its block -- one position and two values per entry -- and reads the NV
// staged values of an entry ONCE for both rows; 128 row pairs per set of vectors, so the 512 threads are four sets of
// NV / 4 vectors each.
template <typename T, int NV, int VS, bool CHEB, int K = 1>
__global__ __launch_bounds__(256 / K * VS) void wide_spmm_kernel(const WideArgs<T> a) {
  constexpr int ES = (int)sizeof(T);
  constexpr int EPL = 16 / ES;                    // elements per 16-byte piece
  constexpr int VP = ES / 2;                      // 16-byte value pieces per chunk of 8 entries
  constexpr int S = WideStride<NV, ES>::value;    // bytes per staged column
  constexpr int LQ = NV < 8 ? NV : 8;             // 16-byte staging loads per lane and unit
  constexpr int GBN = NV / LQ;                    // units per trip over the column pieces
  constexpr int TPS = kWideRows / K;              // threads per set of vectors (= row groups of a block)
  constexpr int NT = TPS * VS;                    // threads
  constexpr int NVT = NV / VS;                    // vectors (accumulators) per thread
  constexpr int NVGT = NVT / EPL;                 // 16-byte pieces a thread reads per entry
  // entry chunks in flight: three for the real types; one for the complex ones, whose arithmetic per
  // entry is four times as long and whose register sets are twice as large
  constexpr bool DEEP = !(std::is_same<T, c32>::value || std::is_same<T, c64>::value) && K == 1;
  static_assert(NV % EPL == 0 && LQ % EPL == 0 && NV % LQ == 0 && NVT % EPL == 0,
                "vectors per pass come in whole 16-byte pieces");
  extern __shared__ __attribute__((aligned(16))) char lds[];
  char *img = lds + 2 * kWideHeader;              // two group lists (this block's, the next block's) in front
  const int tid = threadIdx.x;
  const int rtid = tid & (TPS - 1);               // row group of the block
  const int vsel = __builtin_amdgcn_readfirstlane(tid / TPS);         // which part of the vectors (wave-uniform)
  const T *Hs = a.H ? a.H - a.n_own : a.X;        // halo row of column c: Hs[c]
  const int last_col = (int)(a.n_cols - 1);
  const int m = a.m;

  struct Ent { rlh_u32x4e v[K * VP]; rlh_u32x4e p; };

  // The header of a block (schedule entry -> block record -> group list) is a chain of three
  // dependent loads: it is fetched one block ahead, the group list into the other half of the header.
  auto fetch_block = [&](int64_t pos_, int slot, WideMeta &mt_) -> int64_t {
    int64_t b_ = -1;
    while (pos_ < a.sched_len && (b_ = a.sched[pos_]) < 0) pos_ += gridDim.x;
    if (pos_ >= a.sched_len) return -1;
    mt_ = a.meta[b_];
    int *g_ = reinterpret_cast<int *>(lds + slot * kWideHeader);
    for (int g = tid; g < mt_.ng; g += NT) g_[g] = a.gsrc[mt_.goff + g];
    return pos_;
  };
  WideMeta mt, mt_next;
  int slot = 0;
  int64_t pos = fetch_block(blockIdx.x, slot, mt);
  __syncthreads();
  while (pos >= 0) {
    const int64_t b = a.sched[pos];
    const int *gcol = reinterpret_cast<const int *>(lds + slot * kWideHeader);
    const int nch = mt.nchunks;
    const int F = mt.ng * kWideGroup;             // staged columns
    const int64_t row = b * kWideRows + K * rtid;   // first row of this thread's group
    auto load_ent = [&](Ent &e, int q) {
      const int64_t ch = mt.eoff + q;
      // (no run-time switches around these loads: a branch per load makes the compiler wait for vmcnt(0)
      // where the paths join -- the phase-ablation switches of the round-2 experiments are gone for that reason)
#pragma unroll
      for (int k = 0; k < K * VP; ++k) e.v[k] = a.vals[(ch * K * VP + k) * TPS + rtid];
      e.p = a.idx[ch * TPS + rtid];
    };
    const int64_t pos_next = fetch_block(pos + gridDim.x, slot ^ 1, mt_next);
    for (int j0 = 0; j0 < m; j0 += NV) {
      const int nvp = (m - j0) < NV ? (m - j0) : NV;     // vectors of this pass
      // the first chunks of entries do not depend on the image: requested before the staging
      // (chunks past the row's last are the next block's or the padding behind the last block: loaded, never used)
      Ent e0, e1, e2, e3;
      load_ent(e0, 0);
      if constexpr (DEEP) {
        load_ent(e1, 1);
        load_ent(e2, 2);
      }
      // ---- stage the windows of vectors j0 .. j0 + nvp - 1
      if (a.vec) {
        // Units of LQ 16-byte loads per lane -- unit s = (trip t over the column pieces, block gb of
        // the vectors) -- in two register sets: the loads of unit s + 1 are issued before the LDS
        // writes of unit s wait for theirs, so the staging exposes one memory latency per block pass
        // instead of one per unit.  Lanes past the last piece repeat it (the same bytes to the same
        // address), vectors past the last repeat the last vector.
        const int CPV = F / EPL;
        const int trips = (CPV + NT - 1) / NT;
        const int units = trips * GBN;
        rlh_u32x4e ra[LQ], rb[LQ];
        auto unit_load = [&](rlh_u32x4e (&r)[LQ], int s_) {
          const int t = s_ / GBN, gb = s_ - t * GBN;
          int cp = tid + t * NT;
          cp = cp < CPV ? cp : CPV - 1;
          const int c = cp * EPL;
          const int col = gcol[c >> kWideGroupShift] + (c & (kWideGroup - 1));
          const bool own = col < a.n_own;
          const T *src = (own ? a.X : Hs) + col;
          const int64_t ld = own ? a.ldx : a.ldh;
#pragma unroll
          for (int u = 0; u < LQ; ++u) {
            int j = j0 + gb * LQ + u;
            j = j < m ? j : m - 1;
            r[u] = *reinterpret_cast<const rlh_u32x4u *>(src + (int64_t)j * ld);     // (T's alignment only)
          }
        };
        auto unit_write = [&](const rlh_u32x4e (&r)[LQ], int s_) {
          const int t = s_ / GBN, gb = s_ - t * GBN;
          int cp = tid + t * NT;
          cp = cp < CPV ? cp : CPV - 1;
          char *dst = img + (unsigned)(cp * EPL) * (unsigned)S + gb * (LQ / EPL) * 16;
#pragma unroll
          for (int u = 0; u < LQ / EPL; ++u)
#pragma unroll
            for (int k = 0; k < EPL; ++k) {       // column c + k: the EPL vectors of piece u of the block
              union { rlh_u32x4e q; unsigned w[4]; } out;
              constexpr int WPE = ES / 4;         // 32-bit words per element
#pragma unroll
              for (int e = 0; e < EPL; ++e)
#pragma unroll
                for (int d = 0; d < WPE; ++d) out.w[e * WPE + d] = r[u * EPL + e][k * WPE + d];
              *reinterpret_cast<rlh_u32x4e *>(dst + k * S + u * 16) = out.q;
            }
        };
        unit_load(ra, 0);
        for (int s_ = 0; s_ < units; s_ += 2) {
          unit_load(rb, s_ + 1 < units ? s_ + 1 : s_);
          unit_write(ra, s_);
          unit_load(ra, s_ + 2 < units ? s_ + 2 : s_);
          if (s_ + 1 < units) unit_write(rb, s_ + 1);
        }
      } else {
        // element-wise staging: groups may reach past the last column (clamped: such positions are
        // never referenced) and pieces may lie across the own / halo boundary
        for (int v = 0; v < nvp; ++v) {
          const int64_t j = j0 + v;
          for (int c = tid; c < F; c += NT) {
            int col = gcol[c >> kWideGroupShift] + (c & (kWideGroup - 1));
            col = col < last_col ? col : last_col;
            const T val = col < a.n_own ? a.X[col + j * a.ldx] : Hs[col + j * a.ldh];
            *reinterpret_cast<T *>(img + (unsigned)c * (unsigned)S + v * ES) = val;
          }
        }
      }
      __syncthreads();
      // ---- multiply: entries in chunks of 8, four register sets
      T acc[K][NVT];
#pragma unroll
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int v = 0; v < NVT; ++v) acc[k][v] = zero_of(T{});
      const char *imgv = img + vsel * (NVT * ES);        // this thread's part of every image row
      auto compute = [&](const Ent &e) {
        union { rlh_u32x4e u[K * VP]; T t[K * 8]; } vv;
#pragma unroll
        for (int k = 0; k < K * VP; ++k) vv.u[k] = e.v[k];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          const unsigned w = e.p[t >> 1];
          const unsigned px = (t & 1) ? (w >> 16) : (w & 0xffffu);
          const char *xa = imgv + px * (unsigned)S;
#pragma unroll
          for (int g = 0; g < NVGT; ++g) {
            const VecA<T, EPL> x = *reinterpret_cast<const VecA<T, EPL> *>(xa + g * 16);
#pragma unroll
            for (int k = 0; k < K; ++k)
#pragma unroll
              for (int e2 = 0; e2 < EPL; ++e2) fma_acc(acc[k][g * EPL + e2], vv.t[k * 8 + t], x.e[e2]);
          }
        }
      };
      if constexpr (!DEEP) {
        for (int q = 0; q < nch; q += 2) {
          load_ent(e1, q + 1);
          compute(e0);
          if (q + 1 >= nch) break;
          load_ent(e0, q + 2 < nch ? q + 2 : nch);
          compute(e1);
        }
      } else
      for (int q = 0; q < nch; q += 4) {
        const int qn = q + 3 < nch + 3 ? q + 3 : nch + 3;
        load_ent(e3, qn < nch + kWidePadChunks - 1 ? qn : nch + kWidePadChunks - 1);
        compute(e0);
        if (q + 1 >= nch) break;
        load_ent(e0, q + 4 < nch ? q + 4 : nch);
        compute(e1);
        if (q + 2 >= nch) break;
        load_ent(e1, q + 5 < nch ? q + 5 : nch);
        compute(e2);
        if (q + 3 >= nch) break;
        load_ent(e2, q + 6 < nch ? q + 6 : nch);
        compute(e3);
      }
      // ---- store
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int64_t rowk = row + k;
        if (rowk < a.n_rows) {
#pragma unroll
          for (int v = 0; v < NVT; ++v)
            if (vsel * NVT + v < nvp) {
              const int64_t j = j0 + vsel * NVT + v;
              if constexpr (!CHEB) {
                nt_store(a.Y + rowk + j * a.ldy, acc[k][v]);
              } else {
                T *pp = a.Y + rowk + j * a.ldy;
                const T res = sub_of(a.cheb.B[rowk + j * a.cheb.ldb], acc[k][v]);      // b - A y
                *pp = add_of(add_of(scale_of(a.cheb.cy, a.X[rowk + j * a.ldx]), scale_of(a.cheb.cp, *pp)),
                             scale_of(a.cheb.cb, res));
              }
            }
        }
      }
      __syncthreads();                            // the next pass / block overwrites the image
    }
    pos = pos_next;
    mt = mt_next;
    slot ^= 1;
  }
}

template <typename T, int NV, int VS, int K = 1>
static int wide_launch_nv(rlh_csr *h, int part, int64_t m, const T *X, int64_t ldx, int64_t n_own, const T *H,
                          int64_t ldh, T *Y, int64_t ldy, const ChebArgs<T> *cheb) {
  Context &c = ctx();
  constexpr int S = WideStride<NV, (int)sizeof(T)>::value;
  constexpr int EPL = 16 / (int)sizeof(T);
  const size_t lds = (size_t)2 * kWideHeader + (size_t)h->wide_gmax * kWideGroup * S;
  RLH_REQUIRE(lds <= (size_t)kWideLdsBytes, "rlh_spmm: the staged image of %d vectors does not fit the LDS", NV);
  // resident workgroups per CU: by registers (one wave per SIMD and workgroup; asked once per
  // instantiation) and by the image size of this operator
  static int fit_plain = 0, fit_cheb = 0;
  if (fit_plain == 0) {
    RLH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&wide_spmm_kernel<T, NV, VS, false, K>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, kWideLdsBytes));
    RLH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&wide_spmm_kernel<T, NV, VS, true, K>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, kWideLdsBytes));
    hipFuncAttributes fa;
    RLH_HIP(hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(&wide_spmm_kernel<T, NV, VS, false, K>)));
    fit_plain = 512 / ((fa.numRegs + 7) / 8 * 8 > 0 ? (fa.numRegs + 7) / 8 * 8 : 8) * K / VS;
    RLH_HIP(hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(&wide_spmm_kernel<T, NV, VS, true, K>)));
    fit_cheb = 512 / ((fa.numRegs + 7) / 8 * 8 > 0 ? (fa.numRegs + 7) / 8 * 8 : 8) * K / VS;
    if (fit_plain < 1) fit_plain = 1;
    if (fit_cheb < 1) fit_cheb = 1;
  }
  int per_cu = cheb ? fit_cheb : fit_plain;
  if (per_cu > (int)(kWideLdsBytes / lds)) per_cu = (int)(kWideLdsBytes / lds);
  if (per_cu > 4) per_cu = 4;
  const int cap = env_int("RLH_WIDE_WG_PER_CU", 0);            // tunable: 0 = as many as fit (at most 4)
  if (cap > 0 && per_cu > cap) per_cu = cap;
  const int32_t *sched = nullptr;
  int64_t sched_len = 0;
  int grid = 0;
  if (int rc = wide_sched(h, c.num_cu * per_cu, part, n_own, &sched, &sched_len, &grid)) return rc;
  if (sched_len == 0 || grid == 0) return 0;
  WideArgs<T> a;
  a.meta = h->wide_meta; a.gsrc = h->wide_gsrc;
  a.idx = (const rlh_u32x4e *)h->wide_idx; a.vals = (const rlh_u32x4e *)h->wide_vals;
  a.n_rows = h->n_rows; a.n_cols = h->n_cols; a.sched = sched; a.sched_len = sched_len;
  a.X = X; a.ldx = ldx; a.n_own = n_own; a.H = H; a.ldh = ldh; a.Y = Y; a.ldy = ldy; a.m = (int)m;
  a.vec = (env_int("RLH_SPMM_VEC", 1) != 0 && h->stage_inbounds &&
           (H == nullptr || n_own == h->n_cols || (h->stage_aligned && n_own % EPL == 0))) ? 1 : 0;
  a.cheb = cheb ? *cheb : ChebArgs<T>{};
  if (cheb)
    hipLaunchKernelGGL((wide_spmm_kernel<T, NV, VS, true, K>), dim3((unsigned)grid), dim3(256 / K * VS), lds, c.stream, a);
  else
    hipLaunchKernelGGL((wide_spmm_kernel<T, NV, VS, false, K>), dim3((unsigned)grid), dim3(256 / K * VS), lds, c.stream, a);
  note_launch(a.vec ? "wide nv=%d vs=%d k=%d vec cheb=%d" : "wide nv=%d vs=%d k=%d elem cheb=%d", NV, VS, K, cheb ? 1 : 0, grid, sched_len);
  RLH_HIP(hipGetLastError());
  return 0;
}

// Vectors per pass: the fewest passes whose image fits the LDS, then the smallest such NV (a smaller
// image lets more workgroups share a CU).  RLH_WIDE_NV forces a value (tunable).
static int wide_choose_nv(const rlh_csr *h, int64_t m, int es) {
  const bool real = h->dtype == RLH_S || h->dtype == RLH_D;
  const int cand[3] = {real ? 8 : 4, real ? 16 : 8, real ? 32 : 16};
  const int forced = env_int("RLH_WIDE_NV", 0);
  int best = 0;
  int64_t best_passes = 0;
  for (int i = 0; i < 3; ++i) {
    const int nv = cand[i];
    if ((int64_t)2 * kWideHeader + (int64_t)h->wide_gmax * kWideGroup * wide_stride(nv, es) > kWideLdsBytes) continue;
    if (forced == nv) return nv;
    const int64_t passes = (m + nv - 1) / nv;
    if (best == 0 || passes < best_passes) { best = nv; best_passes = passes; }
  }
  return best;
}

int RLH_WIDE_FN(rlh_csr *h, int part, int64_t m, const void *X_, int64_t ldx, int64_t n_own, const void *H_,
                int64_t ldh, void *Y_, int64_t ldy, const void *B_, int64_t ldb, double cy, double cp, double cb) {
  using T = typename DType<RLH_WIDE_DT>::T;
  constexpr bool real = !DType<RLH_WIDE_DT>::cplx;
  const T *X = (const T *)X_, *H = (const T *)H_;
  T *Y = (T *)Y_;
  ChebArgs<T> cargs{(const T *)B_, ldb, cy, cp, cb};
  const ChebArgs<T> *cheb = B_ ? &cargs : nullptr;
  const int nv = wide_choose_nv(h, m, (int)sizeof(T));
  RLH_REQUIRE(nv > 0, "rlh_spmm: no staged image of this operator fits the LDS");
  if constexpr (real) {
    // row pairs (h->wide_k == 2): four vectors per thread and row, i.e. NV / 4 sets of 128 threads
    if (h->wide_k == 2) {
      if (nv == 8) return wide_launch_nv<T, 8, 2, 2>(h, part, m, X, ldx, n_own, H, ldh, Y, ldy, cheb);
      return wide_launch_nv<T, 16, 4, 2>(h, part, m, X, ldx, n_own, H, ldh, Y, ldy, cheb);
    }
  }
  if (nv == (real ? 8 : 4)) return wide_launch_nv<T, (real ? 8 : 4), 1>(h, part, m, X, ldx, n_own, H, ldh, Y, ldy, cheb);
  // Two 256-thread workgroups per CU overlap one block's staging with the other's arithmetic (band of
  // 31 entries, m = 32: 1.9 ms against 2.6 ms for one 512-thread workgroup); where the image leaves room
  // for one workgroup only, 512 threads split the vectors of a pass (FE surrogate 0.054 -> 0.049 ms,
  // complex128 stencil 1.97 -> 1.54 ms).  RLH_WIDE_VS forces 1 or 2 (tunable).
  int vs = (int64_t)2 * kWideHeader + (int64_t)h->wide_gmax * kWideGroup * wide_stride(nv, (int)sizeof(T)) <= kWideLdsBytes / 2 ? 1 : 2;
  const int forced_vs = env_int("RLH_WIDE_VS", 0);
  if (forced_vs == 1 || forced_vs == 2) vs = forced_vs;
  if (nv == (real ? 16 : 8))
    return vs == 1 ? wide_launch_nv<T, (real ? 16 : 8), 1>(h, part, m, X, ldx, n_own, H, ldh, Y, ldy, cheb)
                   : wide_launch_nv<T, (real ? 16 : 8), 2>(h, part, m, X, ldx, n_own, H, ldh, Y, ldy, cheb);
  return vs == 1 ? wide_launch_nv<T, (real ? 32 : 16), 1>(h, part, m, X, ldx, n_own, H, ldh, Y, ldy, cheb)
                 : wide_launch_nv<T, (real ? 32 : 16), 2>(h, part, m, X, ldx, n_own, H, ldh, Y, ldy, cheb);
}

}  // namespace rlh
