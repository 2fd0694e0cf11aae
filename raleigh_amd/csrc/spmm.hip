// K13: sparse symmetric/Hermitian operator Y = A X on a block of vectors.
//
// The reference keeps triu(A) in 1-based CSR and calls mkl_?csrmm with the
// 'SUNF'/'HUNF' descriptor on the column-major n x m block
// (raleigh/algebra/sparse_mkl.py:16-48, raleigh/algebra/mkl_wrap.py:204-276).
// Here the caller hands over the FULL 0-based CSR (both triangles); at creation it is re-laid-out
// on the host (spmm_build.hip, spmm_wide_build.hip) in one of three device layouts (rlh_csr_layout reports which):
//  * 1024-row windowed ELL (this file, well_spmm_kernel): rows of at most 8 entries of a real
//    type with column locality -- stencils.  A block's column windows are staged through the LDS,
//    the row's entries stay in registers for all vectors.  Measured 54.6 % of the 8 TB/s peak on
//    the 7-point Laplacian at n = 10^7, m = 32 (1.21 x the algorithmic traffic).
//  * 256-row interleaved windowed layout (spmm_wide.inc): any row length, any type, with column
//    locality -- FE matrices, wide bands, all complex operators.  Entries stream through registers
//    in chunks of 8, the LDS image is [column][vector].
//  * sliced ELLPACK, slice height 64 (sell_spmm_kernel): no column locality.  One 8-byte gather of
//    X per stored entry and vector; limited by the rate at which a CU retires per-lane gathers
//    (profiles/r01_spmm_sweep2.txt), not by HBM: 34 % on the 7-point Laplacian.
#include "spmm.h"

namespace rlh {

// Work mapping (speed only; any placement gives the same result).  Workgroups b and b + 8
// share an XCD and its 4 MiB L2 under the observed round-robin placement.
//  * The slices are cut into chunks of `chunk` consecutive slices; chunk c belongs to XCD
//    c % 8 and the workgroups of an XCD walk its chunks in order, so rows that reference each
//    other are processed at about the same time on the same L2, and the eight XCDs advance
//    through adjacent chunks (one contiguous window of X for the Infinity Cache).
//  * The m vectors are cut into tiles of JT.  The waves of a workgroup take DIFFERENT tiles of
//    the SAME slice (tiles_per_block of them), which keeps the set of rows in flight per XCD --
//    and with it the L2 footprint of the gathered X lines -- small; the matrix entries of the
//    slice are fetched once per workgroup through L1.
// Fused Chebyshev step (CHEB), three-term form: with t = A y the row's results update
//   p = cy y + cp p + cb (b - t)
// in the same pass (device polynomial preconditioner: y = y_k, p = y_{k-1} on entry and y_{k+1} on
// return, b the right-hand side).  p is read and written by the row's own lane only, so it is
// updated in place; it must not alias y, which other rows are still gathering.  Per element the
// step reads y, p, b and writes p (the two-term form with a residual and a direction block read
// three and wrote three).
template <typename T, int JT, int TT, bool CHEB>
__global__ __launch_bounds__(256, (JT * TT >= 64 ? 1 : 2)) void sell_spmm_kernel(const int64_t *__restrict__ slice_ptr,
                                                        const int32_t *__restrict__ cols,
                                                        const T *__restrict__ vals, int64_t n_rows,
                                                        int64_t n_slices, const T *__restrict__ X, int64_t ldx,
                                                        int64_t n_own, const T *__restrict__ H, int64_t ldh,
                                                        T *__restrict__ Y, int64_t ldy, int m, int chunk,
                                                        int ntiles, int tiles_per_block, ChebArgs<T> cheb) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int xcd = blockIdx.x & 7;                                  // gridDim.x is a multiple of 8
  const int slices_per_block = 4 / tiles_per_block;
  const int64_t q0 = (int64_t)(blockIdx.x >> 3) * slices_per_block + wave / tiles_per_block;
  const int64_t q_stride = (int64_t)(gridDim.x >> 3) * slices_per_block;
  const int64_t nchunks = (n_slices + chunk - 1) / chunk;
  for (int tile = wave % tiles_per_block; tile < ntiles; tile += tiles_per_block) {
    const int j0 = tile * JT;
    const int jv = (m - j0) < JT ? (m - j0) : JT;
    const T *__restrict__ Xp = X + (int64_t)j0 * ldx;
    const T *__restrict__ Hp = H ? H + (int64_t)j0 * ldh : nullptr;
    T *__restrict__ Yp = Y + (int64_t)j0 * ldy;
    for (int64_t q = q0;; q += q_stride) {
      const int64_t c = (q / chunk) * 8 + xcd;
      if (c >= nchunks) break;
      const int64_t slice = c * chunk + q % chunk;
      if (slice >= n_slices) continue;
      const int64_t base = slice_ptr[slice];
      const int width = (int)((slice_ptr[slice + 1] - base) >> 6);
      const int64_t row = slice * 64 + lane;
      T acc[JT];
#pragma unroll
      for (int j = 0; j < JT; ++j) acc[j] = zero_of(T{});
      // entries in groups of TT: the group's column indices and values stay in registers while
      // the vectors of the tile are walked, so the TT gathers of one vector (neighbouring
      // entries of X for a stencil row) are issued back to back and share L1 lines
      for (int t0 = 0; t0 < width; t0 += TT) {
        const T *xc[TT];
        int64_t ldc[TT];
        T v[TT];
#pragma unroll
        for (int u = 0; u < TT; ++u) {
          const int t = (t0 + u) < width ? (t0 + u) : (width - 1);
          const int64_t e = base + (int64_t)t * 64 + lane;
          const int64_t cidx = __builtin_nontemporal_load(cols + e);   // streamed once per sweep
          v[u] = nt_load(vals + e);
          if (t0 + u >= width) v[u] = zero_of(T{});
          const bool own = cidx < n_own;               // off-shard rows live in the halo block
          xc[u] = own ? Xp + cidx : Hp + (cidx - n_own);
          ldc[u] = own ? ldx : ldh;
        }
        // all TT x JT gathers are issued before the first FMA needs one (memory-level
        // parallelism comes from the wave itself, not from occupancy)
        T xv[TT][JT];
#pragma unroll
        for (int u = 0; u < TT; ++u)
#pragma unroll
          for (int j = 0; j < JT; ++j) {
            const int jj = j < jv ? j : 0;             // clamp: columns >= m re-read column j0
            xv[u][j] = xc[u][(int64_t)jj * ldc[u]];
          }
#pragma unroll
        for (int u = 0; u < TT; ++u)
#pragma unroll
          for (int j = 0; j < JT; ++j) fma_acc(acc[j], v[u], xv[u][j]);
      }
      if (row < n_rows) {
        if constexpr (!CHEB) {
#pragma unroll
          for (int j = 0; j < JT; ++j)
            if (j < jv) nt_store(Yp + row + (int64_t)j * ldy, acc[j]);
        } else {
#pragma unroll
          for (int j = 0; j < JT; ++j)
            if (j < jv) {
              const int64_t jc = j0 + j;
              T *pp = Yp + row + (int64_t)j * ldy;
              const T res = sub_of(cheb.B[row + jc * cheb.ldb], acc[j]);      // b - A y
              *pp = add_of(add_of(scale_of(cheb.cy, Xp[row + (int64_t)j * ldx]), scale_of(cheb.cp, *pp)),
                           scale_of(cheb.cb, res));
            }
        }
      }
    }
  }
}

LaunchNote &launch_note() {
  static LaunchNote note;
  return note;
}

template <typename T, int JT, int TT>
static int launch_spmm_t(const rlh_csr *h, int64_t m, const T *X, int64_t ldx, int64_t n_own, const T *H, int64_t ldh,
                       T *Y, int64_t ldy, const ChebArgs<T> *cheb) {
  Context &c = ctx();
  static int fit = 0;                                        // resident workgroups per CU of this instantiation
  if (fit == 0) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, sell_spmm_kernel<T, JT, TT, false>, 256, 0) != hipSuccess || nb < 1)
      nb = 1;
    fit = nb > 8 ? 8 : nb;
  }
  int per_cu = fit;
  const int cap = env_int("RLH_SPMM_WG_PER_CU", 2);         // 0: as many as fit (tunable; 2 measured best)
  if (cap > 0 && per_cu > cap) per_cu = cap;
  const int chunk = env_int("RLH_SPMM_CHUNK", 64);      // slices per row chunk (tunable)
  const int tpb_cap = env_int("RLH_SPMM_TPB", 1);       // waves of a workgroup on one slice (tunable)
  const int ntiles = (int)((m + JT - 1) / JT);
  int tiles_per_block = ntiles >= 4 ? 4 : (ntiles >= 2 ? 2 : 1);
  if (tiles_per_block > tpb_cap) tiles_per_block = tpb_cap >= 2 ? 2 : 1;
  const int slices_per_block = 4 / tiles_per_block;
  int64_t nb = (int64_t)c.num_cu * per_cu;
  const int64_t need = ((h->n_slices + slices_per_block - 1) / slices_per_block + 7) / 8 * 8;
  if (nb > need) nb = need;
  nb = (nb + 7) / 8 * 8;
  if (cheb) {
    if constexpr (JT < 32) {       // (32 accumulators + the fused epilogue spill: the fused step takes tiles of 16)
      hipLaunchKernelGGL((sell_spmm_kernel<T, JT, TT, true>), dim3((unsigned)nb), dim3(256), 0, c.stream, h->slice_ptr,
                         h->cols, (const T *)h->vals, h->n_rows, h->n_slices, X, ldx, n_own, H, ldh, Y, ldy, (int)m,
                         chunk < 1 ? 1 : chunk, ntiles, tiles_per_block, *cheb);
      note_launch("sell jt=%d tt=%d tpb=%d cheb=1", JT, TT, tiles_per_block, 0, nb, h->n_slices);
    }
  } else {
    hipLaunchKernelGGL((sell_spmm_kernel<T, JT, TT, false>), dim3((unsigned)nb), dim3(256), 0, c.stream, h->slice_ptr,
                       h->cols, (const T *)h->vals, h->n_rows, h->n_slices, X, ldx, n_own, H, ldh, Y, ldy, (int)m,
                       chunk < 1 ? 1 : chunk, ntiles, tiles_per_block, ChebArgs<T>{});
    note_launch("sell jt=%d tt=%d tpb=%d cheb=0", JT, TT, tiles_per_block, 0, nb, h->n_slices);
  }
  RLH_HIP(hipGetLastError());
  return 0;
}

template <typename T, int JT>
static int launch_spmm(const rlh_csr *h, int64_t m, const T *X, int64_t ldx, int64_t n_own, const T *H, int64_t ldh,
                       T *Y, int64_t ldy, const ChebArgs<T> *cheb) {
  const int tt = env_int("RLH_SPMM_TT", 1);             // entries per register group (tunable)
  if (tt >= 8) return launch_spmm_t<T, JT, 8>(h, m, X, ldx, n_own, H, ldh, Y, ldy, cheb);
  if (tt >= 4) return launch_spmm_t<T, JT, 4>(h, m, X, ldx, n_own, H, ldh, Y, ldy, cheb);
  return launch_spmm_t<T, JT, 1>(h, m, X, ldx, n_own, H, ldh, Y, ldy, cheb);
}


// ------------------------------------------------------------------ Windowed ELL
// The sliced kernel above is limited by the rate at which a CU's vector-memory path retires
// per-lane gathers (one 8-byte gather per stored entry and vector: measured ~19 cycles per
// 512-byte wave gather whatever the locality, profiles/r01_spmm_sweep2.txt), not by HBM.  For
// matrices with column locality (banded, stencil, FE after a bandwidth-reducing ordering) the
// gathers of a block of rows fall into a few contiguous column windows, so this layout moves
// them to the LDS, whose read rate is 8x higher:
//  * rows are cut into blocks of 1024 (one row per thread of a 1024-thread workgroup, 16 waves);
//  * per block the referenced columns are merged into windows (gaps <= 32 columns are bridged),
//    each padded to a multiple of 64 columns: a "staging group" is 64 consecutive columns that
//    one wave copies from the block of vectors into the LDS with one coalesced load;
//  * an entry stores its value and the 16-bit position of its column in the staged image;
//    the entries of the thread's row stay in registers for all the vectors of the block;
//  * per step the workgroup computes as many vectors as one LDS buffer holds while the loads that
//    fill the other buffer with the next ones are in flight (register-staged double buffer,
//    one barrier per step).
// Each element of X is then loaded once per window it lies in (3.4x for the 7-point stencil on
// 215^3: centre + y neighbours in one window, the two z planes in one each) instead of once per
// entry (7x), and the seven reads per row come out of the LDS.
// (WellCfg and the entry storage of a block, well_val_index / well_idx_index: spmm.h, shared with the host builder)
// the row's WMAX values and positions (the host pads every row to WMAX slots: value 0 at the position of
// the row's own first entry, so a padding slot of a row with at least one entry never touches a column the row does
// not reference; an empty row's slots take position 0 of the image)
template <typename T, int WMAX>
__device__ __forceinline__ void well_load_entries(const T *__restrict__ vals, const uint16_t *__restrict__ idx,
                                                  int64_t eoff, int tid, int width, T (&v)[WMAX], unsigned (&pos)[WMAX]) {
  constexpr int VPG = 16 / (int)sizeof(T) > 0 ? 16 / (int)sizeof(T) : 1;
  static_assert(WMAX % 8 == 0 && WMAX % VPG == 0, "entry slots come in 16-byte pieces");
#pragma unroll
  for (int g = 0; g < WMAX / VPG; ++g) {
    union { rlh_u32x4e u; T t[VPG]; } piece;
    piece.u = __builtin_nontemporal_load(reinterpret_cast<const rlh_u32x4e *>(vals + well_val_index<T>(eoff, g * VPG, tid)));
#pragma unroll
    for (int k = 0; k < VPG; ++k) v[g * VPG + k] = piece.t[k];
  }
#pragma unroll
  for (int g = 0; g < WMAX / 8; ++g) {
    union { rlh_u32x4e u; unsigned short h[8]; } piece;
    piece.u = __builtin_nontemporal_load(reinterpret_cast<const rlh_u32x4e *>(idx + well_idx_index(eoff, g * 8, tid)));
#pragma unroll
    for (int k = 0; k < 8; ++k) pos[g * 8 + k] = (unsigned)piece.h[k];
  }
}

// The same with the values out of the stacks' dictionary: the row's pattern index (4 bytes) and the 8 values of that
// pattern (a few dozen 16-byte lines that stay in the L1 / L2 for the whole launch) instead of 8 values per row.
// Positions likewise where the handle has position patterns (dtab): within a member of a stack the staged position of a
// stencil row's k-th entry is the row's index in the block plus a constant, so the row stores which of the member's
// few tuples of constants it uses (upper half of its pattern word) instead of 8 positions.
template <typename T, int WMAX>
__device__ __forceinline__ void well_load_entries_pat(const T *__restrict__ table, const int32_t *__restrict__ pat,
                                                      const uint16_t *__restrict__ dtab, const uint16_t *__restrict__ idx,
                                                      int64_t eoff, int64_t pblock, int tid, T (&v)[WMAX],
                                                      unsigned (&pos)[WMAX]) {
  constexpr int VPG = 16 / (int)sizeof(T) > 0 ? 16 / (int)sizeof(T) : 1;
  static_assert(WMAX == 8, "one 16-byte piece of positions per row");
  const unsigned word = (unsigned)pat[pblock * kWellRows + tid];
  const int32_t pid = (int32_t)(word & 0xffffu);
#pragma unroll
  for (int g = 0; g < WMAX / VPG; ++g) {
    union { rlh_u32x4e u; T t[VPG]; } piece;
    piece.u = *reinterpret_cast<const rlh_u32x4e *>(table + (int64_t)pid * WMAX + g * VPG);
#pragma unroll
    for (int k = 0; k < VPG; ++k) v[g * VPG + k] = piece.t[k];
  }
  union { rlh_u32x4e u; unsigned short h[8]; } piece;
  if (dtab) {
    piece.u = *reinterpret_cast<const rlh_u32x4e *>(dtab + (pblock * kStkMaxDeltas + (int64_t)(word >> 16)) * 8);
#pragma unroll
    for (int k = 0; k < 8; ++k) pos[k] = ((unsigned)piece.h[k] + (unsigned)tid) & 0xffffu;
  } else {
    piece.u = __builtin_nontemporal_load(reinterpret_cast<const rlh_u32x4e *>(idx + well_idx_index(eoff, 0, tid)));
#pragma unroll
    for (int k = 0; k < 8; ++k) pos[k] = (unsigned)piece.h[k];
  }
}

// Exchange within a quad of lanes (DPP quad_perm): CTRL 0xB1 = lane ^ 1, 0x4E = lane ^ 2.
template <typename T, int CTRL>
__device__ __forceinline__ T dpp_quad(T v) {
  constexpr int W = (int)(sizeof(T) / 4);
  union { T t; int w[W]; } a, b;
  a.t = v;
#pragma unroll
  for (int k = 0; k < W; ++k) b.w[k] = __builtin_amdgcn_update_dpp(0, a.w[k], CTRL, 0xf, 0xf, true);
  return b.t;
}

template <typename T, int WMAX, int EPL, bool CHEB>
__global__ __launch_bounds__(1024) void well_spmm_kernel(const WellMeta *__restrict__ meta,
                                                         const int32_t *__restrict__ gsrc,
                                                         const uint16_t *__restrict__ idx,
                                                         const T *__restrict__ vals, int64_t n_rows, int64_t n_cols,
                                                         const int32_t *__restrict__ sched, int64_t sched_len,
                                                         const T *__restrict__ X, int64_t ldx,
                                                         int64_t n_own, const T *__restrict__ H, int64_t ldh,
                                                         T *__restrict__ Y, int64_t ldy, int m, int cps_cap,
                                                         ChebArgs<T> cheb) {
  constexpr int SMAX = WellCfg<T>::SMAX;      // staging loads per thread and step
  constexpr int BUF = kWellRows * SMAX;       // elements per LDS buffer
  __shared__ T lds[2 * BUF];
  char *ldsb = reinterpret_cast<char *>(lds);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const unsigned lane8 = (unsigned)lane * (unsigned)sizeof(T);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const T *Hs = H ? H - n_own : X;            // halo row of column c: Hs[c]
  const int last_col = (int)(n_cols - 1);
  // The step bodies below are straight-line on purpose: every load and LDS write of a step is
  // issued unconditionally (surplus staging slots repeat the step's last group, entry slots past
  // the block's width are zeroed), so the compiler keeps counted vmcnt waits and the loads of two
  // steps really are in flight together; with per-load predicates it waited for vmcnt(0) before
  // every load.
  for (int64_t pos = blockIdx.x; pos < sched_len; pos += gridDim.x) {
    const int64_t b = sched[pos];
    if (b < 0) continue;
    const WellMeta mt = meta[b];
    const int width = mt.width_ng & 255;
    const int ng = mt.width_ng >> 8;          // >= 1
    const int F = ng * 64;                    // staged elements per vector
    // vectors per step: as many as the LDS buffer holds, evened out over the steps
    int cps = (16 * SMAX) / ng;
    if (cps > cps_cap) cps = cps_cap;
    if (cps > m) cps = m;
    const int nsteps = (m + cps - 1) / cps;
    cps = (m + nsteps - 1) / nsteps;
    const int G = ng * cps;                   // staging groups per step
    const int64_t row = b * kWellRows + tid;
    const bool whole_block = (b + 1) * kWellRows <= n_rows;     // workgroup-uniform: no row past the end
    // the row's entries: registers for the whole block of vectors (slots past the block's width
    // read the next block's entries -- the arrays are padded -- and are zeroed)
    // Positions: one register per entry holding the byte offset, or (PACK: 32 slots of an 8-byte
    // type, where 32 more registers would spill) two 16-bit positions per register, unpacked at use.
    constexpr bool PACK = WMAX * sizeof(T) >= 256;
    T v[WMAX];
    unsigned ixb[PACK ? WMAX / 2 : WMAX];
    {
      unsigned px[WMAX];
      well_load_entries<T, WMAX>(vals, idx, mt.eoff, tid, width, v, px);
#pragma unroll
      for (int t = 0; t < WMAX; ++t) {
        if constexpr (!PACK) ixb[t] = px[t] * (unsigned)sizeof(T);
        else if (t & 1) ixb[t / 2] |= px[t] << 16;
        else ixb[t / 2] = px[t];
      }
    }
    auto entry_offset = [&](int t) -> unsigned {       // byte offset of entry t's column in a staged vector
      if constexpr (!PACK) return ixb[t];
      else return ((ixb[t / 2] >> (16 * (t & 1))) & 0xffffu) * (unsigned)sizeof(T);
    };
    // this thread's share of a step's staging: one load moves EPL elements per lane, i.e. EPL
    // consecutive 64-column groups per wave; slot i of the wave covers groups q .. q + EPL - 1,
    // q = EPL (wave + 16 i), of the step's G (vector cc = q / ng of the step, groups q % ng .. of
    // the block: ng is a multiple of 8, so a slot never straddles two vectors)
    constexpr int SLOTS = SMAX / EPL;
    constexpr int LPG = 64 / EPL;             // lanes per group
    int sbase[SLOTS];                         // byte offset of the slot's groups in an LDS buffer (wave-uniform)
    int scc[SLOTS];                           // vector within the step (wave-uniform)
    int scol[SLOTS];                          // first column this lane reads
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
      int q = (wave + 16 * i) * EPL;
      if (q > G - EPL) q = G - EPL;           // surplus slots repeat the last groups
      const int cc = q / ng, g = q - cc * ng;
      scc[i] = __builtin_amdgcn_readfirstlane(cc);
      sbase[i] = __builtin_amdgcn_readfirstlane((cc * F + g * 64) * (int)sizeof(T));
      if constexpr (EPL == 1)
        scol[i] = __builtin_amdgcn_readfirstlane(gsrc[mt.goff + g]);
      else
        scol[i] = gsrc[mt.goff + g + lane / LPG] + (lane % LPG) * EPL;
    }
    VecU<T, EPL> stA[SLOTS];
    auto stage_load = [&](int s, VecU<T, EPL> (&st)[SLOTS]) {
#pragma unroll
      for (int i = 0; i < SLOTS; ++i) {
        int j = s * cps + scc[i];
        if (j > m - 1) j = m - 1;             // a short last step re-reads the last vector
        int c;
        if constexpr (EPL == 1) {
          c = scol[i] + lane;
          if (c > last_col) c = last_col;     // group padding past the last column re-reads it
        } else {
          c = scol[i];                        // the host checked: groups in range, pieces on one side of n_own
        }
        const T *src = c < n_own ? X + (int64_t)j * ldx : Hs + (int64_t)j * ldh;
        st[i] = *reinterpret_cast<const VecU<T, EPL> *>(src + c);
      }
    };
    // LDS addresses are formed at the point of use from an opaque scalar (the byte offset of the
    // buffer, or of the vector in it) plus a per-thread register: left to itself the compiler
    // hoists one address register per (buffer, vector, entry) out of the step loop and spills.
    auto stage_write = [&](int s, const VecU<T, EPL> (&st)[SLOTS]) {
      unsigned boff = (unsigned)(s & 1) * (unsigned)(BUF * sizeof(T));
      asm volatile("" : "+s"(boff));
#pragma unroll
      for (int i = 0; i < SLOTS; ++i) {
        VecA<T, EPL> val;
#pragma unroll
        for (int k = 0; k < EPL; ++k) val.e[k] = st[i].e[k];
        *reinterpret_cast<VecA<T, EPL> *>(ldsb + (lane8 * EPL + (boff + (unsigned)sbase[i]))) = val;
      }
    };
    auto row_product = [&](unsigned bo) -> T {          // (A y)[row] for the vector staged at byte offset bo
      asm volatile("" : "+s"(bo));
      T acc = zero_of(T{});
#pragma unroll
      for (int t = 0; t < WMAX; ++t) fma_acc(acc, v[t], *reinterpret_cast<const T *>(ldsb + (entry_offset(t) + bo)));
      return acc;
    };
    auto compute = [&](int s) {
      unsigned boff = (unsigned)(s & 1) * (unsigned)(BUF * sizeof(T));
      int j = s * cps;
      const int jend = (j + cps < m) ? j + cps : m;
      if constexpr (CHEB && sizeof(T) <= 8) {
        // Two vectors at a time with the two results of a lane pair exchanged (DPP), so that a lane
        // holds rows rb, rb + 1 of ONE vector: y, p, b are then read and p written as 2-element
        // pieces (8 bytes for float, 16 for double) -- half the vector-memory instructions of the
        // element-wise epilogue, which is what bounds the fused step at small block sizes.
        if (whole_block) {
          const int q = lane & 1;
          const int64_t rb = row - q;
          struct alignas(sizeof(T)) V2 { T e[2]; };
          for (; j + 1 < jend; j += 2) {
            const T a0 = row_product(boff), a1 = row_product(boff + (unsigned)F * (unsigned)sizeof(T));
            boff += 2u * (unsigned)F * (unsigned)sizeof(T);
            const T got = dpp_quad<T, 0xB1>(q ? a0 : a1);           // the neighbour's result for MY vector
            const T t0 = q ? got : a0, t1 = q ? a1 : got;           // (A y) at rows rb, rb + 1 of vector j + q
            const int64_t jq = j + q;
            V2 *pp = reinterpret_cast<V2 *>(Y + rb + jq * ldy);
            const V2 pv = *pp;
            const V2 bv = *reinterpret_cast<const V2 *>(cheb.B + rb + jq * cheb.ldb);
            const V2 yv = *reinterpret_cast<const V2 *>(X + rb + jq * ldx);
            V2 out;
            out.e[0] = add_of(add_of(scale_of(cheb.cy, yv.e[0]), scale_of(cheb.cp, pv.e[0])),
                              scale_of(cheb.cb, sub_of(bv.e[0], t0)));
            out.e[1] = add_of(add_of(scale_of(cheb.cy, yv.e[1]), scale_of(cheb.cp, pv.e[1])),
                              scale_of(cheb.cb, sub_of(bv.e[1], t1)));
            *pp = out;
          }
        }
      }
      for (; j < jend; ++j) {
        asm volatile("" : "+s"(boff));
        T acc = zero_of(T{});
#pragma unroll
        for (int t = 0; t < WMAX; ++t) fma_acc(acc, v[t], *reinterpret_cast<const T *>(ldsb + (entry_offset(t) + boff)));
        if (row < n_rows) {
          if constexpr (!CHEB) {
            nt_store(Y + row + (int64_t)j * ldy, acc);
          } else {
            T *pp = Y + row + (int64_t)j * ldy;
            const T res = sub_of(cheb.B[row + (int64_t)j * cheb.ldb], acc);     // b - A y
            *pp = add_of(add_of(scale_of(cheb.cy, X[row + (int64_t)j * ldx]), scale_of(cheb.cp, *pp)),
                         scale_of(cheb.cb, res));
          }
        }
        boff += (unsigned)F * (unsigned)sizeof(T);
      }
    };
    if constexpr (PACK || EPL == 1 || (CHEB && sizeof(T) == 8)) {     // (the fp64 fused step spilled 52 bytes with two sets)
      // one register set only (the element-wise staging of unaligned layouts needs SMAX slots per
      // set): the loads of step s + 1 are in flight during the arithmetic of step s
      stage_load(0, stA);
      stage_write(0, stA);
      __syncthreads();
      for (int s = 0; s + 1 < nsteps; ++s) {
        stage_load(s + 1, stA);
        compute(s);
        stage_write(s + 1, stA);
        __syncthreads();
      }
      compute(nsteps - 1);
    } else {
      // Two register sets: the loads of step s + 2 are issued at the start of step s and written
      // to the LDS at the end of step s + 1, so they have two steps (and two barriers, which plain
      // loads survive) to arrive.
      VecU<T, EPL> stB[SLOTS];
      stage_load(0, stA);
      stage_load(nsteps > 1 ? 1 : 0, stB);
      stage_write(0, stA);
      __syncthreads();
      int s = 0;
      for (; s + 3 < nsteps; s += 2) {          // both prefetch targets exist
        stage_load(s + 2, stA);                 // B holds step s + 1
        compute(s);
        stage_write(s + 1, stB);
        __syncthreads();
        stage_load(s + 3, stB);                 // A holds step s + 2
        compute(s + 1);
        stage_write(s + 2, stA);
        __syncthreads();
      }
      const int left = nsteps - s;              // 1, 2 or 3 steps, nothing beyond them to prefetch
      if (left == 3) {
        stage_load(s + 2, stA);
        compute(s);
        stage_write(s + 1, stB);
        __syncthreads();
        compute(s + 1);
        stage_write(s + 2, stA);
        __syncthreads();
        compute(s + 2);
      } else if (left == 2) {
        compute(s);
        stage_write(s + 1, stB);
        __syncthreads();
        compute(s + 1);
      } else {
        compute(s);
      }
    }
    __syncthreads();                          // the next block's first stage overwrites the buffers
  }
}

// ------------------------------------------------------------------ Stacked blocks
// What bounds the windowed kernel on a 3-D stencil is the volume it stages, not the arithmetic: a 1024-row block of the
// 7-point Laplacian on 215^3 stages 3.4 elements per row and vector (its own rows + the y neighbours, and the two z planes
// in a window each), the 5-point one on 3152^2 3.25, a band matrix 1.06 -- and the three run at 1.36, 1.34 and 1.04 ms
// (profiles/r01_spmm_windowed.txt).  The z-plane windows of block b are the OWN rows of the blocks one grid plane further
// on: a workgroup that takes R such blocks together (thread l = row l of each of them) stages the shared windows once,
// (2 + R * 1.42) / R elements per row instead of 3.42.  The host picks the stacks on the window-overlap graph (greedy
// matching: the unstacked block that overlaps a block's windows most), so nothing here knows about grids; blocks without a
// partner run as stacks of one.  Same entry storage, staging plan and step pipeline as above (16-byte staging only: the
// caller checks that every group is in range); the two staging buffers are the CU's whole LDS (kStkR, kStkBufBytes: spmm.h).
template <typename T, int R>
__global__ __launch_bounds__(1024) void well_stack_kernel(const WellMeta *__restrict__ meta,
                                                          const int32_t *__restrict__ member,
                                                          const int32_t *__restrict__ gsrc,
                                                          const uint16_t *__restrict__ idx,
                                                          const T *__restrict__ vals, int64_t n_rows,
                                                          const int32_t *__restrict__ sched, int64_t sched_len,
                                                          const T *__restrict__ X, int64_t ldx,
                                                          T *__restrict__ Y, int64_t ldy, int m, int cps_cap) {
  constexpr int WMAX = 8;
  constexpr int EPL = 16 / (int)sizeof(T);         // elements per 16-byte piece = 64-column groups per wave load
  constexpr int GPS = 16 * EPL;                    // groups one staging slot of the 16 waves covers
  constexpr int BUFG = kStkBufBytes / (64 * (int)sizeof(T));     // groups per buffer
  constexpr int SLOTS = BUFG / GPS;
  static_assert(SLOTS * GPS == BUFG, "a buffer is a whole number of slots");
  extern __shared__ __align__(16) char ldsb[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const unsigned lane16 = (unsigned)lane * 16u;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int64_t pos = blockIdx.x; pos < sched_len; pos += gridDim.x) {
    const int64_t sb = sched[pos];
    if (sb < 0) continue;
    const WellMeta mt = meta[sb];
    const int ng = mt.width_ng >> 8;               // >= 8, a multiple of 8
    const int F = ng * 64;
    int cps = BUFG / ng;
    if (cps > cps_cap) cps = cps_cap;
    if (cps > m) cps = m;
    const int nsteps = (m + cps - 1) / cps;
    cps = (m + nsteps - 1) / nsteps;
    const int G = ng * cps;
    // entries: values, and byte offsets in a staged vector -- for 8-byte types two 16-bit positions per register,
    // unpacked at use (16 more registers spill)
    constexpr bool PACK = sizeof(T) >= 8;
    int64_t row[R];
    T v[R][WMAX];
    unsigned ixb[R][PACK ? WMAX / 2 : WMAX];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int2 mr = reinterpret_cast<const int2 *>(member)[sb * R + r];       // first row, rows (0: no such member)
      row[r] = tid < mr.y ? (int64_t)mr.x + tid : n_rows;             // (no such row: its slots hold zeros)
      unsigned px[WMAX];
      well_load_entries<T, WMAX>(vals, idx, mt.eoff + 8 * r, tid, WMAX, v[r], px);
#pragma unroll
      for (int t = 0; t < WMAX; ++t) {
        if constexpr (!PACK) ixb[r][t] = px[t] * (unsigned)sizeof(T);
        else if (t & 1) ixb[r][t / 2] |= px[t] << 16;
        else ixb[r][t / 2] = px[t];
      }
    }
    int sbase[SLOTS], scc[SLOTS], scol[SLOTS];
    constexpr int LPG = 64 / EPL;
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
      int q = (wave + 16 * i) * EPL;
      if (q > G - EPL) q = G - EPL;                // surplus slots repeat the last groups
      const int cc = q / ng, g = q - cc * ng;
      scc[i] = __builtin_amdgcn_readfirstlane(cc);
      sbase[i] = __builtin_amdgcn_readfirstlane((cc * F + g * 64) * (int)sizeof(T));
      scol[i] = gsrc[mt.goff + g + lane / LPG] + (lane % LPG) * EPL;
    }
    auto stage_load = [&](int s, VecU<T, EPL> (&st)[SLOTS]) {
#pragma unroll
      for (int i = 0; i < SLOTS; ++i) {
        int j = s * cps + scc[i];
        if (j > m - 1) j = m - 1;
        st[i] = *reinterpret_cast<const VecU<T, EPL> *>(X + (int64_t)j * ldx + scol[i]);
      }
    };
    auto stage_write = [&](int s, const VecU<T, EPL> (&st)[SLOTS]) {
      unsigned boff = (unsigned)(s & 1) * (unsigned)kStkBufBytes;
      asm volatile("" : "+s"(boff));
#pragma unroll
      for (int i = 0; i < SLOTS; ++i) {
        VecA<T, EPL> val;
#pragma unroll
        for (int k = 0; k < EPL; ++k) val.e[k] = st[i].e[k];
        *reinterpret_cast<VecA<T, EPL> *>(ldsb + (lane16 + (boff + (unsigned)sbase[i]))) = val;
      }
    };
    auto compute = [&](int s) {
      unsigned boff = (unsigned)(s & 1) * (unsigned)kStkBufBytes;
      int j = s * cps;
      const int jend = (j + cps < m) ? j + cps : m;
      for (; j < jend; ++j) {
        asm volatile("" : "+s"(boff));
#pragma unroll
        for (int r = 0; r < R; ++r) {
          T acc = zero_of(T{});
#pragma unroll
          for (int t = 0; t < WMAX; ++t) {
            if constexpr (!PACK) {
              fma_acc(acc, v[r][t], *reinterpret_cast<const T *>(ldsb + (ixb[r][t] + boff)));
            } else if ((t & 1) == 0) {
              unsigned w = ixb[r][t / 2];
              asm volatile("" : "+v"(w));          // (unpacked per vector: hoisted out of the loop the offsets take 16 registers again)
              fma_acc(acc, v[r][t], *reinterpret_cast<const T *>(ldsb + ((w & 0xffffu) * (unsigned)sizeof(T) + boff)));
              fma_acc(acc, v[r][t + 1], *reinterpret_cast<const T *>(ldsb + ((w >> 16) * (unsigned)sizeof(T) + boff)));
            }
          }
          if (row[r] < n_rows) nt_store(Y + row[r] + (int64_t)j * ldy, acc);
        }
        boff += (unsigned)F * (unsigned)sizeof(T);
      }
    };
    if constexpr (sizeof(T) >= 8) {
      // one register set (two spill 36 bytes in fp64): the loads of step s + 1 are in flight during the arithmetic of step s
      VecU<T, EPL> stA[SLOTS];
      stage_load(0, stA);
      stage_write(0, stA);
      __syncthreads();
      for (int s = 0; s + 1 < nsteps; ++s) {
        stage_load(s + 1, stA);
        compute(s);
        stage_write(s + 1, stA);
        __syncthreads();
      }
      compute(nsteps - 1);
      __syncthreads();
      continue;
    }
    VecU<T, EPL> stA[SLOTS], stB[SLOTS];
    stage_load(0, stA);
    stage_load(nsteps > 1 ? 1 : 0, stB);
    stage_write(0, stA);
    __syncthreads();
    int s = 0;
    for (; s + 3 < nsteps; s += 2) {
      stage_load(s + 2, stA);
      compute(s);
      stage_write(s + 1, stB);
      __syncthreads();
      stage_load(s + 3, stB);
      compute(s + 1);
      stage_write(s + 2, stA);
      __syncthreads();
    }
    const int left = nsteps - s;
    if (left == 3) {
      stage_load(s + 2, stA);
      compute(s);
      stage_write(s + 1, stB);
      __syncthreads();
      compute(s + 1);
      stage_write(s + 2, stA);
      __syncthreads();
      compute(s + 2);
    } else if (left == 2) {
      compute(s);
      stage_write(s + 1, stB);
      __syncthreads();
      compute(s + 1);
    } else {
      compute(s);
    }
    __syncthreads();
  }
}

// The same stacks with the staging done by LDS-DMA (global_load_lds_dwordx4: 16 bytes per lane straight into the LDS at a
// wave-uniform base + 16 * lane, which is exactly the staged image's layout) into a ring of four slots of one vector each:
// no staging registers (the register-staged kernel above spills at R = 2 in fp64), no ds_write pass, and three vectors in
// flight instead of two steps.  One step = one vector:  wait until its DMAs have landed (counted vmcnt: the DMAs of the
// two later vectors stay in flight);  barrier (every wave's pieces are there, and every
// wave is done with the slot the next DMA overwrites);  issue the DMAs of the vector three steps ahead;  row products
// of this vector out of its slot and the R stores.  The compiler does not count asm loads, so every wait on the DMAs is
// written here, from the number of DMAs this wave has issued after them (LDS-DMAs complete in order among themselves);
// a stack with a ragged member (the last row block of the matrix) waits for vmcnt(0) instead.
// The floor of this access pattern -- DMAs, stores and the entries, no LDS reads -- was measured at 1.09 of the kernel's
// 1.15-1.20 ms on lap3d 215^3 fp64 (profiles/r03_spmm_stack.txt, section 5); a version whose ring ran on across the stack
// boundaries, with the next stack's entries prefetched into a second register set, measured the same and is not kept.
template <int N> __device__ __forceinline__ void wait_vm_le() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); }

// wait until at most n vector-memory operations of this wave are outstanding (s_waitcnt takes an immediate)
__device__ __forceinline__ void wait_vm_outstanding(int n) {
#define RLH_WC(k) case k: wait_vm_le<k>(); break;
#define RLH_WC8(k) RLH_WC(k) RLH_WC(k + 1) RLH_WC(k + 2) RLH_WC(k + 3) RLH_WC(k + 4) RLH_WC(k + 5) RLH_WC(k + 6) RLH_WC(k + 7)
  switch (n) {
    RLH_WC8(0) RLH_WC8(8) RLH_WC8(16)
    default: wait_vm_le<0>(); break;              // (never too little)
  }
#undef RLH_WC8
#undef RLH_WC
}

// "this value is needed now" for the compiler's wait placement
__device__ __forceinline__ void stk_touch(float &v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void stk_touch(double &v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void stk_touch(c32 &v) { asm volatile("" : "+v"(v.re), "+v"(v.im)); }
__device__ __forceinline__ void stk_touch(c64 &v) { asm volatile("" : "+v"(v.re), "+v"(v.im)); }

// one store instruction per value (the waits count instructions)
__device__ __forceinline__ void stk_store(float *p, float v) { __builtin_nontemporal_store(v, p); }
__device__ __forceinline__ void stk_store(double *p, double v) { __builtin_nontemporal_store(v, p); }
__device__ __forceinline__ void stk_store(c32 *p, c32 v) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  __builtin_nontemporal_store(f32x2{v.re, v.im}, reinterpret_cast<f32x2 *>(p));
}
__device__ __forceinline__ void stk_store(c64 *p, c64 v) {
  typedef double f64x2 __attribute__((ext_vector_type(2)));
  __builtin_nontemporal_store(f64x2{v.re, v.im}, reinterpret_cast<f64x2 *>(p));
}

// CHEB (16-byte elements): the fused Chebyshev step  P = cy y + cp P + cb (B - A y)  on the same ring -- X is y (staged),
// Y is P (read and written in place), y[row] comes out of the staged image (slot 7 of every row holds its own column's
// position: stk_self).  P and B are ordinary loads, and ordinary loads and LDS-DMAs do not retire in order with each other
// (see the waits below), so this variant never counts: every wait is for everything.  With the two slots of a 16-byte ring
// that costs nothing in depth -- the DMA of vector j + 1 and the operands of vector j are in flight together while the
// products of vector j are formed, one wait, then the update and its stores.
template <typename T, int R, int LD, bool CHEB = false>
__global__ __launch_bounds__(1024) void well_stack_dma_kernel(const WellMeta *__restrict__ meta,
                                                              const int32_t *__restrict__ member,
                                                              const int32_t *__restrict__ gsrc,
                                                              const uint16_t *__restrict__ idx,
                                                              const T *__restrict__ vals, const int32_t *__restrict__ pat,
                                                              const uint16_t *__restrict__ dtab, int64_t n_rows,
                                                              const int32_t *__restrict__ sched, int64_t sched_len,
                                                              const T *__restrict__ X, int64_t ldx, int64_t n_own,
                                                              const T *__restrict__ H, int64_t ldh,
                                                              T *__restrict__ Y, int64_t ldy, int m, ChebArgs<T> cheb) {
  constexpr int WMAX = 8;
  constexpr int NB = StkRing<T>::NB, D = NB - 1;   // D vectors ahead
  static_assert(!CHEB || NB == 2, "the fused step drains the ring every vector: two slots only");
  constexpr int SLOT = StkRing<T>::SLOT;
  constexpr int EPL = 16 / (int)sizeof(T);         // elements per 16-byte piece
  constexpr int LPG = 64 / EPL;
  static_assert((D - 1) * LD + D * R < 24, "wait_vm_outstanding's cases");      // (10 + 6)
  extern __shared__ __align__(16) char ldsb[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int64_t pos = blockIdx.x; pos < sched_len; pos += gridDim.x) {
    const int64_t sb = sched[pos];
    if (sb < 0) continue;
    const WellMeta mt = meta[sb];
    const int ng = mt.width_ng >> 8;               // a multiple of 8, <= SLOT / (64 sizeof(T)) and <= 16 EPL LD
    // entries: values, and two 16-bit positions per register as stored (unpacked at use)
    int row[R];                                    // this thread's row of member r (-1: none), 32 bits: n < 2^31
    T v[R][WMAX];
    unsigned ixb[R][WMAX / 2];
    bool whole = true;                             // every member present has all its 1024 rows (workgroup-uniform)
    int nmem = 0;                                  // members present: the first nmem (a stack of one: the plain block)
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int2 mr = reinterpret_cast<const int2 *>(member)[sb * R + r];       // first row, rows (0: no such member)
      if (mr.y > 0) {
        nmem = r + 1;
        whole = whole && mr.y == kWellRows;
      }
      row[r] = tid < mr.y ? mr.x + tid : -1;
      unsigned px[WMAX];
      // (not for 16-byte elements: the second path costs complex128 six spilled registers, and scratch traffic would
      // sit in the same counter as the DMAs)
      if (sizeof(T) < 16 && pat) well_load_entries_pat<T, WMAX>(vals, pat, dtab, idx, mt.eoff + 8 * r, sb * R + r, tid, v[r], px);
      else well_load_entries<T, WMAX>(vals, idx, mt.eoff + 8 * r, tid, WMAX, v[r], px);
#pragma unroll
      for (int t = 0; t < WMAX; t += 2) ixb[r][t / 2] = px[t] | (px[t + 1] << 16);
    }
    // a vector's image is ng / EPL pieces of 16 bytes per lane, moved by the first nw waves, LD pieces each at most: wave
    // w takes pieces w, w + nw, ...: `mine` of them (the waits below count per wave; a wave with many pieces keeps more
    // of the later vectors in flight behind the interleaved stores than sixteen waves with one or two each)
    int scol[LD];                                  // first column this lane fetches, per piece
    const int npieces = ng / EPL;
    const int nw = __builtin_amdgcn_readfirstlane((npieces + LD - 1) / LD);
    const int mine = __builtin_amdgcn_readfirstlane(wave < nw ? (npieces - wave + nw - 1) / nw : 0);
#pragma unroll
    for (int i = 0; i < LD; ++i) {
      int q = (wave + nw * i) * EPL;
      if (q > ng - EPL) q = ng - EPL;              // (a piece this wave does not have: any valid address)
      scol[i] = gsrc[mt.goff + q + lane / LPG] + (lane % LPG) * EPL;
    }
    // the entries and the staging plan are in their registers before the first DMA is issued: the compiler's own wait for
    // them would otherwise come at their first use, inside the pipeline, as a vmcnt(0) that drains the ring
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
      for (int t = 0; t < WMAX; ++t) stk_touch(v[r][t]);
#pragma unroll
      for (int t = 0; t < WMAX / 2; ++t) asm volatile("" : "+v"(ixb[r][t]));
    }
#pragma unroll
    for (int i = 0; i < LD; ++i) asm volatile("" : "+v"(scol[i]));
    auto issue = [&](int j) {                      // the DMAs of vector j into slot j % NB
      const unsigned slot = (unsigned)(j & (NB - 1)) * (unsigned)SLOT;
      const T *src = X + (int64_t)j * ldx;
      const T *hsrc = H ? H + (int64_t)j * ldh - n_own : src;   // halo row of column c: hsrc[c] (pieces never lie across n_own)
#pragma unroll
      for (int i = 0; i < LD; ++i) {
        if (i >= mine) break;
        const T *g = (scol[i] < n_own ? src : hsrc) + scol[i];
        unsigned dst = slot + (unsigned)(wave + nw * i) * 1024u, keep;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(g), "s"(dst) : "memory");
      }
    };
    auto compute = [&](int j) {
      unsigned boff = (unsigned)(j & (NB - 1)) * (unsigned)SLOT;
      asm volatile("" : "+s"(boff));
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (r >= nmem) break;
        T acc = zero_of(T{});
#pragma unroll
        for (int t = 0; t < WMAX; t += 2) {
          unsigned w = ixb[r][t / 2];
          asm volatile("" : "+v"(w));              // (unpacked per vector: hoisted out of the loop the offsets take 16 registers)
          fma_acc(acc, v[r][t], *reinterpret_cast<const T *>(ldsb + ((w & 0xffffu) * (unsigned)sizeof(T) + boff)));
          fma_acc(acc, v[r][t + 1], *reinterpret_cast<const T *>(ldsb + ((w >> 16) * (unsigned)sizeof(T) + boff)));
        }
        // (non-temporal stores: 1.107 against 1.140 ms with plain ones, variants taking turns in one process)
        if (whole || row[r] >= 0) stk_store(Y + (int64_t)row[r] + (int64_t)j * ldy, acc);
      }
    };
    // every wave is done with the previous stack's slots (its last vectors were read after the last barrier)
    __builtin_amdgcn_s_barrier();
    if constexpr (CHEB) {
      issue(0);
      for (int j = 0; j < m; ++j) {
        if (j == 0) wait_vm_outstanding(0);        // (later vectors: drained by the wait below)
        // every wave's pieces of vector j have landed, and every wave has formed its products of vector j - 1: the
        // other slot is free
        __builtin_amdgcn_s_barrier();
        if (j + 1 < m) issue(j + 1);
        unsigned boff = (unsigned)(j & (NB - 1)) * (unsigned)SLOT;
        asm volatile("" : "+s"(boff));
        // one member at a time -- products, operands, wait, update: the kernel sits at the 128 registers a wave of a
        // 1024-thread workgroup has (the entries alone are 16 per row), and a spilled operand is reloaded behind a wait of
        // its own.  Slot 7 is the row's own column with value 0: y[row], not part of the product.  The first member's
        // wait covers the ring's DMA, which has been in flight since before its products.
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if (r >= nmem) break;
          T acc = zero_of(T{});
#pragma unroll
          for (int t = 0; t < WMAX - 2; t += 2) {
            unsigned w = ixb[r][t / 2];
            asm volatile("" : "+v"(w));
            fma_acc(acc, v[r][t], *reinterpret_cast<const T *>(ldsb + ((w & 0xffffu) * (unsigned)sizeof(T) + boff)));
            fma_acc(acc, v[r][t + 1], *reinterpret_cast<const T *>(ldsb + ((w >> 16) * (unsigned)sizeof(T) + boff)));
          }
          unsigned w = ixb[r][WMAX / 2 - 1];
          asm volatile("" : "+v"(w));
          fma_acc(acc, v[r][WMAX - 2], *reinterpret_cast<const T *>(ldsb + ((w & 0xffffu) * (unsigned)sizeof(T) + boff)));
          const T yv = *reinterpret_cast<const T *>(ldsb + ((w >> 16) * (unsigned)sizeof(T) + boff));
          T out = sub_of(scale_of(cheb.cy, yv), scale_of(cheb.cb, acc));
          const bool live = whole || row[r] >= 0;
          T *pp = Y + (int64_t)row[r] + (int64_t)j * ldy;
          T pv = zero_of(T{}), bv = zero_of(T{});
          if (live) {
            pv = *pp;
            bv = cheb.B[(int64_t)row[r] + (int64_t)j * cheb.ldb];
          }
          wait_vm_outstanding(0);
          stk_touch(pv);
          stk_touch(bv);
          out = add_of(add_of(out, scale_of(cheb.cp, pv)), scale_of(cheb.cb, bv));
          if (live) stk_store(pp, out);
        }
      }
      continue;
    }
    for (int j = 0; j < D && j < m; ++j) issue(j);
    for (int j = 0; j < m; ++j) {
      // DMAs issued after those of vector j: the later vectors in flight.  The stores of the last steps are younger too,
      // but they are NOT counted as allowed: LDS-DMAs and ordinary vector-memory operations do not complete in order with
      // each other (seen with loads in the bfloat16 kernel below), and a store that has completed early would let an
      // unfinished DMA through the count; if they are still outstanding this waits for one more vector than necessary
      // (counting them as allowed measured the same time to within the noise: profiles/r03_spmm_stack.txt).
      const int later = m - 1 - j < D - 1 ? m - 1 - j : D - 1;
      // (a short member -- the last block of the matrix, or the plane-aligned blocks -- changes nothing here: the count
      // rests on the DMAs alone, whatever stores a wave does or does not issue)
      wait_vm_outstanding(later * mine);
      __builtin_amdgcn_s_barrier();
      if (j + D < m) issue(j + D);
      compute(j);
    }
  }
}

// ------------------------------------------------------------------ bfloat16 Chebyshev step
// The fused three-term step with the three blocks y, p, b stored as bfloat16 (the preconditioner
// only steers the search directions: on lap3d 64^3, degree 24, the iteration count goes from 27 to
// 28 with bfloat16 storage) and all arithmetic in float32 against the float32 windowed operator.
// Per element the step then moves 2-byte values: 4.5 x 2 bytes instead of 4.5 x 4.
//  * staging: a 16-byte piece is 8 elements, one wave load covers 8 groups (1 KiB); the LDS image
//    is bfloat16 (an entry's position times 2 is its byte offset), 8 vectors per step;
//  * the row results of 8 vectors go through a wave-private LDS tile [vector][row] and come back
//    as 8 consecutive rows of ONE vector per lane, so y, p, b are read and p is written as 16-byte
//    pieces (one wave access = the wave's 64 rows x 8 vectors).
// (bf16_to_f32, f32_to_bf16 and cheb_update are in spmm.h: the interleaved layout's step shares them)
struct alignas(16) Bf8 { unsigned short e[8]; };
struct alignas(8) Bf8U { unsigned short e[8]; };                           // staging piece: groups start on multiples of 4 columns

constexpr int kBfCps = 8;                          // vectors per step (fewer when 8 staged images exceed a buffer)
constexpr int kBfBufBytes = 56 * 1024;             // per staging buffer (2 of them + 32 KiB of wave tiles)

template <int WMAX>
__global__ __launch_bounds__(1024) void well_cheb_bf16_kernel(const WellMeta *__restrict__ meta,
                                                              const int32_t *__restrict__ gsrc,
                                                              const uint16_t *__restrict__ idx,
                                                              const float *__restrict__ vals, int64_t n_rows,
                                                              const int32_t *__restrict__ sched, int64_t sched_len,
                                                              const unsigned short *__restrict__ Yk, int64_t ldy,
                                                              int64_t n_own, const unsigned short *__restrict__ H,
                                                              int64_t ldh,
                                                              unsigned short *__restrict__ P, int64_t ldp,
                                                              const unsigned short *__restrict__ B, int64_t ldb,
                                                              int m, float cy, float cp, float cb) {
  constexpr int SLOTS = 4;                         // ceil(56 KiB / 16 B / 1024 threads)
  __shared__ __attribute__((aligned(16))) char ldsb[2 * kBfBufBytes + 16 * kBfCps * 64 * 4];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float *tile = reinterpret_cast<float *>(ldsb + 2 * kBfBufBytes) + wave * (kBfCps * 64);   // [vector][row] of this wave
  for (int64_t pos = blockIdx.x; pos < sched_len; pos += gridDim.x) {
    const int64_t b = sched[pos];
    if (b < 0) continue;
    const WellMeta mt = meta[b];
    const int width = mt.width_ng & 255;
    const int ng = mt.width_ng >> 8;               // multiple of 8, <= 128
    const int F2 = ng * 128;                       // bytes per staged vector
    int cps = kBfBufBytes / F2;                    // >= 3
    if (cps > kBfCps) cps = kBfCps;
    if (cps > m) cps = m;
    const int nsteps = (m + cps - 1) / cps;
    const int G = ng * cps;                        // staging groups per step (G / 8 <= 56 pieces: 4 per wave)
    const int64_t row0 = b * kWellRows + (int64_t)wave * 64;      // first row of this wave
    const int64_t row = row0 + lane;
    float v[WMAX];
    unsigned ixb[WMAX];
    well_load_entries<float, WMAX>(vals, idx, mt.eoff, tid, width, v, ixb);
#pragma unroll
    for (int t = 0; t < WMAX; ++t) ixb[t] *= 2u;        // byte offset in the bfloat16 image
    // staging slots: 8 groups (one 16-byte piece per lane) each
    int sbase[SLOTS], scc[SLOTS], scol[SLOTS];
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
      int q = (wave + 16 * i) * 8;
      if (q > G - 8) q = G - 8;                    // surplus slots repeat the last groups
      const int cc = q / ng, g = q - cc * ng;
      scc[i] = __builtin_amdgcn_readfirstlane(cc);
      sbase[i] = __builtin_amdgcn_readfirstlane(cc * F2 + g * 128);
      scol[i] = gsrc[mt.goff + g + lane / 8] + (lane % 8) * 8;
    }
    Bf8U stA[SLOTS], stB[SLOTS];
    auto stage_load = [&](int s, Bf8U (&st)[SLOTS]) {
#pragma unroll
      for (int i = 0; i < SLOTS; ++i) {
        int j = s * cps + scc[i];
        if (j > m - 1) j = m - 1;
        const int c = scol[i];                      // (pieces never lie across n_own: the host checked)
        const unsigned short *src = c < n_own ? Yk + (int64_t)j * ldy + c : H + (int64_t)j * ldh + (c - n_own);
        st[i] = *reinterpret_cast<const Bf8U *>(src);
      }
    };
    auto stage_write = [&](int s, const Bf8U (&st)[SLOTS]) {
      unsigned boff = (unsigned)(s & 1) * (unsigned)kBfBufBytes;
      asm volatile("" : "+s"(boff));
#pragma unroll
      for (int i = 0; i < SLOTS; ++i) {
        Bf8 val;
#pragma unroll
        for (int k = 0; k < 8; ++k) val.e[k] = st[i].e[k];
        *reinterpret_cast<Bf8 *>(ldsb + ((unsigned)lane * 16u + (boff + (unsigned)sbase[i]))) = val;
      }
    };
    auto compute = [&](int s) {
      unsigned boff = (unsigned)(s & 1) * (unsigned)kBfBufBytes;
      const int j0 = s * cps;
      // after the row products, lane L takes vector j0 + L / 8, rows 8 (L % 8) .. + 7 of the wave's 64;
      // its pieces of p, b, y are requested FIRST (from clamped, always valid addresses) so that
      // their latency passes under the LDS work below instead of after it
      const int c8 = lane >> 3, rg = lane & 7;
      const int j = j0 + c8;
      const int64_t r8 = row0 + rg * 8;
      const bool mine = c8 < cps && j < m && r8 < n_rows;
      const bool whole = mine && r8 + 8 <= n_rows;
      const int jc = j < m ? j : m - 1;
      const int64_t rc = whole ? r8 : 0;
      unsigned short *pp = P + (int64_t)jc * ldp + rc;
      const Bf8 pv = *reinterpret_cast<const Bf8 *>(pp);           // (the host checked 16-byte alignment)
      const Bf8 bv = *reinterpret_cast<const Bf8 *>(B + (int64_t)jc * ldb + rc);
      const Bf8 yv = *reinterpret_cast<const Bf8 *>(Yk + (int64_t)jc * ldy + rc);
      // (A y)[row] for the step's vectors -> the wave's tile
#pragma unroll 1
      for (int c = 0; c < cps; ++c) {
        unsigned bo = boff + (unsigned)c * (unsigned)F2;
        asm volatile("" : "+s"(bo));
        float acc = 0.f;
        if (j0 + c < m) {
#pragma unroll
          for (int t = 0; t < WMAX; ++t)
            acc = fmaf(v[t], bf16_to_f32(*reinterpret_cast<const unsigned short *>(ldsb + (ixb[t] + bo))), acc);
        }
        tile[c * 64 + lane] = acc;
      }
      const int ct = c8 < cps ? c8 : 0;
      float t8[8];
      {
        const float4 lo = *reinterpret_cast<const float4 *>(tile + ct * 64 + rg * 8);
        const float4 hi = *reinterpret_cast<const float4 *>(tile + ct * 64 + rg * 8 + 4);
        t8[0] = lo.x; t8[1] = lo.y; t8[2] = lo.z; t8[3] = lo.w;
        t8[4] = hi.x; t8[5] = hi.y; t8[6] = hi.z; t8[7] = hi.w;
      }
      if (whole) {
        Bf8 out;
#pragma unroll
        for (int k = 0; k < 8; ++k)
          out.e[k] = f32_to_bf16(cheb_update(cy, bf16_to_f32(yv.e[k]), cp, bf16_to_f32(pv.e[k]), cb, bf16_to_f32(bv.e[k]), t8[k]));
        *reinterpret_cast<Bf8 *>(pp) = out;
      } else if (mine) {                           // the last rows of the matrix
        unsigned short *pq = P + (int64_t)j * ldp + r8;
        const unsigned short *bq = B + (int64_t)j * ldb + r8, *yq = Yk + (int64_t)j * ldy + r8;
        for (int k = 0; k < 8 && r8 + k < n_rows; ++k)
          pq[k] = f32_to_bf16(cheb_update(cy, bf16_to_f32(yq[k]), cp, bf16_to_f32(pq[k]), cb, bf16_to_f32(bq[k]), t8[k]));
      }
    };
    stage_load(0, stA);
    stage_load(1, stB);                            // (clamped to the last vector if there is no step 1)
    stage_write(0, stA);
    __syncthreads();
    int s = 0;
    for (; s + 3 < nsteps; s += 2) {
      stage_load(s + 2, stA);
      compute(s);
      stage_write(s + 1, stB);
      __syncthreads();
      stage_load(s + 3, stB);
      compute(s + 1);
      stage_write(s + 2, stA);
      __syncthreads();
    }
    const int left = nsteps - s;
    if (left == 3) {
      stage_load(s + 2, stA);
      compute(s);
      stage_write(s + 1, stB);
      __syncthreads();
      compute(s + 1);
      stage_write(s + 2, stA);
      __syncthreads();
      compute(s + 2);
    } else if (left == 2) {
      compute(s);
      stage_write(s + 1, stB);
      __syncthreads();
      compute(s + 1);
    } else {
      compute(s);
    }
    __syncthreads();
  }
}


template <typename T, int WMAX, int EPL>
static int launch_well_we(const rlh_csr *h, int part, int64_t m, const T *X, int64_t ldx, int64_t n_own, const T *H,
                          int64_t ldh, T *Y, int64_t ldy, const ChebArgs<T> *cheb) {
  Context &c = ctx();
  // launch order: all blocks, or the blocks without / with halo columns (rlh_spmm_part)
  const int32_t *sched;
  int64_t sched_len;
  int nb;                                               // one workgroup per CU, persistent
  h->well_launch.pick(part, &sched, &sched_len, &nb);
  if (nb == 0) return 0;
  const int cps_cap = env_int("RLH_SPMM_CPS", 8);       // vectors per step (tunable)
  if (cheb)
    hipLaunchKernelGGL((well_spmm_kernel<T, WMAX, EPL, true>), dim3((unsigned)nb), dim3(1024), 0, c.stream,
                       h->well_meta, h->well_gsrc, h->well_idx, (const T *)h->well_vals, h->n_rows, h->n_cols,
                       sched, sched_len, X, ldx, n_own, H, ldh, Y, ldy, (int)m,
                       cps_cap < 1 ? 1 : cps_cap, *cheb);
  else
    hipLaunchKernelGGL((well_spmm_kernel<T, WMAX, EPL, false>), dim3((unsigned)nb), dim3(1024), 0, c.stream,
                       h->well_meta, h->well_gsrc, h->well_idx, (const T *)h->well_vals, h->n_rows, h->n_cols,
                       sched, sched_len, X, ldx, n_own, H, ldh, Y, ldy, (int)m,
                       cps_cap < 1 ? 1 : cps_cap, ChebArgs<T>{});
  note_launch(cheb ? "well epl=%d cheb=1" : "well epl=%d cheb=0", EPL, 0, 0, 0, nb, sched_len);
  RLH_HIP(hipGetLastError());
  return 0;
}

template <typename T, int WMAX>
static int launch_well_w(const rlh_csr *h, int part, int64_t m, const T *X, int64_t ldx, int64_t n_own, const T *H,
                         int64_t ldh, T *Y, int64_t ldy, const ChebArgs<T> *cheb) {
  // 16-byte staging loads when every piece is whole: groups inside the column range, and with a
  // halo block no piece across the own / halo boundary (aligned groups, n_own a multiple of the
  // piece); the addresses themselves only need T's alignment
  constexpr int EPL = 16 / (int)sizeof(T);
  if constexpr (EPL > 1) {
    const int vec = env_int("RLH_SPMM_VEC", 1);         // 0: 8-byte staging (tunable)
    const bool whole = h->stage_inbounds && (H == nullptr || n_own == h->n_cols || (h->stage_aligned && n_own % EPL == 0));
    if (vec && whole) return launch_well_we<T, WMAX, EPL>(h, part, m, X, ldx, n_own, H, ldh, Y, ldy, cheb);
  }
  return launch_well_we<T, WMAX, 1>(h, part, m, X, ldx, n_own, H, ldh, Y, ldy, cheb);
}

// ------------------------------------------------------------------ bfloat16 Chebyshev step on the stacks
// The fused step of well_cheb_bf16_kernel on the stacked layout, staged by LDS-DMA like well_stack_dma_kernel.  At the
// block size the driver uses for ten eigenpairs (16 vectors) the kernel above spends its time at block boundaries -- two
// steps of eight vectors per block, 1.75 GB of algorithmic traffic in 457 us = 3.8 TB/s -- so here:
//  * two slots of VPS = 2 bfloat16 images (16 KB each: ng <= 128 groups);  one step = VPS vectors: wait for the step's
//    DMAs (issued during the step before), barrier, DMAs of the next step into the other slot, the row products of the
//    stack's two members into registers.  (One vector per step with a ring of 2, 4 or 6 slots: 380 us; two per step: 363.)
//  * every eight vectors the results go through a wave-private tile [vector][row] and come back as eight consecutive
//    rows of one vector per lane, so that y, p, b are read and p is written as 16-byte pieces.  Those operands (three
//    quarters of the step's traffic) are LDS-DMAs too -- into a wave-private area, 1 KB per operand and member, issued at
//    the start of the group of eight: as ordinary loads they did NOT complete in order with the DMAs (a counted wait on
//    a DMA issued after them returned with their registers still in flight: NaNs at 215^3, none in the small tests),
//    and a vmcnt(0) for them would wait for the vectors in flight as well.
//  * a step's DMAs are issued during the step before, so the only DMAs younger than them are, at the first step of a
//    group, the group's 3 nmem operand DMAs (issued in the previous group's epilogue, ahead of its stores): that is what
//    the wait allows.
constexpr int kBfImageBytes = 16 * 1024;           // ng <= 128 groups of 64 two-byte elements
constexpr int kBfRingBytes = 64 * 1024;
constexpr int kBfOperandBytes = 6 * 1024;          // per wave: [member][p, b, y] x 64 lanes x 16 bytes (its first 2 KB double as the tile)

// (where the step's time goes -- y DMAs, row products, operand DMAs and update taken out in turn -- is measured in
// profiles/r03_spmm_stack.txt, section 10)
template <int R, int VPS>
__global__ __launch_bounds__(1024) void well_stack_cheb_bf16_kernel(const WellMeta *__restrict__ meta,
                                                                    const int32_t *__restrict__ member,
                                                                    const int32_t *__restrict__ gsrc,
                                                                    const uint16_t *__restrict__ idx,
                                                                    const float *__restrict__ vals,
                                                                    const int32_t *__restrict__ pat,
                                                                    const uint16_t *__restrict__ dtab, int64_t n_rows,
                                                                    const int32_t *__restrict__ sched, int64_t sched_len,
                                                                    const unsigned short *__restrict__ Yk, int64_t ldy,
                                                                    int64_t n_own, const unsigned short *__restrict__ H,
                                                                    int64_t ldh, unsigned short *__restrict__ P, int64_t ldp,
                                                                    const unsigned short *__restrict__ B, int64_t ldb,
                                                                    int m, float cy, float cp, float cb) {
  constexpr int WMAX = 8, IMG = kBfImageBytes, SLOT = VPS * IMG;       // two slots of VPS images
  static_assert(R * 3 * 1024 <= kBfOperandBytes && 2 * SLOT <= kBfRingBytes && 8 % VPS == 0, "operand area; ring");
  extern __shared__ __align__(16) char ldsb[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned opbase = (unsigned)kBfRingBytes + (unsigned)wave * (unsigned)kBfOperandBytes;   // this wave's operand area
  const int c8 = lane >> 3, rg = lane & 7;         // epilogue: vector c8 of the group, rows 8 rg .. 8 rg + 7 of the wave's 64
  auto dma16 = [&](const void *g, unsigned dst) {  // 16 bytes per lane to the LDS at dst + 16 lane (dst wave-uniform)
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(g), "s"(dst) : "memory");
  };
  for (int64_t pos = blockIdx.x; pos < sched_len; pos += gridDim.x) {
    const int64_t sb = sched[pos];
    if (sb < 0) continue;
    const WellMeta mt = meta[sb];
    const int ng = mt.width_ng >> 8;               // a multiple of 8, <= 128
    int64_t row0[R];                               // first of this wave's 64 rows in member r
    float v[R][WMAX];
    unsigned ixb[R][WMAX / 2];
    bool whole = true;
    int nmem = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int2 mr = reinterpret_cast<const int2 *>(member)[sb * R + r];       // first row (a multiple of 8 here), rows
      if (mr.y > 0) {
        nmem = r + 1;
        whole = whole && mr.y == kWellRows;
      }
      // (float32 operators keep the uniform 1024-row blocks: a short member can only be the last block of the matrix, so
      // "row < n_rows" below is "row is in the member")
      row0[r] = mr.y > 0 ? (int64_t)mr.x + (int64_t)wave * 64 : n_rows;
      unsigned px[WMAX];
      if (pat) well_load_entries_pat<float, WMAX>(vals, pat, dtab, idx, mt.eoff + 8 * r, sb * R + r, tid, v[r], px);
      else well_load_entries<float, WMAX>(vals, idx, mt.eoff + 8 * r, tid, WMAX, v[r], px);
#pragma unroll
      for (int t = 0; t < WMAX; t += 2) ixb[r][t / 2] = px[t] | (px[t + 1] << 16);
    }
    // one 16-byte piece per lane = 8 elements: a wave's DMA covers 8 groups; wave w moves piece w of the ng / 8
    const int mine = __builtin_amdgcn_readfirstlane(wave < ng / 8 ? 1 : 0);
    int scol;
    {
      int q = wave * 8;
      if (q > ng - 8) q = ng - 8;
      scol = gsrc[mt.goff + q + lane / 8] + (lane % 8) * 8;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
      for (int t = 0; t < WMAX; ++t) asm volatile("" : "+v"(v[r][t]));
#pragma unroll
      for (int t = 0; t < WMAX / 2; ++t) asm volatile("" : "+v"(ixb[r][t]));
    }
    asm volatile("" : "+v"(scol));
    auto issue = [&](int j, unsigned par) {        // the images of vectors j, j + 1 (clamped) into slot `par`
      if (!mine) return;
#pragma unroll
      for (int u = 0; u < VPS; ++u) {
        const int jv = j + u < m ? j + u : m - 1;
        dma16((scol < n_own ? Yk + (int64_t)jv * ldy : H + (int64_t)jv * ldh - n_own) + scol,
              par * (unsigned)SLOT + (unsigned)u * (unsigned)IMG + (unsigned)wave * 1024u);
      }
    };
    __builtin_amdgcn_s_barrier();                  // every wave is done with the previous stack's slots
    unsigned par = 0;                              // slot of the step in hand
    issue(0, 0);
    // this lane's operands of the update of the group that starts at vector j0: rows r8 .. r8 + 7 of vector j0 + c8
    // (clamped where the lane has none), 3 nmem DMAs per wave
    auto operands = [&](int j0) {
      const int jv = j0 + c8;
      const int jc = jv < m ? jv : m - 1;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (r >= nmem) break;
        const int64_t r8 = row0[r] + rg * 8;
        const int64_t rc = r8 + 8 <= n_rows ? r8 : 0;
        dma16(P + (int64_t)jc * ldp + rc, opbase + (unsigned)(r * 3 + 0) * 1024u);
        dma16(B + (int64_t)jc * ldb + rc, opbase + (unsigned)(r * 3 + 1) * 1024u);
        dma16(Yk + (int64_t)jc * ldy + rc, opbase + (unsigned)(r * 3 + 2) * 1024u);
      }
    };
    operands(0);
    for (int j0 = 0; j0 < m; j0 += 8) {
      const int cnt = m - j0 < 8 ? m - j0 : 8;     // vectors of this group
      const int jv = j0 + c8;
      const bool act = c8 < cnt;
      float acc[R][8];
#pragma unroll
      for (int jj = 0; jj < 8; jj += VPS) {
#pragma unroll
        for (int u = 0; u < VPS; ++u)
#pragma unroll
          for (int r = 0; r < R; ++r) acc[r][jj + u] = 0.f;
        if (jj < cnt) {
          const int j = j0 + jj;
          // (a wave that moves no image has nothing to wait for here -- and must not: a wait would make it, and through
          // the barrier every wave, sit out the acknowledgement of its last stores)
          if (!whole) wait_vm_le<0>();
          else if (mine) wait_vm_outstanding(jj == 0 ? 3 * nmem : 0);
          __builtin_amdgcn_s_barrier();
          const int jn = jj + VPS < cnt ? j + VPS : j0 + 8;          // first vector of the next step
          if (jn < m) issue(jn, par ^ 1u);
          unsigned boff = par * (unsigned)SLOT;
          asm volatile("" : "+s"(boff));
#pragma unroll
          for (int u = 0; u < VPS; ++u) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
              if (r >= nmem) break;
              float a = 0.f;
#pragma unroll
              for (int t = 0; t < WMAX; t += 2) {
                unsigned w = ixb[r][t / 2];
                asm volatile("" : "+v"(w));
                a = fmaf(v[r][t], bf16_to_f32(*reinterpret_cast<const unsigned short *>(ldsb + ((w & 0xffffu) * 2u + boff))), a);
                a = fmaf(v[r][t + 1], bf16_to_f32(*reinterpret_cast<const unsigned short *>(ldsb + ((w >> 16) * 2u + boff))), a);
              }
              acc[r][jj + u] = a;                   // (a vector past the block's last: computed on a repeated image, not used)
            }
            boff += (unsigned)IMG;
          }
          par ^= 1u;
        }
      }
      // the operands have landed with the DMAs of the group's last step, issued after them -- unless the group has one
      // step only (or this wave issues no vector DMAs)
      if (cnt <= VPS || !mine || !whole) wait_vm_le<0>();
      // the update of this group, member by member; the member's operands first (their area doubles as the tile)
      rlh_u32x4e outs[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (r >= nmem) break;
        union { rlh_u32x4e u; unsigned short e[8]; } pu, bu, yu, ou;
        pu.u = *reinterpret_cast<const rlh_u32x4e *>(ldsb + opbase + (unsigned)(r * 3 + 0) * 1024u + (unsigned)lane * 16u);
        bu.u = *reinterpret_cast<const rlh_u32x4e *>(ldsb + opbase + (unsigned)(r * 3 + 1) * 1024u + (unsigned)lane * 16u);
        yu.u = *reinterpret_cast<const rlh_u32x4e *>(ldsb + opbase + (unsigned)(r * 3 + 2) * 1024u + (unsigned)lane * 16u);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // (read before the tile overwrites them)
        float *tile = reinterpret_cast<float *>(ldsb + opbase + (unsigned)(r * 3) * 1024u);
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) tile[jj * 64 + lane] = acc[r][jj];
        float t8[8];
        {
          const float4 lo = *reinterpret_cast<const float4 *>(tile + c8 * 64 + rg * 8);
          const float4 hi = *reinterpret_cast<const float4 *>(tile + c8 * 64 + rg * 8 + 4);
          t8[0] = lo.x; t8[1] = lo.y; t8[2] = lo.z; t8[3] = lo.w;
          t8[4] = hi.x; t8[5] = hi.y; t8[6] = hi.z; t8[7] = hi.w;
        }
        const int64_t r8 = row0[r] + rg * 8;
        if (whole || r8 + 8 <= n_rows) {
#pragma unroll
          for (int k = 0; k < 8; ++k)
            ou.e[k] = f32_to_bf16(cheb_update(cy, bf16_to_f32(yu.e[k]), cp, bf16_to_f32(pu.e[k]), cb, bf16_to_f32(bu.e[k]), t8[k]));
          outs[r] = ou.u;
        } else if (act && r8 < n_rows) {           // the last rows of the matrix
          unsigned short *pq = P + (int64_t)jv * ldp + r8;
          const unsigned short *bq = B + (int64_t)jv * ldb + r8, *yq = Yk + (int64_t)jv * ldy + r8;
          for (int k = 0; k < 8 && r8 + k < n_rows; ++k)
            pq[k] = f32_to_bf16(cheb_update(cy, bf16_to_f32(yq[k]), cp, bf16_to_f32(pq[k]), cb, bf16_to_f32(bq[k]), t8[k]));
        }
      }
      // the next group's operands BEFORE this group's stores (this wave's reads of the area are done: its own LDS
      // operations complete in order, and t8 has been consumed): the stores are then the youngest operations of the wave and
      // no counted wait ever has to sit out their acknowledgement
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (j0 + 8 < m) operands(j0 + 8);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (r >= nmem) break;
        const int64_t r8 = row0[r] + rg * 8;
        if ((whole || r8 + 8 <= n_rows) && act) *reinterpret_cast<rlh_u32x4e *>(P + (int64_t)jv * ldp + r8) = outs[r];
      }
    }
  }
}

// one launch of the LDS-DMA stack kernel (CHEB: its fused Chebyshev step)
template <typename T, bool CHEB>
static int launch_stack_dma(const rlh_csr *h, const int32_t *pat, const int32_t *sched, int64_t sched_len, int grid, int64_t m,
                            const T *X, int64_t ldx, int64_t n_own, const T *H, int64_t ldh, T *Y, int64_t ldy,
                            const ChebArgs<T> &cheb) {
  constexpr int LD = 5;                                  // 16-byte pieces per issuing wave and vector (<= 80 pieces)
  static bool attr_dma = false;
  if (!attr_dma) {
    RLH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&well_stack_dma_kernel<T, kStkR, LD, CHEB>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, kStkLdsBytes));
    attr_dma = true;
  }
  hipLaunchKernelGGL((well_stack_dma_kernel<T, kStkR, LD, CHEB>), dim3((unsigned)grid), dim3(1024), kStkLdsBytes,
                     ctx().stream, h->stk_meta, h->stk_member, h->stk_gsrc, h->stk_idx,
                     pat ? (const T *)h->stk_table : (const T *)h->stk_vals, pat, pat ? h->stk_dtab : nullptr, h->n_rows,
                     sched, sched_len, X, ldx, n_own, H, ldh, Y, ldy, (int)m, cheb);
  const uint16_t *dtab = h->stk_dtab;
  note_launch(!pat ? "stack dma vals idx cheb=%d" : dtab ? "stack dma pat dtab cheb=%d" : "stack dma pat idx cheb=%d",
              CHEB ? 1 : 0, 0, 0, 0, grid, sched_len);
  RLH_HIP(hipGetLastError());
  return 0;
}

template <typename T>
static int launch_stack(const rlh_csr *h, int part, int64_t m, const T *X, int64_t ldx, int64_t n_own, const T *H,
                        int64_t ldh, T *Y, int64_t ldy, bool dma, const ChebArgs<T> *cheb = nullptr) {
  Context &c = ctx();
  const int32_t *sched;
  int64_t sched_len;
  int grid;
  h->stk_launch.pick(part, &sched, &sched_len, &grid);
  if (grid == 0) return 0;
  constexpr bool cplx = std::is_same<T, c32>::value || std::is_same<T, c64>::value;
  if (dma) {
    constexpr int EPL = 16 / (int)sizeof(T);
    const int32_t *pat = sizeof(T) < 16 && env_int("RLH_SPMM_STACK_PAT", 1) != 0 ? h->stk_pat : nullptr;   // the value dictionary, where the handle has one
    RLH_REQUIRE(h->stk_gmax <= 80 * EPL, "rlh_spmm: a stack of %d staging groups", h->stk_gmax);   // (a slot holds 40 or 80 pieces)
    if (cheb) {
      if constexpr (sizeof(T) == 16)
        return launch_stack_dma<T, true>(h, pat, sched, sched_len, grid, m, X, ldx, n_own, H, ldh, Y, ldy, *cheb);
      else
        RLH_REQUIRE(false, "rlh_spmm_cheb: the stacked fused step exists for 16-byte elements only");
    }
    return launch_stack_dma<T, false>(h, pat, sched, sched_len, grid, m, X, ldx, n_own, H, ldh, Y, ldy, ChebArgs<T>{});
  }
  RLH_REQUIRE(part == 0 && H == nullptr, "rlh_spmm: the register-staged stack kernel takes the whole operator only");
  if constexpr (!cplx) {
    static bool attr = false;
    if (!attr) {
      RLH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&well_stack_kernel<T, kStkR>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 2 * kStkBufBytes));
      attr = true;
    }
    const int cps_cap = env_int("RLH_SPMM_CPS", 8);
    hipLaunchKernelGGL((well_stack_kernel<T, kStkR>), dim3((unsigned)grid), dim3(1024), 2 * kStkBufBytes, c.stream,
                       h->stk_meta, h->stk_member, h->stk_gsrc, h->stk_idx, (const T *)h->stk_vals, h->n_rows, sched,
                       sched_len, X, ldx, Y, ldy, (int)m, cps_cap < 1 ? 1 : cps_cap);
    note_launch("stack reg", 0, 0, 0, 0, grid, sched_len);
    RLH_HIP(hipGetLastError());
  }
  return 0;
}

template <typename T>
static int launch_well(const rlh_csr *h, int part, int64_t m, const T *X, int64_t ldx, int64_t n_own, const T *H,
                       int64_t ldh, T *Y, int64_t ldy, const ChebArgs<T> *cheb) {
  // (rows of more than 8 entries and the complex types use the interleaved layout, spmm_wide.inc)
  return launch_well_w<T, 8>(h, part, m, X, ldx, n_own, H, ldh, Y, ldy, cheb);
}

// Y = A X on the stacked layout where the handle has one and the call fits it: the whole operator on own columns with
// either kernel; with a halo block, or on the interior / boundary part of the rows (rlh_spmm_part), the LDS-DMA kernel,
// whose 16-byte pieces must then lie on one side of the own / halo boundary.
template <typename T>
static int stack_dispatch(rlh_csr *h, int part, int64_t m, const T *X, int64_t ldx, int64_t n_own, const T *H, int64_t ldh,
                          T *Y, int64_t ldy, bool *done, const ChebArgs<T> *cheb = nullptr) {
  constexpr bool cplx = std::is_same<T, c32>::value || std::is_same<T, c64>::value;
  constexpr int EPL = 16 / (int)sizeof(T);
  *done = false;
  if (h->stk_blocks == 0 || env_int("RLH_SPMM_STACK", 1) == 0) return 0;
  bool dma = h->stk_gmax * 64 * (int)sizeof(T) <= StkRing<T>::SLOT && (cplx || env_int("RLH_SPMM_STACK_DMA", 1) != 0);
  if (cplx && !dma) return 0;
  // float32, whole operator on own columns: the register-staged kernel (0.66 against 0.71 ms on lap3d 215^3 m = 32 -- with
  // one or two DMA pieces per wave the waits, which do not count the interleaved stores as allowed, keep too little in
  // flight; RLH_SPMM_STACK_DMA=2 takes the DMA kernel regardless)
  if (sizeof(T) == 4 && !cplx && part == 0 && H == nullptr && env_int("RLH_SPMM_STACK_DMA", 1) < 2) dma = false;
  // the last staging group may reach up to 7 columns past n_cols: inside the block's leading dimension, or not this way
  if (h->stk_overhang > 0 && (H != nullptr && n_own != h->n_cols ? ldh < h->n_cols - n_own + h->stk_overhang
                                                                  : ldx < h->n_cols + h->stk_overhang)) {
    static bool said = false;
    if (!said && env_int("RLH_SPMM_VERBOSE", 0) != 0) {
      said = true;
      fprintf(stderr, "rlh_spmm_part: stacks not used (overhang %d, ldh %lld, ldx %lld, n_cols %lld, n_own %lld)\n", h->stk_overhang,
              (long long)ldh, (long long)ldx, (long long)h->n_cols, (long long)n_own);
    }
    return 0;
  }
  if (part != 0 || H != nullptr) {
    if (!dma || (H != nullptr && n_own != h->n_cols && !(h->stk_aligned && n_own % EPL == 0))) {
      static bool said = false;
      if (!said && env_int("RLH_SPMM_VERBOSE", 0) != 0) {
        said = true;
        fprintf(stderr, "rlh_spmm_part: stacks not used (dma %d, aligned %d, n_own %lld, gmax %d, overhang %d)\n", (int)dma,
                h->stk_aligned, (long long)n_own, h->stk_gmax, h->stk_overhang);
      }
      return 0;
    }
    if (part != 0)
      if (int rc = h->stk_launch.split(n_own)) return rc;
  }
  if (cheb && !dma) return 0;
  *done = true;
  return launch_stack<T>(h, part, m, X, ldx, n_own, H, ldh, Y, ldy, dma, cheb);
}

template <int DT>
static int spmm_impl(rlh_csr *h, int part, int64_t m, const void *X_, int64_t ldx, int64_t n_own, const void *H_,
                     int64_t ldh, void *Y_, int64_t ldy, const void *B_ = nullptr, int64_t ldb = 0, double cy = 0.0,
                     double cp = 0.0, double cb = 0.0) {
  using T = typename DType<DT>::T;
  constexpr int JTMAX = DType<DT>::cplx ? 16 : 32;
  const T *X = (const T *)X_, *H = (const T *)H_;
  T *Y = (T *)Y_;
  ChebArgs<T> cargs{(const T *)B_, ldb, cy, cp, cb};
  const ChebArgs<T> *cheb = B_ ? &cargs : nullptr;
  if (cheb == nullptr && (DType<DT>::cplx || h->well_blocks > 0)) {     // (a complex operator: the stacks beside its other layout)
    bool done = false;
    const int rc = stack_dispatch<T>(h, part, m, X, ldx, n_own, H, ldh, Y, ldy, &done);
    if (rc || done) return rc;
  }
  // the fused Chebyshev step of a 16-byte operator on the same stacks (rows of at most 7 entries that store their diagonal)
  if (cheb != nullptr && sizeof(T) == 16 && env_int("RLH_SPMM_STACK_CHEB", 1) != 0) {
    bool done = false;
    if (h->stk_self) {
      const int rc = stack_dispatch<T>(h, part, m, X, ldx, n_own, H, ldh, Y, ldy, &done, cheb);
      if (rc || done) return rc;
    }
    {
      static bool said = false;
      if (!said && env_int("RLH_SPMM_VERBOSE", 0) != 0) {
        said = true;
        fprintf(stderr, "rlh_spmm_cheb: stacked fused step not used (stacks %lld, self %d, part %d, halo %d, n_own %lld, n_cols %lld, gmax %d, aligned %d)\n",
                (long long)h->stk_blocks, h->stk_self, part, H != nullptr, (long long)n_own, (long long)h->n_cols, h->stk_gmax, h->stk_aligned);
      }
    }
    // (RLH_SPMM_STACK_CHEB=2: the tests' way of knowing which kernel ran)
    RLH_REQUIRE(env_int("RLH_SPMM_STACK_CHEB", 1) < 2, "rlh_spmm_cheb: the stacked fused step does not take this operator or call");
  }
  if (h->wide_blocks > 0) {
    switch (DT) {
      case RLH_S: return wide_spmm_s(h, part, m, X_, ldx, n_own, H_, ldh, Y_, ldy, B_, ldb, cy, cp, cb);
      case RLH_D: return wide_spmm_d(h, part, m, X_, ldx, n_own, H_, ldh, Y_, ldy, B_, ldb, cy, cp, cb);
      case RLH_C: return wide_spmm_c(h, part, m, X_, ldx, n_own, H_, ldh, Y_, ldy, B_, ldb, cy, cp, cb);
      default:    return wide_spmm_z(h, part, m, X_, ldx, n_own, H_, ldh, Y_, ldy, B_, ldb, cy, cp, cb);
    }
  }
  if constexpr (!DType<DT>::cplx) {
    if (h->well_blocks > 0) {
      if (part != 0)
        if (int rc = h->well_launch.split(n_own)) return rc;
      return launch_well<T>(h, part, m, X, ldx, n_own, H, ldh, Y, ldy, cheb);
    }
  }
  if (part == 1) return 0;                    // sliced layout: everything happens in part 2
  const int jt_cap = env_int("RLH_SPMM_JT", 16);        // vectors per lane tile (tunable; 16 measured best at m = 32 fp64)
  if (m <= 4 || jt_cap <= 4) return launch_spmm<T, 4>(h, m, X, ldx, n_own, H, ldh, Y, ldy, cheb);
  if (m <= 8 || jt_cap <= 8) return launch_spmm<T, 8>(h, m, X, ldx, n_own, H, ldh, Y, ldy, cheb);
  if (m <= 16 || JTMAX == 16 || jt_cap <= 16 || cheb) return launch_spmm<T, 16>(h, m, X, ldx, n_own, H, ldh, Y, ldy, cheb);
  return launch_spmm<T, (JTMAX == 32 ? 32 : 16)>(h, m, X, ldx, n_own, H, ldh, Y, ldy, cheb);
}

template <typename T>
__global__ __launch_bounds__(256) void gather_rows_kernel(const int64_t *__restrict__ idx, int64_t nidx,
                                                          const T *__restrict__ X, int64_t ldx,
                                                          T *__restrict__ Out, int64_t ldo) {
  const T *x = X + (int64_t)blockIdx.y * ldx;
  T *o = Out + (int64_t)blockIdx.y * ldo;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nidx; i += stride) o[i] = x[idx[i]];
}

template <int DT>
static int gather_rows_impl(int64_t nidx, const int64_t *d_idx, int64_t m, const void *X, int64_t ldx, void *Out,
                            int64_t ldo) {
  using T = typename DType<DT>::T;
  Context &c = ctx();
  int64_t nb = (nidx + 255) / 256;
  const int64_t cap = ((int64_t)c.num_cu * 8 + m - 1) / m;
  if (nb > cap) nb = cap;
  if (nb < 1) nb = 1;
  return for_col_panels(m, [&](int64_t j0, int64_t mp) {
    hipLaunchKernelGGL((gather_rows_kernel<T>), dim3((unsigned)nb, (unsigned)mp), dim3(256), 0, c.stream, d_idx, nidx,
                       (const T *)X + j0 * ldx, ldx, (T *)Out + j0 * ldo, ldo);
    RLH_HIP(hipGetLastError());
    return 0;
  });
}

}  // namespace rlh

using namespace rlh;

extern "C" {

int rlh_csr_destroy(rlh_csr_t h) {
  if (!h) return 0;
  if (ctx().ready) (void)hipStreamSynchronize(ctx().stream);
  delete h;
  return 0;
}

int rlh_csr_info(rlh_csr_t h, int64_t *n_rows, int64_t *n_cols, int64_t *nnz, int64_t *device_bytes) {
  RLH_REQUIRE(h != nullptr, "rlh_csr_info: null handle");
  if (n_rows) *n_rows = h->n_rows;
  if (n_cols) *n_cols = h->n_cols;
  if (nnz) *nnz = h->nnz;
  if (device_bytes) *device_bytes = h->device_bytes;
  return 0;
}

}  // extern "C"
// the layout conditions of the bfloat16 Chebyshev step: ONE definition for the launch and for rlh_csr_bf16_ready
// (the 1024-row windowed layout stages by 16-byte pieces only: every group inside the column range; the interleaved layout
// has an element-wise staging for the others, so any float32 handle in it is taken)
static inline bool bf16_layout_ok(const rlh_csr *h) {
  return h->dtype == RLH_S && ((h->well_blocks > 0 && h->stage_inbounds) || h->wide_blocks > 0);
}
static inline bool bf16_halo_ok(const rlh_csr *h, int64_t n_own, int64_t ldh) {
  return h->stage_aligned && n_own % 8 == 0 && ldh % 8 == 0;
}
// the bfloat16 Chebyshev step on the stacks, VPS vectors per step (the caller has checked that the stacks take the call)
template <int VPS>
static int launch_stack_cheb_bf16(rlh_csr *h, int part, int64_t m, const unsigned short *Y, int64_t ldy, int64_t n_own,
                                  const unsigned short *H, int64_t ldh, unsigned short *P, int64_t ldp,
                                  const unsigned short *B, int64_t ldb, float cy, float cp, float cb) {
  if (part != 0)
    if (int rc = h->stk_launch.split(n_own)) return rc;
  const int32_t *sched;
  int64_t sched_len;
  int grid;
  h->stk_launch.pick(part, &sched, &sched_len, &grid);
  if (grid == 0) return 0;
  constexpr int lds = kBfRingBytes + 16 * kBfOperandBytes;
  const int32_t *pat = env_int("RLH_SPMM_STACK_PAT", 1) != 0 ? h->stk_pat : nullptr;
  static bool attr = false;
  if (!attr) {
    RLH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&well_stack_cheb_bf16_kernel<kStkR, VPS>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    attr = true;
  }
  hipLaunchKernelGGL((well_stack_cheb_bf16_kernel<kStkR, VPS>), dim3((unsigned)grid), dim3(1024), lds, ctx().stream,
                     h->stk_meta, h->stk_member, h->stk_gsrc, h->stk_idx,
                     pat ? (const float *)h->stk_table : (const float *)h->stk_vals, pat, pat ? h->stk_dtab : nullptr,
                     h->n_rows, sched, sched_len, Y, ldy, n_own, H, ldh, P, ldp, B, ldb, (int)m, cy, cp, cb);
  const uint16_t *dtab = h->stk_dtab;
  note_launch(!pat ? "stack bf16 vps=%d vals idx" : dtab ? "stack bf16 vps=%d pat dtab" : "stack bf16 vps=%d pat idx", VPS, 0, 0, 0,
              grid, sched_len);
  RLH_HIP(hipGetLastError());
  return 0;
}
extern "C" {

int rlh_spmm_last_launch(char *buf, int64_t len) {
  RLH_REQUIRE(buf != nullptr && len > 0, "rlh_spmm_last_launch: no buffer");
  const LaunchNote &n = launch_note();
  if (n.what == nullptr) {
    snprintf(buf, (size_t)len, "none");
    return 0;
  }
  char kernel[96];
  snprintf(kernel, sizeof kernel, n.what, n.v[0], n.v[1], n.v[2], n.v[3]);
  snprintf(buf, (size_t)len, "%s grid=%d len=%lld", kernel, n.grid, (long long)n.len);
  return 0;
}

int rlh_csr_layout(rlh_csr_t h, int *layout, int64_t *stored, double *staged_per_slot) {
  RLH_REQUIRE(h != nullptr, "rlh_csr_layout: null handle");
  if (layout) *layout = h->wide_blocks > 0 ? 2 : (h->well_blocks > 0 ? 1 : 0);
  if (stored) *stored = h->padded;
  if (staged_per_slot) *staged_per_slot = h->stage_ratio;
  return 0;
}

int rlh_csr_stacks(rlh_csr_t h, int64_t *stacks, double *staged_per_row, double *staged_per_row_stacked) {
  RLH_REQUIRE(h != nullptr, "rlh_csr_stacks: null handle");
  if (stacks) *stacks = h->stk_blocks;
  if (staged_per_row) *staged_per_row = h->well_staged;
  if (staged_per_row_stacked) *staged_per_row_stacked = h->stk_staged;
  return 0;
}

int rlh_csr_bf16_ready(rlh_csr_t h, int64_t n_own, int64_t ldh, int *ok) {
  RLH_REQUIRE(h != nullptr && ok != nullptr, "rlh_csr_bf16_ready: null argument");
  *ok = bf16_layout_ok(h) && h->n_rows <= n_own && n_own <= h->n_cols && (n_own == h->n_cols || bf16_halo_ok(h, n_own, ldh));
  return 0;
}

int rlh_spmm_part(rlh_csr_t h, int part, int64_t m, const void *X, int64_t ldx, int64_t n_own, const void *H,
                  int64_t ldh, void *Y, int64_t ldy) {
  launch_note().what = nullptr;
  if (int rc = require_ready()) return rc;
  RLH_REQUIRE(h != nullptr, "rlh_spmm: null handle");
  RLH_REQUIRE(part >= 0 && part <= 2, "rlh_spmm: part must be 0 (all rows), 1 (interior) or 2 (boundary)");
  RLH_REQUIRE(m >= 0, "rlh_spmm: negative block size");
  if (m == 0 || h->n_rows == 0) return 0;
  RLH_REQUIRE(Y && (X || n_own == 0), "rlh_spmm: null block pointer");
  RLH_REQUIRE(n_own >= 0 && n_own <= h->n_cols, "rlh_spmm: n_own out of range");
  RLH_REQUIRE(n_own == h->n_cols || H, "rlh_spmm: halo block missing for columns >= n_own");
  RLH_REQUIRE(ldx >= n_own && ldy >= h->n_rows && (!H || ldh >= h->n_cols - n_own),
              "rlh_spmm: leading dimension smaller than the operator size");
  RLH_REQUIRE(X != Y, "rlh_spmm: in-place application is not supported");
  switch (h->dtype) {
    case RLH_S: return spmm_impl<RLH_S>(h, part, m, X, ldx, n_own, H, ldh, Y, ldy);
    case RLH_D: return spmm_impl<RLH_D>(h, part, m, X, ldx, n_own, H, ldh, Y, ldy);
    case RLH_C: return spmm_impl<RLH_C>(h, part, m, X, ldx, n_own, H, ldh, Y, ldy);
    case RLH_Z: return spmm_impl<RLH_Z>(h, part, m, X, ldx, n_own, H, ldh, Y, ldy);
  }
  return 1;
}

int rlh_spmm(rlh_csr_t h, int64_t m, const void *X, int64_t ldx, int64_t n_own, const void *H, int64_t ldh, void *Y,
             int64_t ldy) {
  return rlh_spmm_part(h, 0, m, X, ldx, n_own, H, ldh, Y, ldy);
}

int rlh_spmm_cheb_part(rlh_csr_t h, int part, int64_t m, const void *Y, int64_t ldy, int64_t n_own, const void *H,
                       int64_t ldh, void *P, int64_t ldp, const void *B, int64_t ldb, double cy, double cp, double cb) {
  launch_note().what = nullptr;
  if (int rc = require_ready()) return rc;
  RLH_REQUIRE(h != nullptr, "rlh_spmm_cheb: null handle");
  RLH_REQUIRE(part >= 0 && part <= 2, "rlh_spmm_cheb: part must be 0 (all rows), 1 (interior) or 2 (boundary)");
  RLH_REQUIRE(m >= 0, "rlh_spmm_cheb: negative block size");
  if (m == 0 || h->n_rows == 0) return 0;
  RLH_REQUIRE(Y && P && B, "rlh_spmm_cheb: null block pointer");
  RLH_REQUIRE(h->n_rows <= n_own && n_own <= h->n_cols, "rlh_spmm_cheb: the operator block must be square in its own rows");
  RLH_REQUIRE(n_own == h->n_cols || H, "rlh_spmm_cheb: halo block missing for columns >= n_own");
  RLH_REQUIRE(ldy >= n_own && ldp >= h->n_rows && ldb >= h->n_rows && (!H || ldh >= h->n_cols - n_own),
              "rlh_spmm_cheb: leading dimension smaller than the operator size");
  RLH_REQUIRE(P != Y && P != B, "rlh_spmm_cheb: P is updated in place and must not alias Y or B");
  switch (h->dtype) {
    case RLH_S: return spmm_impl<RLH_S>(h, part, m, Y, ldy, n_own, H, ldh, P, ldp, B, ldb, cy, cp, cb);
    case RLH_D: return spmm_impl<RLH_D>(h, part, m, Y, ldy, n_own, H, ldh, P, ldp, B, ldb, cy, cp, cb);
    case RLH_C: return spmm_impl<RLH_C>(h, part, m, Y, ldy, n_own, H, ldh, P, ldp, B, ldb, cy, cp, cb);
    case RLH_Z: return spmm_impl<RLH_Z>(h, part, m, Y, ldy, n_own, H, ldh, P, ldp, B, ldb, cy, cp, cb);
  }
  return 1;
}

int rlh_spmm_cheb(rlh_csr_t h, int64_t m, const void *Y, int64_t ldy, int64_t n_own, const void *H, int64_t ldh,
                  void *P, int64_t ldp, const void *B, int64_t ldb, double cy, double cp, double cb) {
  return rlh_spmm_cheb_part(h, 0, m, Y, ldy, n_own, H, ldh, P, ldp, B, ldb, cy, cp, cb);
}

int rlh_spmm_cheb_bf16_part(rlh_csr_t h, int part, int64_t m, const void *Y16, int64_t ldy, int64_t n_own,
                            const void *H16, int64_t ldh, void *P16, int64_t ldp, const void *B16, int64_t ldb,
                            double cy, double cp, double cb) {
  launch_note().what = nullptr;
  if (int rc = require_ready()) return rc;
  RLH_REQUIRE(h != nullptr, "rlh_spmm_cheb_bf16: null handle");
  RLH_REQUIRE(part >= 0 && part <= 2, "rlh_spmm_cheb_bf16: part must be 0 (all rows), 1 (interior) or 2 (boundary)");
  RLH_REQUIRE(m >= 0, "rlh_spmm_cheb_bf16: negative block size");
  if (m == 0 || h->n_rows == 0) return 0;
  RLH_REQUIRE(bf16_layout_ok(h),
              "rlh_spmm_cheb_bf16: needs a float32 operator in the 256-row interleaved layout or in the 1024-row windowed layout "
              "(rows of at most 8 entries) with every staging group inside the column range; the sliced layout is not taken");
  RLH_REQUIRE(h->n_rows <= n_own && n_own <= h->n_cols, "rlh_spmm_cheb_bf16: the operator block must be square in its own rows");
  RLH_REQUIRE(n_own == h->n_cols || (H16 && bf16_halo_ok(h, n_own, ldh) && ((uintptr_t)H16 % 16) == 0),
              "rlh_spmm_cheb_bf16: a halo block needs n_own and ldh to be multiples of 8, a 16-byte aligned block "
              "and staging groups on multiples of 8 columns");
  RLH_REQUIRE(Y16 && P16 && B16 && P16 != Y16 && P16 != B16, "rlh_spmm_cheb_bf16: bad block pointers");
  RLH_REQUIRE(ldy >= n_own && ldp >= h->n_rows && ldb >= h->n_rows && ldy % 8 == 0 && ldp % 8 == 0 && ldb % 8 == 0 &&
                  ((uintptr_t)Y16 % 16) == 0 && ((uintptr_t)P16 % 16) == 0 && ((uintptr_t)B16 % 16) == 0,
              "rlh_spmm_cheb_bf16: blocks must be 16-byte aligned with leading dimensions that are multiples of 8");
  if (h->wide_blocks > 0) return wide_cheb_bf16(h, part, m, Y16, ldy, n_own, H16, ldh, P16, ldp, B16, ldb, cy, cp, cb);
  Context &c = ctx();
  const unsigned short *Y = (const unsigned short *)Y16, *B = (const unsigned short *)B16;
  const unsigned short *H = H16 ? (const unsigned short *)H16 : Y;
  unsigned short *P = (unsigned short *)P16;
  // the stacked layout (8 elements per 16-byte piece: groups on multiples of 8 columns, images of at most 128 groups)
  if (h->stk_blocks > 0 && h->stk_aligned && h->stk_gmax <= kBfImageBytes / 128 && env_int("RLH_SPMM_STACK", 1) != 0 &&
      env_int("RLH_SPMM_STACK_BF16", 1) != 0 &&
      (h->stk_overhang == 0 || (H16 != nullptr && n_own != h->n_cols ? ldh >= h->n_cols - n_own + h->stk_overhang
                                                                      : ldy >= h->n_cols + h->stk_overhang))) {
    if (env_int("RLH_SPMM_BF16_VPS", 2) >= 2)
      return launch_stack_cheb_bf16<2>(h, part, m, Y, ldy, n_own, H, ldh, P, ldp, B, ldb, (float)cy, (float)cp, (float)cb);
    return launch_stack_cheb_bf16<1>(h, part, m, Y, ldy, n_own, H, ldh, P, ldp, B, ldb, (float)cy, (float)cp, (float)cb);
  }
  if (part != 0)
    if (int rc = h->well_launch.split(n_own)) return rc;
  const int32_t *sched;
  int64_t sched_len;
  int nb;
  h->well_launch.pick(part, &sched, &sched_len, &nb);
  if (nb == 0) return 0;
#define RLH_BF_LAUNCH(W)                                                                                          \
  hipLaunchKernelGGL((well_cheb_bf16_kernel<W>), dim3((unsigned)nb), dim3(1024), 0, c.stream, h->well_meta,       \
                     h->well_gsrc, h->well_idx, (const float *)h->well_vals, h->n_rows, sched, sched_len, Y, ldy, \
                     n_own, H, ldh, P, ldp, B, ldb, (int)m, (float)cy, (float)cp, (float)cb)
  RLH_BF_LAUNCH(8);
#undef RLH_BF_LAUNCH
  note_launch("well bf16", 0, 0, 0, 0, nb, sched_len);
  RLH_HIP(hipGetLastError());
  return 0;
}

int rlh_spmm_cheb_bf16(rlh_csr_t h, int64_t m, const void *Y16, int64_t ldy, void *P16, int64_t ldp, const void *B16,
                       int64_t ldb, double cy, double cp, double cb) {
  RLH_REQUIRE(h != nullptr, "rlh_spmm_cheb_bf16: null handle");
  RLH_REQUIRE(h->n_rows == h->n_cols, "rlh_spmm_cheb_bf16: needs a square float32 operator (a row shard goes through "
                                      "rlh_spmm_cheb_bf16_part)");
  return rlh_spmm_cheb_bf16_part(h, 0, m, Y16, ldy, h->n_cols, nullptr, 0, P16, ldp, B16, ldb, cy, cp, cb);
}

int rlh_gather_rows_bf16(int64_t nidx, const int64_t *d_idx, int64_t m, const void *X16, int64_t ldx, void *Out16,
                         int64_t ldo) {
  if (int rc = require_ready()) return rc;
  RLH_REQUIRE(nidx >= 0 && m >= 0, "rlh_gather_rows_bf16: negative size");
  if (nidx == 0 || m == 0) return 0;
  RLH_REQUIRE(d_idx && X16 && Out16 && ldo >= nidx, "rlh_gather_rows_bf16: bad arguments");
  Context &c = ctx();
  int64_t nb = (nidx + 255) / 256;
  const int64_t cap = ((int64_t)c.num_cu * 8 + m - 1) / m;
  if (nb > cap) nb = cap;
  if (nb < 1) nb = 1;
  return for_col_panels(m, [&](int64_t j0, int64_t mp) {
    hipLaunchKernelGGL((gather_rows_kernel<unsigned short>), dim3((unsigned)nb, (unsigned)mp), dim3(256), 0, c.stream,
                       d_idx, nidx, (const unsigned short *)X16 + j0 * ldx, ldx, (unsigned short *)Out16 + j0 * ldo, ldo);
    RLH_HIP(hipGetLastError());
    return 0;
  });
}

int rlh_gather_rows(int dtype, int64_t nidx, const int64_t *d_idx, int64_t m, const void *X, int64_t ldx, void *Out,
                    int64_t ldo) {
  if (int rc = require_ready()) return rc;
  RLH_REQUIRE(dtype_valid(dtype), "rlh_gather_rows: unknown dtype %d", dtype);
  RLH_REQUIRE(nidx >= 0 && m >= 0, "rlh_gather_rows: negative size");
  if (nidx == 0 || m == 0) return 0;
  RLH_REQUIRE(d_idx && X && Out, "rlh_gather_rows: null pointer");
  RLH_REQUIRE(ldo >= nidx, "rlh_gather_rows: output leading dimension smaller than the index count");
  switch (dtype) {
    case RLH_S: return gather_rows_impl<RLH_S>(nidx, d_idx, m, X, ldx, Out, ldo);
    case RLH_D: return gather_rows_impl<RLH_D>(nidx, d_idx, m, X, ldx, Out, ldo);
    case RLH_C: return gather_rows_impl<RLH_C>(nidx, d_idx, m, X, ldx, Out, ldo);
    case RLH_Z: return gather_rows_impl<RLH_Z>(nidx, d_idx, m, X, ldx, Out, ldo);
  }
  return 1;
}

}  // extern "C"
