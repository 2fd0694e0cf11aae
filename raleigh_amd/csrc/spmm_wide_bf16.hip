// K13, interleaved windowed layout: the fused Chebyshev step on bfloat16 work blocks,
//   p <- bf16_rne(cy y + cp p + cb (b - A y)),
// against a float32 handle as spmm_wide_build.hip / spmm_build_device.hip leave it (wide_meta, wide_gsrc, wide_idx,
// wide_vals, the schedules of wide_sched; rows per thread wide_k = 1 or 2).  Same semantics as well_cheb_bf16_kernel
// (spmm.hip): y, p, b and the halo block are column-major bfloat16, the matrix values are float32, t = A y is
// accumulated in float32 and the update is rounded once, to nearest even; y and b are not written, nor are rows at or
// beyond n_rows or vectors at or beyond m.
//
// The structure is that of wide_spmm_kernel (spmm_wide.inc): one workgroup per block of 256 rows taken from the
// schedule, the group list fetched one block ahead, the entries streamed through registers in chunks of 8.  What
// differs is the element size of everything but the matrix:
//  * the staged image [column][vector] holds 2-byte elements: a 16-byte piece is 8 columns of one vector on the
//    global side and 8 vectors of one column in the LDS; the column stride is NV * 2 + 16 bytes made an odd number of
//    16-byte slots, so that the ds_read_b128 of lanes on consecutive columns fall on different slots of the 256-byte
//    bank row (strides 48, 48, 80 bytes for NV = 8, 16, 32);
//  * staging: a lane loads the 8-column piece of 8 vectors (8 loads of 16 bytes), transposes the 8 x 8 half-words in
//    registers and writes 8 ds_write_b128 (one per column).  Work items are (piece, block of 8 vectors) with the
//    block of vectors running fastest over the lanes: the eight columns of a piece are 8 S bytes apart, a multiple
//    of the 128 bytes over which writes are banked, so lanes on different pieces collide and only the lanes on the
//    NV / 8 vector blocks of one piece do not (the float kernel's 4-column pieces collide 4-way at twice the writes);
//  * multiply: an entry reads its NV staged values with NV / 8 ds_read_b128 and widens them in registers (a shift
//    or a mask per value); accumulators and matrix values are float32;
//  * store: the thread's own row of y, p, b is read as bfloat16 -- requested together with the staging loads, so a
//    pass exposes one memory latency, not two -- and p written as bfloat16 (row pairs: as one 32-bit word per vector).
// Nothing here waits on another workgroup; no atomics.
#include <type_traits>

#include "spmm.h"

namespace rlh {

struct WideBfArgs {
  const WideMeta *meta;
  const int32_t *gsrc;
  const rlh_u32x4e *idx;         // [chunk][row]: 8 positions
  const rlh_u32x4e *vals;        // [chunk][piece][row]: float32
  int64_t n_rows, n_cols;
  const int32_t *sched;
  int64_t sched_len;
  const unsigned short *Y; int64_t ldy;
  int64_t n_own;
  const unsigned short *H; int64_t ldh;
  unsigned short *P; int64_t ldp;
  const unsigned short *B; int64_t ldb;
  int m;
  int vec;                       // 16-byte staging loads allowed (groups in range, pieces on one side of n_own)
  float cy, cp, cb;
};

typedef unsigned rlh_u32x4h __attribute__((ext_vector_type(4), aligned(2)));   // a 16-byte piece of bfloat16 on any column

constexpr int wide_bf16_stride(int nv) { return (((nv * 2 + 16) / 16) & 1) ? nv * 2 + 16 : nv * 2 + 32; }

// NV: vectors per pass (8, 16, 32).  K: rows per thread (the handle's wide_k).  VS: sets of 256 / K threads that work on
// the same rows and different NV / VS of the vectors (8 or 16 per thread).
template <int NV, int VS, int K>
__global__ __launch_bounds__(256 / K * VS) void wide_cheb_bf16_kernel(const WideBfArgs a) {
  constexpr int EPL = 8;                          // elements per 16-byte piece
  constexpr int VP = 2;                           // 16-byte value pieces per chunk of 8 entries (float32)
  constexpr int S = wide_bf16_stride(NV);         // bytes per staged column
  constexpr int GBN = NV / EPL;                   // blocks of 8 vectors per pass
  constexpr int TPS = kWideRows / K;              // threads per set of vectors (= row groups of a block)
  constexpr int NT = TPS * VS;                    // threads
  constexpr int NVT = NV / VS;                    // vectors (accumulators) per thread and row
  constexpr int NVGT = NVT / EPL;                 // 16-byte pieces a thread reads per entry
  constexpr bool DEEP = K == 1;                   // entry chunks in flight: three, one for the row pairs (as the float kernel)
  static_assert(NV % EPL == 0 && NVT % EPL == 0 && (GBN & (GBN - 1)) == 0, "vectors per thread come in whole 16-byte pieces");
  extern __shared__ __attribute__((aligned(16))) char lds[];
  char *img = lds + 2 * kWideHeader;              // two group lists (this block's, the next block's) in front
  const int tid = threadIdx.x;
  const int rtid = tid & (TPS - 1);               // row group of the block
  const int vsel = __builtin_amdgcn_readfirstlane(tid / TPS);         // which part of the vectors (wave-uniform)
  const unsigned short *Hs = a.H ? a.H - a.n_own : a.Y;               // halo row of column c: Hs[c]
  const int last_col = (int)(a.n_cols - 1);
  const int m = a.m;

  struct Ent { rlh_u32x4e v[K * VP]; rlh_u32x4e p; };
  typedef typename std::conditional<K == 2, unsigned, unsigned short>::type Own;     // a thread's rows of one vector

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
      // the thread's own elements of y, p, b are requested here as well, so that the store does not expose a second
      // memory latency per pass: from clamped, always valid addresses (no branch around the loads); a row pair is one
      // aligned 32-bit word of a block (rows 2 r, 2 r + 1; leading dimensions are multiples of 8)
      const int nmine = nvp - vsel * NVT;                // vectors of this pass that are this thread's (may be <= 0)
      const int64_t jt = j0 + vsel * NVT;
      const bool whole = row + K - 1 < a.n_rows;         // every row of the thread's group exists
      Own yv[NVT], pv[NVT], bv[NVT];
      {
        const int64_t rowc = whole ? row : 0;
#pragma unroll
        for (int v = 0; v < NVT; ++v) {
          const int64_t jc = jt + v < m ? jt + v : m - 1;
          yv[v] = *reinterpret_cast<const Own *>(a.Y + rowc + jc * a.ldy);
          pv[v] = *reinterpret_cast<const Own *>(a.P + rowc + jc * a.ldp);
          bv[v] = *reinterpret_cast<const Own *>(a.B + rowc + jc * a.ldb);
        }
      }
      // ---- stage the windows of vectors j0 .. j0 + nvp - 1
      if (a.vec) {
        // Work item w = (piece of 8 columns, block gb of 8 vectors), gb fastest; unit s_ = items s_ NT .. + NT - 1, in
        // two register sets: the loads of unit s_ + 1 are issued before the LDS writes of unit s_ wait for theirs.
        // Items past the last repeat it (the same bytes to the same address), vectors past the last repeat the last.
        const int items = (F / EPL) * GBN;
        const int units = (items + NT - 1) / NT;
        rlh_u32x4e ra[EPL], rb[EPL];
        auto unit_load = [&](rlh_u32x4e (&r)[EPL], int s_) {
          int w = tid + s_ * NT;
          w = w < items ? w : items - 1;
          const int c = (w / GBN) * EPL, gb = w & (GBN - 1);
          const int col = gcol[c >> kWideGroupShift] + (c & (kWideGroup - 1));
          const bool own = col < a.n_own;
          const unsigned short *src = (own ? a.Y : Hs) + col;
          const int64_t ld = own ? a.ldy : a.ldh;
#pragma unroll
          for (int u = 0; u < EPL; ++u) {
            int j = j0 + gb * EPL + u;
            j = j < m ? j : m - 1;
            r[u] = *reinterpret_cast<const rlh_u32x4h *>(src + (int64_t)j * ld);
          }
        };
        auto unit_write = [&](const rlh_u32x4e (&r)[EPL], int s_) {
          int w = tid + s_ * NT;
          w = w < items ? w : items - 1;
          const int c = (w / GBN) * EPL, gb = w & (GBN - 1);
          char *dst = img + (unsigned)c * (unsigned)S + gb * 16;
#pragma unroll
          for (int k = 0; k < EPL; ++k) {           // column c + k: vectors 8 gb .. 8 gb + 7, two per word
            rlh_u32x4e out;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
              const unsigned lo = r[2 * d][k >> 1], hi = r[2 * d + 1][k >> 1];
              out[d] = (k & 1) ? ((lo >> 16) | (hi & 0xffff0000u)) : ((lo & 0xffffu) | (hi << 16));
            }
            *reinterpret_cast<rlh_u32x4e *>(dst + k * S) = out;
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
            const unsigned short val = col < a.n_own ? a.Y[col + j * a.ldy] : Hs[col + j * a.ldh];
            *reinterpret_cast<unsigned short *>(img + (unsigned)c * (unsigned)S + v * 2) = val;
          }
        }
      }
      __syncthreads();
      // ---- multiply: entries in chunks of 8, four register sets
      float acc[K][NVT];
#pragma unroll
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int v = 0; v < NVT; ++v) acc[k][v] = 0.f;
      const char *imgv = img + vsel * (NVT * 2);         // this thread's part of every image row
      auto compute = [&](const Ent &e) {
        union { rlh_u32x4e u[K * VP]; float t[K * 8]; } vv;
#pragma unroll
        for (int k = 0; k < K * VP; ++k) vv.u[k] = e.v[k];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          const unsigned w = e.p[t >> 1];
          const unsigned px = (t & 1) ? (w >> 16) : (w & 0xffffu);
          const char *xa = imgv + px * (unsigned)S;
#pragma unroll
          for (int g = 0; g < NVGT; ++g) {
            const rlh_u32x4e x = *reinterpret_cast<const rlh_u32x4e *>(xa + g * 16);
#pragma unroll
            for (int d = 0; d < 4; ++d) {
              const float lo = __uint_as_float(x[d] << 16), hi = __uint_as_float(x[d] & 0xffff0000u);
#pragma unroll
              for (int k = 0; k < K; ++k) {
                acc[k][g * EPL + 2 * d] = fmaf(vv.t[k * 8 + t], lo, acc[k][g * EPL + 2 * d]);
                acc[k][g * EPL + 2 * d + 1] = fmaf(vv.t[k * 8 + t], hi, acc[k][g * EPL + 2 * d + 1]);
              }
            }
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
      if (whole) {
#pragma unroll
        for (int v = 0; v < NVT; ++v)
          if (v < nmine) {
            if constexpr (K == 2) {
              const unsigned lo = f32_to_bf16(cheb_update(a.cy, __uint_as_float(yv[v] << 16), a.cp, __uint_as_float(pv[v] << 16),
                                                          a.cb, __uint_as_float(bv[v] << 16), acc[0][v]));
              const unsigned hi = f32_to_bf16(cheb_update(a.cy, __uint_as_float(yv[v] & 0xffff0000u), a.cp,
                                                          __uint_as_float(pv[v] & 0xffff0000u), a.cb,
                                                          __uint_as_float(bv[v] & 0xffff0000u), acc[K - 1][v]));
              *reinterpret_cast<unsigned *>(a.P + row + (jt + v) * a.ldp) = lo | (hi << 16);
            } else {
              a.P[row + (jt + v) * a.ldp] =
                  f32_to_bf16(cheb_update(a.cy, bf16_to_f32(yv[v]), a.cp, bf16_to_f32(pv[v]), a.cb, bf16_to_f32(bv[v]), acc[0][v]));
            }
          }
      } else if (K == 2 && row < a.n_rows) {
        // the last row of a matrix with an odd number of rows (one thread of the whole launch): it has no partner to
        // make a 32-bit word with, so yv / pv / bv (read from row 0 above) are not used and its elements are read here
        for (int v = 0; v < NVT && v < nmine; ++v) {
          unsigned short *pp = a.P + row + (jt + v) * a.ldp;
          *pp = f32_to_bf16(cheb_update(a.cy, bf16_to_f32(a.Y[row + (jt + v) * a.ldy]), a.cp, bf16_to_f32(*pp), a.cb,
                                        bf16_to_f32(a.B[row + (jt + v) * a.ldb]), acc[0][v]));
        }
      }
      __syncthreads();                            // the next pass / block overwrites the image
    }
    pos = pos_next;
    mt = mt_next;
    slot ^= 1;
  }
}

static inline size_t wide_bf16_lds(const rlh_csr *h, int nv) {
  return (size_t)2 * kWideHeader + (size_t)h->wide_gmax * kWideGroup * wide_bf16_stride(nv);
}

template <int NV, int VS, int K>
static int wide_bf16_launch(rlh_csr *h, int part, WideBfArgs &a) {
  Context &c = ctx();
  const size_t lds = wide_bf16_lds(h, NV);
  RLH_REQUIRE(lds <= (size_t)kWideLdsBytes, "rlh_spmm_cheb_bf16: the staged image of %d vectors does not fit the LDS", NV);
  // resident workgroups per CU: by registers (asked once per instantiation) and by the image size of this operator
  static int fit = 0;
  if (fit == 0) {
    const void *fn = reinterpret_cast<const void *>(&wide_cheb_bf16_kernel<NV, VS, K>);
    RLH_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kWideLdsBytes));
    hipFuncAttributes fa;
    RLH_HIP(hipFuncGetAttributes(&fa, fn));
    const int regs = (fa.numRegs + 7) / 8 * 8 > 0 ? (fa.numRegs + 7) / 8 * 8 : 8;
    fit = 512 / regs * K / VS;
    if (fit < 1) fit = 1;
  }
  int per_cu = fit;
  if (per_cu > (int)(kWideLdsBytes / lds)) per_cu = (int)(kWideLdsBytes / lds);
  if (per_cu > 4) per_cu = 4;
  const int cap = env_int("RLH_WIDE_WG_PER_CU", 0);            // tunable: 0 = as many as fit (at most 4)
  if (cap > 0 && per_cu > cap) per_cu = cap;
  int grid = 0;
  if (int rc = wide_sched(h, c.num_cu * per_cu, part, a.n_own, &a.sched, &a.sched_len, &grid)) return rc;
  if (a.sched_len == 0 || grid == 0) return 0;
  hipLaunchKernelGGL((wide_cheb_bf16_kernel<NV, VS, K>), dim3((unsigned)grid), dim3(256 / K * VS), lds, c.stream, a);
  note_launch(a.vec ? "wide bf16 nv=%d vs=%d k=%d vec" : "wide bf16 nv=%d vs=%d k=%d elem", NV, VS, K, 0, grid, a.sched_len);
  RLH_HIP(hipGetLastError());
  return 0;
}

int wide_cheb_bf16(rlh_csr *h, int part, int64_t m, const void *Y16, int64_t ldy, int64_t n_own, const void *H16,
                   int64_t ldh, void *P16, int64_t ldp, const void *B16, int64_t ldb, double cy, double cp, double cb) {
  // vectors per pass: the fewest passes whose image fits the LDS, then the smallest such NV (RLH_WIDE_NV forces one)
  const int cand[3] = {8, 16, 32};
  const int forced = env_int("RLH_WIDE_NV", 0);
  int nv = 0;
  int64_t best_passes = 0;
  for (int i = 0; i < 3; ++i) {
    if (wide_bf16_lds(h, cand[i]) > (size_t)kWideLdsBytes) continue;
    if (forced == cand[i]) { nv = forced; break; }
    const int64_t passes = (m + cand[i] - 1) / cand[i];
    if (nv == 0 || passes < best_passes) { nv = cand[i]; best_passes = passes; }
  }
  RLH_REQUIRE(nv > 0, "rlh_spmm_cheb_bf16: no staged image of this operator fits the LDS");
  WideBfArgs a;
  a.meta = h->wide_meta; a.gsrc = h->wide_gsrc;
  a.idx = (const rlh_u32x4e *)h->wide_idx; a.vals = (const rlh_u32x4e *)h->wide_vals;
  a.n_rows = h->n_rows; a.n_cols = h->n_cols; a.sched = nullptr; a.sched_len = 0;
  a.Y = (const unsigned short *)Y16; a.ldy = ldy; a.n_own = n_own;
  a.H = n_own < h->n_cols ? (const unsigned short *)H16 : nullptr; a.ldh = ldh;
  a.P = (unsigned short *)P16; a.ldp = ldp; a.B = (const unsigned short *)B16; a.ldb = ldb; a.m = (int)m;
  // 16-byte staging loads: every group inside the column range and, with a halo block, no piece across n_own (the
  // pieces of a vector may start on any column: the loads are declared 2-byte aligned)
  a.vec = (env_int("RLH_SPMM_VEC", 1) != 0 && h->stage_inbounds &&
           (a.H == nullptr || (h->stage_aligned && n_own % 8 == 0))) ? 1 : 0;
  a.cy = (float)cy; a.cp = (float)cp; a.cb = (float)cb;
  if (h->wide_k == 2) {                           // row pairs: eight vectors per thread and row, NV / 8 sets of 128 threads
    if (nv == 8) return wide_bf16_launch<8, 1, 2>(h, part, a);
    if (nv == 16) return wide_bf16_launch<16, 2, 2>(h, part, a);
    return wide_bf16_launch<32, 4, 2>(h, part, a);
  }
  if (nv == 8) return wide_bf16_launch<8, 1, 1>(h, part, a);
  // as the float launcher: two 256-thread workgroups per CU where two images fit, else 512 threads that split the
  // vectors of a pass (RLH_WIDE_VS forces 1 or 2)
  int vs = wide_bf16_lds(h, nv) <= (size_t)kWideLdsBytes / 2 ? 1 : 2;
  const int forced_vs = env_int("RLH_WIDE_VS", 0);
  if (forced_vs == 1 || forced_vs == 2) vs = forced_vs;
  if (nv == 16) return vs == 1 ? wide_bf16_launch<16, 1, 1>(h, part, a) : wide_bf16_launch<16, 2, 1>(h, part, a);
  return vs == 1 ? wide_bf16_launch<32, 1, 1>(h, part, a) : wide_bf16_launch<32, 2, 1>(h, part, a);
}

}  // namespace rlh
