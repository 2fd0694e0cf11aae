// K13: dense operator of 8-bit data, Y = A X - u c^T / Y = A^T X - u c^T for a row-major uint8 / int8 matrix A
// and float32 blocks X, Y (PCA and truncated SVD of images: the data are bytes at the source).
//
// Reference: the gemm of raleigh/algebra/dense_cublas.py:732-776 on the data converted to float32; here the
// data stay bytes in HBM (a quarter of the float32 footprint) and the products run on v_mfma_f32_32x32x16_bf16:
//  * every integer in [-128, 255] is exactly a bfloat16, so A is converted on its way into the LDS, exactly;
//  * every float32 x is exactly h + m + l with h = rn(x), m = rn(x - h), l = x - h - m three bfloat16 numbers
//    (3 x 8 significant bits, the exponent range of float32; exact unless l falls into the float32 denormals,
//    and a finite x within one bfloat16 ulp of the largest float32 has no such split): the X tile is split into
//    the three planes on its way into the LDS;
//  * a product of two bfloat16 numbers is exact in float32.
// A X = A h + A m + A l, three MFMAs per k-step on one float32 accumulator: the only error is that of the float32
// accumulation, as in the float32 kernel (dense.hip), at 3/16 of its matrix-core cycles.
//
// Conventions of dense_mfma2_f32_kernel: C^T tile of BN vectors x 128 output rows per 256-thread workgroup, the
// vector index on the MFMA row and the output row on the MFMA column (= lane & 31), so an accumulator register
// stores as 128-byte runs of the column-major Y; K split over gridDim.z into a workspace [split][vector][row]
// that bytes_splitk_reduce sums in a fixed order (no atomics: results are bit-identical between calls and
// handles); the rank-one epilogue in the tile store or in the reduce.  BK = 32, LDS double buffered (one barrier
// per K step, the global loads of step t + 1 in flight during the MFMAs of step t).
//
// LDS image, the same for A and for each plane of X: [row][32 bfloat16] = 64 bytes = four 16-byte chunks per row,
// row r stored at position r ^ ((r >> 4) & 3), its chunk c at c ^ ((r >> 2) & 3).  A fragment is one
// ds_read_b128 per operand tile and k-step of 16 (lane l: row l & 31, chunk 2 s + (l >> 5): k = 8 (l >> 5) + j,
// the operand map of the instruction); 16 consecutive rows with one chunk number fall into 16 different 16-byte
// slots of the 256-byte bank line.  ONE copy of A serves both products: for A^T the tile arrives as rows of A
// (128 consecutive bytes each) and every thread transposes a 4 x 4 block of bytes in registers, so that it
// too is written with 8-byte pieces of four consecutive k (rows 4 q + j of the image: the row permutation
// spreads them over the bank line).
#include <memory>
#include <type_traits>

#include "common.h"

struct rlh_bytes {
  int kind = 0;                        // RLH_BYTES_U8 / RLH_BYTES_I8
  int64_t rows = 0, cols = 0, lda = 0; // lda: bytes per row on the device, a multiple of 16
  int64_t ncp = 0;                     // cols rounded up to 16: what the kernels read of a row (zero padded when owned;
                                       // a borrowed matrix has ncp == cols, so nothing beyond its columns is read)
  const unsigned char *A = nullptr;     // what the kernels read: own.get(), or the caller's array (borrowed)
  rlh::DevBuf<unsigned char> own;      // the handle's padded copy: empty for a borrowed matrix
  rlh::DevBuf<char> work;              // split-K partial tiles
};

namespace rlh {
namespace {

struct BytesArgs {
  const unsigned char *A; int64_t lda, ncp;
  int64_t ny, nx;                      // Op is ny x nx
  const float *X; int64_t ldx;
  float *Y; int64_t ldy;
  int m;
  int x_vec;                           // X can be read in 16-byte pieces
  const float *r1_u, *r1_c;            // Y[i, v] -= u[i] * c[v] (u null: ones; c null: no term)
};

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float r1_apply(const BytesArgs &a, float y, int64_t i, int v) {
  if (!a.r1_c) return y;
  const float u = a.r1_u ? a.r1_u[i] : 1.f;
  return y - u * a.r1_c[v];
}

// two float32 rounded to nearest even bfloat16, packed (a in the low half)
__device__ __forceinline__ unsigned pack_rn(float a, float b) {
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a, b}, bf16x2));
}
__device__ __forceinline__ float lo_f(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float hi_f(unsigned w) { return __uint_as_float(w & 0xffff0000u); }

// byte j of the dword d as the bits of a float32 (exact; its upper 16 bits are the bfloat16)
template <bool SGN>
__device__ __forceinline__ unsigned byte_f(unsigned d, int j) {
  if (SGN) return __float_as_uint((float)(int)(signed char)((d >> (8 * j)) & 0xffu));
  return __float_as_uint((float)((d >> (8 * j)) & 0xffu));
}
// two exact bfloat16 from float32 bit patterns whose low 16 bits are zero
__device__ __forceinline__ unsigned pack_exact(unsigned lo_bits, unsigned hi_bits) { return (hi_bits & 0xffff0000u) | (lo_bits >> 16); }

__device__ __forceinline__ int lds_off(int r, int chunk) { return ((r ^ ((r >> 4) & 3)) << 6) + ((chunk ^ ((r >> 2) & 3)) << 4); }

template <int BN, bool A_KC, bool SGN>
__global__ __launch_bounds__(256, 2) void bytes_mfma_kernel(BytesArgs a, float *__restrict__ part, int64_t kchunk) {
  constexpr int MR = 128, BK = 32;              // (BK = 32 = two MFMA k-steps is built into the fragment reads)
  constexpr int WGN = (BN >= 64) ? 2 : 1;          // waves along the vector dimension
  constexpr int WGM = 4 / WGN;                     // waves along the output-row dimension
  constexpr int TN = BN / WGN / 32, TM = MR / WGM / 32;
  constexpr int UB = BN * BK / 4 / 256;            // pieces of four k of the X tile per thread and K step
  static_assert(TN >= 1 && TM >= 1 && UB >= 1, "tile split");

  __shared__ __attribute__((aligned(16))) char ldsA[2][MR * 64];
  __shared__ __attribute__((aligned(16))) char ldsX[2][3][BN * 64];

  const unsigned char *__restrict__ A = a.A;
  const float *__restrict__ X = a.X;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WGN, wn = wave % WGN;
  const int64_t i0 = (int64_t)blockIdx.x * MR;
  const int v0 = blockIdx.y * BN;
  const int64_t kbeg = (int64_t)blockIdx.z * kchunk;
  const int64_t kend = (kbeg + kchunk) < a.nx ? (kbeg + kchunk) : a.nx;

  u32x4 ra;                                        // 16 bytes of A per thread and K step
  f32x4 rb[UB];
  // EDGE false: a whole K step of a block that can be read in 16-byte pieces -- straight-line code, every load
  // unconditional (rows and vectors beyond the edge are clamped: computed, never stored).  EDGE true: the last K
  // step of a split and blocks at odd addresses, element by element.  (One body with the tests inside put a branch
  // around every load and the wait for it right behind.)
  auto load_tiles_as = [&](int64_t k0, auto edge) {
    constexpr bool EDGE = decltype(edge)::value;
    if constexpr (A_KC) {          // 16 consecutive k of one output row (the padding of a row holds zeros)
      const int r = tid >> 1;
      int64_t i = i0 + r;
      i = i < a.ny ? i : a.ny - 1;
      const int64_t k = k0 + (tid & 1) * 16;
      if constexpr (EDGE) {
        ra = u32x4{0u, 0u, 0u, 0u};
        if (k + 16 <= a.ncp) ra = *reinterpret_cast<const u32x4 *>(A + i * a.lda + k);
      } else {
        ra = *reinterpret_cast<const u32x4 *>(A + i * a.lda + k);
      }
    } else {                       // a 4 x 4 block: output rows iq .. iq + 3 at k = kq .. kq + 3
      const int kq = (tid >> 5) * 4;
      int64_t i = i0 + (tid & 31) * 4;
      i = i < a.ncp ? i : a.ncp - 4;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t k = k0 + kq + q;
        unsigned d = 0u;
        if (!EDGE || k < kend) d = *reinterpret_cast<const unsigned *>(A + k * a.lda + i);
        ra[q] = d;
      }
    }
#pragma unroll
    for (int q = 0; q < UB; ++q) {
      const int u = tid + q * 256;
      const int c = u >> 3;
      int vc = v0 + c;
      vc = vc < a.m ? vc : a.m - 1;
      const int64_t k = k0 + (u & 7) * 4;
      const float *p = X + (int64_t)vc * a.ldx + k;
      if constexpr (!EDGE) {
        rb[q] = *reinterpret_cast<const f32x4 *>(p);
      } else {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (k + e < kend) v[e] = p[e];
        rb[q] = v;
      }
    }
  };
  auto load_tiles = [&](int64_t k0) {              // (wave-uniform choice)
    if (a.x_vec && k0 + BK <= kend) load_tiles_as(k0, std::false_type{});
    else load_tiles_as(k0, std::true_type{});
  };
  auto store_tiles = [&](int buf) {
    char *la = ldsA[buf];
    if constexpr (A_KC) {
      const int r = tid >> 1, c0 = (tid & 1) * 2;
#pragma unroll
      for (int h = 0; h < 2; ++h) {                  // eight k each: one 16-byte chunk
        const unsigned d0 = ra[2 * h], d1 = ra[2 * h + 1];
        u32x4 w;
        w[0] = pack_exact(byte_f<SGN>(d0, 0), byte_f<SGN>(d0, 1));
        w[1] = pack_exact(byte_f<SGN>(d0, 2), byte_f<SGN>(d0, 3));
        w[2] = pack_exact(byte_f<SGN>(d1, 0), byte_f<SGN>(d1, 1));
        w[3] = pack_exact(byte_f<SGN>(d1, 2), byte_f<SGN>(d1, 3));
        *reinterpret_cast<u32x4 *>(la + lds_off(r, c0 + h)) = w;
      }
    } else {
      const int kq = (tid >> 5) * 4, iq = (tid & 31) * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {                  // image row iq + j: its four k from the four loaded dwords
        u32x2 w;
        w[0] = pack_exact(byte_f<SGN>(ra[0], j), byte_f<SGN>(ra[1], j));
        w[1] = pack_exact(byte_f<SGN>(ra[2], j), byte_f<SGN>(ra[3], j));
        *reinterpret_cast<u32x2 *>(la + lds_off(iq + j, kq >> 3) + ((kq >> 2) & 1) * 8) = w;
      }
    }
#pragma unroll
    for (int q = 0; q < UB; ++q) {
      const int u = tid + q * 256;
      const int c = u >> 3, kq = (u & 7) * 4;
      const f32x4 x = rb[q];
      u32x2 h, m, l;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const float x0 = x[2 * e], x1 = x[2 * e + 1];
        h[e] = pack_rn(x0, x1);
        const float r0 = x0 - lo_f(h[e]), r1 = x1 - hi_f(h[e]);       // exact
        m[e] = pack_rn(r0, r1);
        l[e] = pack_rn(r0 - lo_f(m[e]), r1 - hi_f(m[e]));             // exact differences of at most 8 bits
      }
      const int off = lds_off(c, kq >> 3) + ((kq >> 2) & 1) * 8;
      *reinterpret_cast<u32x2 *>(ldsX[buf][0] + off) = h;
      *reinterpret_cast<u32x2 *>(ldsX[buf][1] + off) = m;
      *reinterpret_cast<u32x2 *>(ldsX[buf][2] + off) = l;
    }
  };

  f32x16 acc[TN][TM];
#pragma unroll
  for (int tn = 0; tn < TN; ++tn)
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[tn][tm][r] = 0.f;

  const int fr = lane & 31, fh = lane >> 5;
  const int mrow0 = wm * (MR / WGM), vcol0 = wn * (BN / WGN);

  int buf = 0;
  if (kbeg < kend) {
    load_tiles(kbeg);
    store_tiles(0);
  }
  __syncthreads();
  for (int64_t k0 = kbeg; k0 < kend; k0 += BK) {
    const bool more = (k0 + BK < kend);
    if (more) load_tiles(k0 + BK);
    const char *la = ldsA[buf];
    // the fragments of both k-steps of 16 are read BEFORE the MFMAs (the scheduling barrier keeps them there: left
    // alone the compiler read each fragment right in front of the MFMA that takes it and waited for the LDS 12 times
    // per K step); the conversions of the next tile (store_tiles) may then be spread between the MFMAs
    bf16x8 fa[2][TM], fx[2][3][TN];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) fa[s][tm] = *reinterpret_cast<const bf16x8 *>(la + lds_off(mrow0 + tm * 32 + fr, 2 * s + fh));
#pragma unroll
      for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
          fx[s][p][tn] = *reinterpret_cast<const bf16x8 *>(ldsX[buf][p] + lds_off(vcol0 + tn * 32 + fr, 2 * s + fh));
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int p = 2; p >= 0; --p)                   // the small terms first
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
          for (int tm = 0; tm < TM; ++tm)
            acc[tn][tm] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fx[s][p][tn], fa[s][tm], acc[tn][tm], 0, 0, 0);
    if (more) store_tiles(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }
  // D[v][i]: col (lane & 31) = output row i, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5) = vector v
  float *__restrict__ out = part ? part + (int64_t)blockIdx.z * a.m * a.ny : a.Y;
  const int64_t ldo = part ? a.ny : a.ldy;
#pragma unroll
  for (int tn = 0; tn < TN; ++tn)
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int v = v0 + vcol0 + tn * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const int64_t i = i0 + mrow0 + tm * 32 + (lane & 31);
        if (v < a.m && i < a.ny) out[i + (int64_t)v * ldo] = part ? acc[tn][tm][r] : r1_apply(a, acc[tn][tm][r], i, v);
      }
}

// the K splits summed in a fixed order, the rank-one epilogue applied
__global__ __launch_bounds__(256) void bytes_splitk_reduce(const float *__restrict__ part, int splits, BytesArgs a) {
  const int v = blockIdx.y;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.ny; i += stride) {
    float s = part[(int64_t)v * a.ny + i];
    for (int z = 1; z < splits; ++z) s += part[((int64_t)z * a.m + v) * a.ny + i];
    a.Y[i + (int64_t)v * a.ldy] = r1_apply(a, s, i, v);
  }
}

// exact sums of squares of the rows: one wave per row, 64-bit integer accumulation (255^2 N exceeds 32 bits)
template <bool SGN>
__global__ __launch_bounds__(256) void bytes_row_sumsq_kernel(const unsigned char *__restrict__ A, int64_t rows, int64_t lda,
                                                              int64_t ncp, double *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const unsigned *__restrict__ p = reinterpret_cast<const unsigned *>(A + r * lda);
  unsigned long long s = 0;
  for (int64_t q = lane; q < ncp / 4; q += 64) {
    const unsigned d = p[q];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int b = SGN ? (int)(signed char)((d >> (8 * j)) & 0xffu) : (int)((d >> (8 * j)) & 0xffu);
      s += (unsigned)(b * b);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  if (lane == 0) out[r] = (double)s;              // below 2^53: exact
}

// largest modulus per workgroup (the padding holds zeros); the host takes the largest of them.  dwords = rows * rowdw,
// rowdw dwords of every row of lda bytes.
template <bool SGN>
__global__ __launch_bounds__(256) void bytes_absmax_kernel(const unsigned char *__restrict__ A, int64_t dwords, int64_t rowdw,
                                                           int64_t lda, int *__restrict__ out) {
  __shared__ int red[4];
  int mx = 0;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < dwords; q += (int64_t)gridDim.x * 256) {
    const int64_t r = q / rowdw;
    const unsigned d = *reinterpret_cast<const unsigned *>(A + r * lda + (q - r * rowdw) * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int b = SGN ? (int)(signed char)((d >> (8 * j)) & 0xffu) : (int)((d >> (8 * j)) & 0xffu);
      b = b < 0 ? -b : b;
      mx = b > mx ? b : mx;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int t = __shfl_down(mx, o, 64);
    mx = t > mx ? t : mx;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) mx = red[w] > mx ? red[w] : mx;
    out[blockIdx.x] = mx;
  }
}

// the padded copy of rlh_bytes_create made on the device: dst rows of lda bytes (a multiple of 16), four bytes per
// thread, the pad zero; src rows row_stride bytes apart, read byte by byte (any alignment)
__global__ __launch_bounds__(256) void bytes_pad_copy_kernel(unsigned char *__restrict__ dst, int64_t lda, const unsigned char *__restrict__ src,
                                                             int64_t row_stride, int64_t rows, int64_t cols) {
  const int64_t rowdw = lda / 4, dwords = rows * rowdw;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < dwords; q += (int64_t)gridDim.x * 256) {
    const int64_t r = q / rowdw, c0 = (q - r * rowdw) * 4;
    unsigned d = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (c0 + j < cols) d |= (unsigned)src[r * row_stride + c0 + j] << (8 * j);
    *reinterpret_cast<unsigned *>(dst + r * lda + c0) = d;
  }
}

template <int BN>
int launch_bytes(rlh_bytes *h, const BytesArgs &a, bool a_kc) {
  Context &c = ctx();
  constexpr int MR = 128;
  const int64_t bx = (a.ny + MR - 1) / MR, by = (a.m + BN - 1) / BN;
  // split K until every CU has a few workgroups (the M x m output alone gives too few), at least 512 k per split
  static const int target = env_int("RLH_BYTES_WG_PER_CU", 8);
  int64_t splits = ((int64_t)c.num_cu * target + bx * by - 1) / (bx * by);
  const int64_t max_by_k = (a.nx + 511) / 512;
  if (splits > max_by_k) splits = max_by_k;
  if (splits > 16) splits = 16;
  while (splits > 1 && (size_t)splits * a.m * a.ny * sizeof(float) > kWorkspaceBytes) --splits;
  if (splits < 1) splits = 1;
  int64_t kchunk = ((a.nx + splits - 1) / splits + 31) / 32 * 32;
  if (kchunk < 32) kchunk = 32;                  // (no columns at all: the rank-one term alone)
  splits = (a.nx + kchunk - 1) / kchunk;
  if (splits < 1) splits = 1;
  float *part = nullptr;
  if (splits > 1) {
    const int64_t need = splits * (int64_t)a.m * a.ny * (int64_t)sizeof(float);
    if (int rc = h->work.reserve((size_t)need)) return rc;      // grows once per larger product, then reused without allocation
    part = (float *)h->work;
  }
  const dim3 grid((unsigned)bx, (unsigned)by, (unsigned)splits);
  const bool sgn = h->kind == RLH_BYTES_I8;
  if (a_kc) {
    if (sgn) hipLaunchKernelGGL((bytes_mfma_kernel<BN, true, true>), grid, dim3(256), 0, c.stream, a, part, kchunk);
    else hipLaunchKernelGGL((bytes_mfma_kernel<BN, true, false>), grid, dim3(256), 0, c.stream, a, part, kchunk);
  } else {
    if (sgn) hipLaunchKernelGGL((bytes_mfma_kernel<BN, false, true>), grid, dim3(256), 0, c.stream, a, part, kchunk);
    else hipLaunchKernelGGL((bytes_mfma_kernel<BN, false, false>), grid, dim3(256), 0, c.stream, a, part, kchunk);
  }
  RLH_HIP(hipGetLastError());
  if (splits > 1) {
    int64_t nb = (a.ny + 255) / 256;
    if (nb > 64) nb = 64;
    hipLaunchKernelGGL(bytes_splitk_reduce, dim3((unsigned)nb, (unsigned)a.m), dim3(256), 0, c.stream, part, (int)splits, a);
    RLH_HIP(hipGetLastError());
  }
  return 0;
}

}  // namespace
}  // namespace rlh

using namespace rlh;

extern "C" int rlh_bytes_create(rlh_bytes_t *ph, int kind, int64_t n_rows, int64_t n_cols, const void *h_data,
                                int64_t row_stride) {
  if (int rc = require_ready()) return rc;
  RLH_REQUIRE(ph, "rlh_bytes_create: null handle pointer");
  *ph = nullptr;
  RLH_REQUIRE(kind == RLH_BYTES_U8 || kind == RLH_BYTES_I8, "rlh_bytes_create: kind must be 0 (uint8) or 1 (int8), got %d", kind);
  RLH_REQUIRE(n_rows >= 0 && n_cols >= 0, "rlh_bytes_create: negative size");
  RLH_REQUIRE(n_rows == 0 || n_cols == 0 || h_data, "rlh_bytes_create: null data");
  RLH_REQUIRE(row_stride >= n_cols, "rlh_bytes_create: row stride smaller than the number of columns");
  std::unique_ptr<rlh_bytes> h(new rlh_bytes());
  h->kind = kind;
  h->rows = n_rows;
  h->cols = n_cols;
  h->lda = (n_cols + 15) / 16 * 16;
  if (h->lda < 16) h->lda = 16;
  h->ncp = h->lda;
  if (int rc = h->own.alloc((size_t)((n_rows > 0 ? n_rows : 1) * h->lda))) return rc;
  h->A = h->own.get();
  if (h->lda != n_cols) RLH_HIP(hipMemset(h->own, 0, h->own.bytes()));
  if (n_rows > 0 && n_cols > 0) RLH_HIP(hipMemcpy2D(h->own, h->lda, h_data, row_stride, n_cols, n_rows, hipMemcpyHostToDevice));
  *ph = h.release();
  return 0;
}

extern "C" int rlh_bytes_create_device(rlh_bytes_t *ph, int kind, int64_t n_rows, int64_t n_cols, const void *d_data,
                                       int64_t row_stride) {
  if (int rc = require_ready()) return rc;
  RLH_REQUIRE(ph, "rlh_bytes_create_device: null handle pointer");
  *ph = nullptr;
  RLH_REQUIRE(kind == RLH_BYTES_U8 || kind == RLH_BYTES_I8, "rlh_bytes_create_device: kind must be 0 (uint8) or 1 (int8), got %d", kind);
  RLH_REQUIRE(n_rows >= 0 && n_cols >= 0, "rlh_bytes_create_device: negative size");
  RLH_REQUIRE(n_rows == 0 || n_cols == 0 || d_data, "rlh_bytes_create_device: null data");
  RLH_REQUIRE(row_stride >= n_cols, "rlh_bytes_create_device: row stride smaller than the number of columns");
  std::unique_ptr<rlh_bytes> h(new rlh_bytes());
  h->kind = kind;
  h->rows = n_rows;
  h->cols = n_cols;
  if (n_rows > 0 && n_cols > 0 && n_cols % 16 == 0 && row_stride % 16 == 0 && (reinterpret_cast<uintptr_t>(d_data) & 15u) == 0) {
    h->A = (const unsigned char *)d_data;      // borrowed: every 16-byte piece the kernels read lies within the columns
    h->lda = row_stride;
    h->ncp = n_cols;
    *ph = h.release();
    return 0;
  }
  h->lda = (n_cols + 15) / 16 * 16;
  if (h->lda < 16) h->lda = 16;
  h->ncp = h->lda;
  Context &c = ctx();
  if (int rc = h->own.alloc((size_t)((n_rows > 0 ? n_rows : 1) * h->lda))) return rc;
  h->A = h->own.get();
  if (n_rows == 0) RLH_HIP(hipMemsetAsync(h->own, 0, h->own.bytes(), c.stream));
  if (n_rows > 0) {
    int64_t nb = (n_rows * (h->lda / 4) + 255) / 256;
    if (nb > 65536) nb = 65536;
    hipLaunchKernelGGL(bytes_pad_copy_kernel, dim3((unsigned)nb), dim3(256), 0, c.stream, h->own, h->lda, (const unsigned char *)d_data,
                       row_stride, n_rows, n_cols);
    RLH_HIP(hipGetLastError());
  }
  *ph = h.release();
  return 0;
}

extern "C" int rlh_bytes_destroy(rlh_bytes_t h) {
  if (!h) return 0;
  if (ctx().ready) (void)hipStreamSynchronize(ctx().stream);
  delete h;
  return 0;
}

extern "C" int rlh_bytes_info(rlh_bytes_t h, int64_t *n_rows, int64_t *n_cols, int64_t *device_bytes, int64_t *workspace_bytes) {
  RLH_REQUIRE(h, "rlh_bytes_info: null handle");
  if (n_rows) *n_rows = h->rows;
  if (n_cols) *n_cols = h->cols;
  if (device_bytes) *device_bytes = (int64_t)(h->own.bytes() + h->work.bytes());
  if (workspace_bytes) *workspace_bytes = (int64_t)h->work.bytes();
  return 0;
}

extern "C" int rlh_bytes_apply(rlh_bytes_t h, int transp, int64_t m, const void *X, int64_t ldx, void *Y, int64_t ldy,
                               const void *d_u, const void *d_c) {
  if (int rc = require_ready()) return rc;
  RLH_REQUIRE(h, "rlh_bytes_apply: null handle");
  RLH_REQUIRE(d_c || !d_u, "rlh_bytes_apply: a vector u without coefficients c");
  RLH_REQUIRE(transp == 0 || transp == 1, "rlh_bytes_apply: transp must be 0 or 1");
  RLH_REQUIRE(m >= 0, "rlh_bytes_apply: negative number of vectors");
  const int64_t ny = transp ? h->cols : h->rows, nx = transp ? h->rows : h->cols;
  if (m == 0 || ny == 0) return 0;
  RLH_REQUIRE(Y && (nx == 0 || X), "rlh_bytes_apply: null pointer");
  RLH_REQUIRE(ldx >= nx && ldy >= ny, "rlh_bytes_apply: Matrix and vectors dimensions incompatible");
  RLH_REQUIRE(m <= 65535, "rlh_bytes_apply: too many vectors");
  BytesArgs a;
  a.A = h->A; a.lda = h->lda; a.ncp = h->ncp;
  a.ny = ny; a.nx = nx;
  a.X = (const float *)X; a.ldx = ldx; a.Y = (float *)Y; a.ldy = ldy; a.m = (int)m;
  a.x_vec = ((reinterpret_cast<uintptr_t>(X) & 15u) == 0 && ldx % 4 == 0) ? 1 : 0;
  a.r1_u = (const float *)d_u; a.r1_c = (const float *)d_c;
  if (m > 64) return launch_bytes<128>(h, a, !transp);
  if (m > 32) return launch_bytes<64>(h, a, !transp);
  return launch_bytes<32>(h, a, !transp);
}

extern "C" int rlh_bytes_row_sumsq(rlh_bytes_t h, double *h_out) {
  if (int rc = require_ready()) return rc;
  RLH_REQUIRE(h, "rlh_bytes_row_sumsq: null handle");
  if (h->rows == 0) return 0;
  RLH_REQUIRE(h_out, "rlh_bytes_row_sumsq: null output");
  Context &c = ctx();
  DevBuf<double> d;
  if (int rc = d.alloc((size_t)h->rows)) return rc;
  const dim3 grid((unsigned)((h->rows + 3) / 4));
  if (h->kind == RLH_BYTES_I8) hipLaunchKernelGGL(bytes_row_sumsq_kernel<true>, grid, dim3(256), 0, c.stream, h->A, h->rows, h->lda, h->ncp, d);
  else hipLaunchKernelGGL(bytes_row_sumsq_kernel<false>, grid, dim3(256), 0, c.stream, h->A, h->rows, h->lda, h->ncp, d);
  RLH_HIP(hipGetLastError());
  RLH_HIP(hipStreamSynchronize(c.stream));
  RLH_HIP(hipMemcpy(h_out, d, h->rows * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int rlh_bytes_absmax(rlh_bytes_t h, double *h_out) {
  if (int rc = require_ready()) return rc;
  RLH_REQUIRE(h && h_out, "rlh_bytes_absmax: null handle or output");
  *h_out = 0.0;
  if (h->rows == 0 || h->cols == 0) return 0;
  Context &c = ctx();
  const int64_t rowdw = h->ncp / 4, dwords = h->rows * rowdw;
  int64_t nb = (dwords + 255) / 256;
  if (nb > 1024) nb = 1024;
  DevBuf<int> d;
  if (int rc = d.alloc((size_t)nb)) return rc;
  if (h->kind == RLH_BYTES_I8) hipLaunchKernelGGL(bytes_absmax_kernel<true>, dim3((unsigned)nb), dim3(256), 0, c.stream, h->A, dwords, rowdw, h->lda, d);
  else hipLaunchKernelGGL(bytes_absmax_kernel<false>, dim3((unsigned)nb), dim3(256), 0, c.stream, h->A, dwords, rowdw, h->lda, d);
  std::vector<int> host((size_t)nb);
  RLH_HIP(hipGetLastError());
  RLH_HIP(hipStreamSynchronize(c.stream));
  RLH_HIP(hipMemcpy(host.data(), d, nb * sizeof(int), hipMemcpyDeviceToHost));
  int mx = 0;
  for (int v : host) mx = v > mx ? v : mx;
  *h_out = (double)mx;
  return 0;
}
