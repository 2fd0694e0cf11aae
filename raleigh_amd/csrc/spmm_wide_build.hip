// Host side of the 256-row interleaved windowed layout of the sparse operator (kernel: spmm_wide.inc).
//
// Rows are cut into blocks of 256 (one row per thread of a 256-thread workgroup).  Per block the
// referenced columns are merged into windows of whole 16-column staging groups (spmm.h
// analyse_blocks); an entry stores its value and the 16-bit position of its column in the block's
// staged image.  Entries are stored in CHUNKS of 8 slots per row, as 16-byte pieces per thread:
//   values    [chunk][piece k][row]   piece k = slots k * VPG .. + VPG - 1,  VPG = 16 / sizeof(T)
//   positions [chunk][row]            8 x uint16
// so a wave fetches a chunk with es / 2 + 1 coalesced 16-byte loads per lane and the kernel streams
// a row of ANY length through a fixed number of registers.  The value bytes are copied as they
// are, so this file is independent of the element type.
#include "spmm.h"

namespace rlh {

// LDS bytes per staged column for NV vectors of es bytes: NV elements + one 16-byte pad, and an odd
// number of 16-byte slots so that consecutive columns fall into different bank groups
// (ds_read_b128 / ds_write_b128 of consecutive columns are then conflict-free).
int wide_stride(int nv, int es) {
  int s = nv * es + 16;
  if (((s / 16) & 1) == 0) s += 16;
  return s;
}

int wide_min_nv(int dtype) { return (dtype == RLH_S || dtype == RLH_D) ? 8 : 4; }

int wide_build(rlh_csr *h, const int64_t *indptr, const int32_t *indices, const void *values_, bool force) {
  const int es = (int)dtype_size(h->dtype);
  const int VP = es / 2;                         // 16-byte value pieces per chunk of 8 slots
  const int VPG = 16 / es;                       // values per piece
  const char *values = (const char *)values_;
  const int64_t n = h->n_rows;
  const int64_t nblocks = (n + kWideRows - 1) / kWideRows;
  h->wide_blocks = 0;
  if (nblocks == 0 || h->nnz == 0) return 0;
  const BlockAnalysis an = analyse_blocks(indptr, indices, n, h->n_cols, kWideRows, kWideGroup, 1);
  h->stage_ratio = an.ratio();
  // every block's image must fit the LDS with the smallest number of vectors per pass, positions
  // are 16 bits, a row has at most 8 * 32767 slots, and the group list must fit the header
  if ((int64_t)an.gmax * kWideGroup * wide_stride(wide_min_nv(h->dtype), es) + 2 * kWideHeader > kWideLdsBytes) return 0;
  if (an.gmax * 4 > kWideHeader || an.wmax > 8 * 32767) return 0;
  if (!force && an.staged * 10 > an.slots * 9) return 0;      // too little column locality for the staging to pay
  // Rows that share their column pattern with the row after them -- the unknowns of a node of a finite-element model: every
  // degree of freedom of a node couples to every degree of freedom of its neighbours -- are given to ONE thread in pairs: the
  // pair's entries are one position and two values, and the staged x values of an entry, which are what bounds the kernel
  // on long rows (every stored entry reads its NV staged values out of the LDS: profiles/r02_spmm_wide.txt), are read once
  // for both rows.  All complete pairs (2 i, 2 i + 1) of the matrix must qualify; real types; RLH_WIDE_PAIR=0: never.
  int K = 1;
  if ((h->dtype == RLH_S || h->dtype == RLH_D) && env_int("RLH_WIDE_PAIR", 1) != 0 && h->nnz >= 16 * n) {
    std::atomic<int> differ{0};
    host_parallel(64, [&](int t, int nt) {
      const int64_t pairs = n / 2;
      for (int64_t q = pairs * t / nt; q < pairs * (t + 1) / nt && !differ.load(std::memory_order_relaxed); ++q) {
        const int64_t r = 2 * q, la = indptr[r + 1] - indptr[r], lb = indptr[r + 2] - indptr[r + 1];
        if (la != lb || memcmp(indices + indptr[r], indices + indptr[r + 1], (size_t)la * sizeof(int32_t)) != 0) differ.store(1);
      }
    });
    if (!differ.load()) K = 2;
  }
  h->wide_k = K;
  const int TPS = kWideRows / K;                  // threads per set of vectors = row groups of a block
  std::vector<WideMeta> meta((size_t)nblocks);
  int64_t eoff = 0, goff = 0;
  for (int64_t b = 0; b < nblocks; ++b) {
    const int nch = std::max(1, (an.width[b] + 7) / 8);
    meta[b] = WideMeta{eoff, (int32_t)goff, (int16_t)nch, (int16_t)an.ngroups[b]};
    eoff += nch;
    goff += an.ngroups[b];
  }
  RLH_REQUIRE(goff < ((int64_t)1 << 31), "rlh_csr_create: too many staging groups");
  std::vector<int32_t> gsrc((size_t)goff);
  const int64_t nchunks = eoff + kWidePadChunks;  // padding: the kernel's prefetch runs ahead of the last block's chunks
  // K = 2: positions [chunk][row pair], values [chunk][row of the pair][piece][row pair]
  std::vector<char> idx((size_t)nchunks * TPS * 16, 0);
  std::vector<char> vals((size_t)nchunks * VP * kWideRows * 16, 0);
  parallel_blocks(nblocks, [&](int64_t b) {
    const std::vector<Win> &ws = an.wins[b];
    fill_group_sources(ws, an.ngroups[b], kWideGroup, gsrc.data() + meta[b].goff);
    const int64_t r0 = b * kWideRows;
    for (int l = 0; l < kWideRows; ++l) {
      const int64_t r = r0 + l;
      const int lt = l / K, lk = l % K;             // thread of the set, row of its group
      // (a row past the end of the matrix: the slots of its pair partner's positions with value 0)
      const int64_t rp_ = r < n ? r : (K > 1 && r - lk < n ? r - lk : -1);
      const int64_t p = rp_ >= 0 ? indptr[rp_] : 0, len = rp_ >= 0 ? indptr[rp_ + 1] - p : 0;
      const bool real_row = r < n;
      // padding slots carry value 0 and the position of the row's own first entry, so that in rows with at
      // least one entry they only ever touch a column the row references (0 * Inf of a foreign column would be
      // NaN); an empty row has no such column and takes position 0 of the image: +0 for finite vectors only
      const uint16_t padpos = len > 0 ? (uint16_t)staged_position(ws, indices[p]) : 0;
      for (int t = 0; t < meta[b].nchunks * 8; ++t) {
        const int64_t q = meta[b].eoff + t / 8;
        const int tt = t % 8;
        if (lk == 0) {
          uint16_t *pi = reinterpret_cast<uint16_t *>(idx.data() + ((size_t)q * TPS + lt) * 16) + tt;
          *pi = t < len ? (uint16_t)staged_position(ws, indices[p + t]) : padpos;
        }
        if (t < len && real_row) {
          char *pv = vals.data() + ((((size_t)q * K + lk) * VP + tt / VPG) * TPS + lt) * 16 + (size_t)(tt % VPG) * es;
          memcpy(pv, values + (size_t)(p + t) * es, (size_t)es);
        }
      }
    }
  });
  stage_flags(gsrc.data(), goff, kWideGroup, h->n_cols, &h->stage_inbounds, &h->stage_aligned);
  well_schedule(an.wins, nblocks, n, kWideRows, ctx().num_cu * 2, h->wide_order);
  h->wide_maxcol.resize((size_t)nblocks);
  for (int64_t b = 0; b < nblocks; ++b) h->wide_maxcol[(size_t)b] = an.wins[b].back().start + an.wins[b].back().len - 1;
  h->wide_gmax = an.gmax;
  if (int rc = h->wide_meta.upload(meta.data(), (size_t)nblocks * sizeof(WideMeta))) return rc;
  if (int rc = h->wide_gsrc.upload(gsrc.data(), (size_t)goff * sizeof(int32_t), sizeof(int32_t))) return rc;
  if (int rc = h->wide_idx.upload(idx.data(), idx.size())) return rc;
  if (int rc = h->wide_vals.upload(vals.data(), vals.size())) return rc;
  h->padded = eoff * 8 * kWideRows;
  h->device_bytes = nblocks * (int64_t)sizeof(WideMeta) + goff * 4 + (int64_t)idx.size() + (int64_t)vals.size();
  h->wide_blocks = nblocks;
  return 0;
}

// The launch order for `slots` resident workgroups over all blocks (part 0), the blocks that
// reference only columns < n_own (part 1) or the others (part 2); built on first use and kept.
int wide_sched(rlh_csr *h, int slots, int part, int64_t n_own, const int32_t **sched, int64_t *len, int *grid) {
  if (part == 0) n_own = 0;
  for (const WideSched &s : h->wide_scheds)
    if (s.slots == slots && s.part == part && s.n_own == n_own) {
      *sched = s.sched; *len = s.len; *grid = s.grid;
      return 0;
    }
  std::vector<int32_t> list, sch;
  for (int32_t b : h->wide_order) {
    const bool interior = h->wide_maxcol[(size_t)b] < n_own;
    if (part == 0 || (part == 1) == interior) list.push_back(b);
  }
  WideSched s{slots, 0, part, n_own, {}, 0};
  if (!list.empty()) {
    well_layout(list, slots, sch, s.grid);
    s.len = (int64_t)sch.size();
    if (int rc = s.sched.upload(sch.data(), sch.size() * sizeof(int32_t))) return rc;
  }
  if (h->wide_scheds.size() >= 16) {             // a bounded cache: drop the oldest
    if (h->wide_scheds.front().sched) (void)hipStreamSynchronize(ctx().stream);
    h->wide_scheds.erase(h->wide_scheds.begin());
  }
  *sched = s.sched; *len = s.len; *grid = s.grid;
  h->wide_scheds.push_back(std::move(s));
  return 0;
}

}  // namespace rlh
