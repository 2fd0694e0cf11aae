// Host side of the sparse operator's creation (K13): rlh_csr_create / rlh_csr_create_upper and the builders of the sliced ELL layout
// (csr_build), the 1024-row windowed layout (well_build) and its stacks (stack_build); kernels: spmm.hip.  Host code only.
#include <string>
#include <type_traits>
#include <unordered_map>

#include "spmm.h"

namespace rlh {

template <int DT>
static int csr_build(rlh_csr *h, const int64_t *indptr, const int32_t *indices, const void *values_) {
  using T = typename DType<DT>::T;
  const T *values = (const T *)values_;
  const int64_t n = h->n_rows, ns = (n + 63) / 64;
  std::vector<int64_t> sp(ns + 1, 0);
  for (int64_t s = 0; s < ns; ++s) {
    int64_t w = 0;
    for (int64_t r = s * 64; r < n && r < (s + 1) * 64; ++r) w = std::max(w, indptr[r + 1] - indptr[r]);
    sp[s + 1] = sp[s] + w * 64;
  }
  const int64_t padded = sp[ns];
  std::vector<int32_t> cols((size_t)padded);
  std::vector<T> vals((size_t)padded);
  for (int64_t s = 0; s < ns; ++s) {
    const int64_t w = (sp[s + 1] - sp[s]) / 64;
    for (int l = 0; l < 64; ++l) {
      const int64_t r = s * 64 + l;
      const int64_t b = r < n ? indptr[r] : 0, len = r < n ? indptr[r + 1] - b : 0;
      // padding entries carry value 0 and an in-range column: the row's first, so that a row with at least one entry
      // never touches a foreign column; an empty row has none and takes column 0 (0 * x[0]: NaN if x[0] is not finite)
      const int32_t padcol = len > 0 ? indices[b] : 0;
      for (int64_t t = 0; t < w; ++t) {
        const int64_t e = sp[s] + t * 64 + l;
        if (t < len) { cols[e] = indices[b + t]; vals[e] = values[b + t]; }
        else { cols[e] = padcol; memset(&vals[e], 0, sizeof(T)); }
      }
    }
  }
  h->n_slices = ns;
  h->padded = padded;
  if (int rc = h->slice_ptr.upload(sp.data(), (size_t)(ns + 1) * sizeof(int64_t))) return rc;
  if (padded > 0) {
    if (int rc = h->cols.upload(cols.data(), (size_t)padded * sizeof(int32_t))) return rc;
    if (int rc = h->vals.upload(vals.data(), (size_t)padded * sizeof(T))) return rc;
  }
  h->device_bytes = (ns + 1) * 8 + padded * (4 + (int64_t)sizeof(T));
  return 0;
}

// The 8 entry slots of `row` (>= n: no such row) as thread l of the block or stack member whose slots start at eoff; padding slots carry
// value 0 and the position of the row's own first entry, so that in a row with at least one entry they only ever touch a column the row references
// (0 * Inf of a foreign column would be NaN).  An EMPTY row has no column of its own: its slots take position 0 of the staged image, so the row is +0
// for finite vectors and NaN where the element at that position is not finite (pinned by the tests; a select in the kernels' store is not worth that case)
template <typename T>
static inline void fill_row_slots(const std::vector<Win> &ws, const int64_t *indptr, const int32_t *indices, const T *values, int64_t row,
                                  int64_t n, int64_t eoff, int l, uint16_t *idx, T *vals) {
  const int64_t p = row < n ? indptr[row] : 0, len = row < n ? indptr[row + 1] - p : 0;
  const uint16_t padpos = len > 0 ? (uint16_t)staged_position(ws, indices[p]) : 0;
  size_t hint = 0;
  for (int32_t t = 0; t < 8; ++t) {
    const int64_t ev = well_val_index<T>(eoff, t, l), ei = well_idx_index(eoff, t, l);
    if (t < len) {
      idx[ei] = (uint16_t)staged_position_walk(ws, indices[p + t], hint);
      vals[ev] = values[p + t];
    } else {
      idx[ei] = padpos;
      memset(&vals[ev], 0, sizeof(T));
    }
  }
}

// What the 1024-row layouts upload per unit (a block, or a stack of R blocks): records, staging groups and the 8 R entry
// slots of its 1024 threads.  idx / vals are NOT zeroed at allocation (a std::vector would fill 0.6 GB serially before the
// host threads overwrite every element of it; left alone, the pages are first touched by the threads that fill them).
template <typename T> struct WellEntries {
  const int R;
  std::vector<WellMeta> meta;
  std::vector<int32_t> gsrc;
  const size_t ne;
  std::unique_ptr<uint16_t[]> idx;
  std::unique_ptr<T[]> vals;
  WellEntries(int64_t units, int R_) : R(R_), meta((size_t)units), ne(meta.size() * 8 * R * kWellRows), idx(new uint16_t[ne]), vals(new T[ne]) {}
  // the units' records from their staging groups and (a block's: `width`) longest row
  int place(const std::vector<int32_t> &ngroups, const std::vector<int32_t> *width) {
    int64_t goff = 0;
    for (size_t u = 0; u < meta.size(); ++u) {
      meta[u] = WellMeta{(int64_t)u * 8 * R, (int32_t)goff, (width ? (*width)[u] : 8) | (ngroups[u] << 8)};
      goff += ngroups[u];
    }
    RLH_REQUIRE(goff < ((int64_t)1 << 31), "rlh_csr_create: too many staging groups");
    gsrc.resize((size_t)goff);
    return 0;
  }
};

// The far stride of a grid operator: the offset (largest column - row) most rows share, e.g. one grid plane for a 3-D
// stencil (0: fewer than 60 % of the sampled rows agree).  Row blocks of a stack are partners one such stride apart.
static int64_t far_stride(const int64_t *indptr, const int32_t *indices, int64_t n) {
  std::unordered_map<int64_t, int64_t> count;
  int64_t samples = 0;
  const int64_t step = std::max<int64_t>(1, n / 50000);
  for (int64_t i = 0; i < n; i += step) {
    if (indptr[i + 1] == indptr[i]) continue;
    const int64_t d = (int64_t)indices[indptr[i + 1] - 1] - i;
    ++samples;
    if (d > 0) ++count[d];
  }
  int64_t best = 0, best_count = 0;
  for (const auto &kv : count)
    if (kv.second > best_count || (kv.second == best_count && kv.first < best)) { best = kv.first; best_count = kv.second; }
  return best_count * 10 >= samples * 6 ? best : 0;
}

// ---- the stacked layout (spmm.hip, "Stacked blocks"): which row blocks there are, which form a stack, what each stack stages
struct StackPlan {
  const int64_t *indptr;                   // the matrix: n rows, and its column count rounded up to a multiple of 8
  const int32_t *indices;                  // (windows may end there: aligned starts at the far end too)
  int64_t n, nc8;
  std::vector<int64_t> brow;               // row block k = rows [brow[k], brow[k + 1])
  std::vector<int32_t> members;            // kStkR row blocks per stack (-1: none)
  std::vector<int32_t> owner;              // the stack of every row block (set_owner)
  std::vector<std::vector<Win>> swins;     // per stack: the windows of its members' columns together (analyse) ...
  std::vector<int32_t> ngroups;            // ... and their staging groups of 64 columns
  int64_t stacks() const { return (int64_t)members.size() / kStkR; }
  bool paired(int64_t sb) const { return members[(size_t)(sb * kStkR + 1)] >= 0; }
  void set_owner() {                               // called wherever `members` changes
    owner.assign(brow.size() - 1, -1);
    for (size_t k = 0; k < members.size(); ++k)
      if (members[k] >= 0) owner[(size_t)members[k]] = (int32_t)(k / kStkR);
  }
  void analyse() {
    swins.assign((size_t)stacks(), std::vector<Win>());
    ngroups.assign((size_t)stacks(), 0);
    parallel_blocks(stacks(), [&](int64_t sb) {
      std::vector<int32_t> cols;
      for (int r = 0; r < kStkR; ++r) {
        const int64_t mb = members[(size_t)(sb * kStkR + r)];
        if (mb >= 0) cols.insert(cols.end(), indices + indptr[brow[(size_t)mb]], indices + indptr[brow[(size_t)mb + 1]]);
      }
      ngroups[(size_t)sb] = find_windows_of(cols, nc8, 32, 64, 8, swins[(size_t)sb]) / 64;
    });
  }
};

// groups one vector's image may have: a buffer of the register-staged kernel for the real types (the LDS-DMA kernel
// takes over from it where the image fits a ring slot), a ring slot for the complex ones (LDS-DMA only)
template <int DT> constexpr int kStkDmaG = StkRing<typename DType<DT>::T>::SLOT / (64 * (int)sizeof(typename DType<DT>::T));
template <int DT> constexpr int kStkBufG = DType<DT>::cplx ? kStkDmaG<DT> : kStkBufBytes / (64 * (int)sizeof(typename DType<DT>::T));

// the row ranges of the blocks: uniform 1024-row blocks, paired by greedy matching on the window-overlap graph (`single`: stacks of one)
static void stack_match(StackPlan &p, const std::vector<std::vector<Win>> &wins, bool single) {
  constexpr int R = kStkR;
  const int64_t nblocks = (int64_t)wins.size(), n = p.n;
  for (int64_t b = 0; b <= nblocks; ++b) p.brow.push_back(std::min(b * kWellRows, n));
  // overlap of block b's windows with the rows of block c, both directions summed
  std::vector<std::vector<std::pair<int32_t, int64_t>>> adj((size_t)nblocks);
  auto bump = [&](int64_t b, int64_t c, int64_t ov) {
    for (auto &e : adj[(size_t)b])
      if (e.first == (int32_t)c) { e.second += ov; return; }
    adj[(size_t)b].push_back({(int32_t)c, ov});
  };
  for_each_overlap(wins, nblocks, n, kWellRows, [&](int64_t b, int64_t c, int64_t ov) {
    if (c == b) return;
    bump(b, c, ov);
    bump(c, b, ov);
  });
  std::vector<char> taken((size_t)nblocks, 0);
  int64_t next_free = 0;
  for (int64_t b = 0; b < nblocks; ++b) {
    if (taken[(size_t)b]) continue;
    const size_t first = p.members.size();
    taken[(size_t)b] = 1;
    p.members.push_back((int32_t)b);
    for (int r = 1; r < R; ++r) {
      int32_t best = -1;
      int64_t wbest = 0;
      if (single) { p.members.push_back(-1); continue; }
      for (size_t k = first; k < p.members.size(); ++k)                  // heaviest free neighbour of the stack so far
        for (const auto &e : adj[(size_t)p.members[k]])
          if (!taken[(size_t)e.first] && (e.second > wbest || (e.second == wbest && best >= 0 && e.first < best))) {
            best = e.first;
            wbest = e.second;
          }
      if (best < 0) {                                                   // none: the next free block in order
        while (next_free < nblocks && taken[(size_t)next_free]) ++next_free;
        if (next_free < nblocks) best = (int32_t)next_free;
      }
      if (best >= 0) taken[(size_t)best] = 1;
      p.members.push_back(best);
    }
  }
  p.set_owner();
}

// Uniform blocks pair up exactly when the far stride of the operator (a grid plane) is a whole number of them, and well
// enough when it nearly is (215^2 = 45.14 blocks: 2.49 staged elements per row).  When a block and its partner one plane
// on are half a block out of step (126^2 = 15.5 blocks), the union of their windows outgrows a slot of the ring and the
// stacks fall apart into stacks of one (config 5 at 126^3: 1.03 ms against 0.82 ms at 128^3).  Then -- and only then: at
// 215^3 the uniform blocks are 4 % faster -- the blocks are cut plane by plane instead, ceil(plane / 1024) blocks of
// (nearly) equal size per plane, so that block j of a plane and block j of the next are exact translates of each other:
// 126^3 complex128 in 0.865 ms.  Float32 operators keep the uniform blocks (their bfloat16 step moves rows in 16-byte
// pieces of eight).  RLH_SPMM_STACK_ALIGN=0: never, =2: whenever a far stride exists.
template <int DT>
static void stack_recut_by_plane(StackPlan &p) {
  constexpr int R = kStkR;
  const int64_t n = p.n;
  const int align_mode = env_int("RLH_SPMM_STACK_ALIGN", 1);
  int64_t apart = 0, pairs = 0;
  for (int64_t sb = 0; sb < p.stacks(); ++sb)
    if (p.paired(sb)) { ++pairs; apart += p.ngroups[(size_t)sb] > std::min(kStkBufG<DT>, kStkDmaG<DT>); }
  const int64_t plane = (R == 2 && DT != RLH_S && align_mode != 0 && (apart * 4 > pairs || align_mode == 2)) ? far_stride(p.indptr, p.indices, n) : 0;
  if (!(plane > kWellRows && plane < n && plane % kWellRows != 0)) return;
  p.brow.assign(1, 0);
  p.members.clear();
  std::vector<int64_t> first_of_plane;              // block id of the first block of every plane
  for (int64_t p0 = 0; p0 < n; p0 += plane) {
    const int64_t len = std::min(plane, n - p0), k = (len + kWellRows - 1) / kWellRows;
    first_of_plane.push_back((int64_t)p.brow.size() - 1);
    for (int64_t j = 1; j <= k; ++j) p.brow.push_back(p0 + len * j / k);
  }
  first_of_plane.push_back((int64_t)p.brow.size() - 1);
  const int64_t planes = (int64_t)first_of_plane.size() - 1;
  for (int64_t q = 0; q < planes; q += 2) {
    const int64_t b0 = first_of_plane[(size_t)q], k0 = first_of_plane[(size_t)q + 1] - b0;
    const int64_t b1 = q + 1 < planes ? first_of_plane[(size_t)q + 1] : -1, k1 = q + 1 < planes ? first_of_plane[(size_t)q + 2] - b1 : 0;
    for (int64_t j = 0; j < std::max(k0, k1); ++j) {
      if (j < k0) { p.members.push_back((int32_t)(b0 + j)); p.members.push_back(j < k1 ? (int32_t)(b1 + j) : -1); }
      else { p.members.push_back((int32_t)(b1 + j)); p.members.push_back(-1); }
    }
  }
  p.set_owner();
  p.analyse();
}

// a stack whose image does not fit (grid planes half a row block out of step with the blocks: 126^2 rows = 15.5
// blocks) is taken apart into stacks of one
// ... and so is a stack of a real type whose image fits the register-staged kernel's buffer but not a slot of the LDS-DMA
// ring, as long as such stacks are few (the blocks of a row shard next to its halo columns: their windows lie in two far
// apart column ranges): one oversized stack would otherwise take the LDS-DMA kernel -- the only one that serves row
// shards -- away from the whole operator (the forced one-rank run of lap3d 215^3 fell back to the unstacked kernel that
// way: 1.33 instead of 1.12 ms per product)
template <int DT>
static void stack_take_apart(StackPlan &p) {
  constexpr int R = kStkR, BUFG = kStkBufG<DT>, DMAG = kStkDmaG<DT>;
  const int64_t nst = p.stacks();
  int64_t over_dma = 0;
  for (int64_t sb = 0; sb < nst; ++sb) over_dma += p.ngroups[(size_t)sb] > DMAG && p.paired(sb);
  const int CAPG = (over_dma > 0 && over_dma * 20 <= nst) ? std::min(BUFG, DMAG) : BUFG;
  bool split = false;
  for (int64_t sb = 0; sb < nst && !split; ++sb) split = p.ngroups[(size_t)sb] > CAPG && p.paired(sb);
  if (!split) return;
  std::vector<int32_t> again;
  for (int64_t sb = 0; sb < nst; ++sb) {
    const bool whole = p.ngroups[(size_t)sb] <= CAPG || !p.paired(sb);
    for (int r = 0; r < R; ++r) {
      again.push_back(p.members[(size_t)(sb * R + r)]);
      if (!whole)
        for (int q = 1; q < R; ++q) again.push_back(-1);
    }
  }
  p.members.swap(again);
  p.set_owner();
  p.analyse();
}

// the entries of the stacks; *self: slot 7 of EVERY row carries the position of the row's own column (stk_self)
template <typename T>
static int stack_fill(const StackPlan &p, const T *values, WellEntries<T> &e, int *self) {
  constexpr int R = kStkR;
  if (int rc = e.place(p.ngroups, nullptr)) return rc;
  std::atomic<int> self_ok{1};
  parallel_blocks(p.stacks(), [&](int64_t sb) {
    const std::vector<Win> &ws = p.swins[(size_t)sb];
    fill_group_sources(ws, p.ngroups[(size_t)sb], 64, e.gsrc.data() + e.meta[(size_t)sb].goff);
    for (int r = 0; r < R; ++r) {
      const int64_t mb = p.members[(size_t)(sb * R + r)], eoff = e.meta[(size_t)sb].eoff + 8 * r;
      for (int l = 0; l < kWellRows; ++l) {
        const int64_t row = mb >= 0 && p.brow[(size_t)mb] + l < p.brow[(size_t)mb + 1] ? p.brow[(size_t)mb] + l : p.n;
        fill_row_slots(ws, p.indptr, p.indices, values, row, p.n, eoff, l, e.idx.get(), e.vals.get());
        // the LAST slot of a row with a free one carries (value 0 and) the position of the row's OWN column, where the row
        // stores its diagonal entry: the fused Chebyshev step then finds y[row] in the staged image instead of reading the
        // block a second time (well_stack_dma_kernel<..., CHEB>); one row without makes the handle say so
        if (row < p.n) {
          const int32_t *c0 = p.indices + p.indptr[row], *c1 = p.indices + p.indptr[row + 1];
          if (c1 - c0 <= 7 && std::find(c0, c1, (int32_t)row) != c1) e.idx[(size_t)well_idx_index(eoff, 7, l)] = (uint16_t)staged_position(ws, (int32_t)row);
          else self_ok.store(0, std::memory_order_relaxed);
        }
      }
    }
  });
  *self = self_ok.load();
  return 0;
}

// value dictionary: the distinct 8-slot value tuples of the rows (byte-wise) into `table`, per row the index of its tuple into `pat`; given up
// (false) beyond kStkMaxPatterns or with RLH_SPMM_STACK_PAT=0.  (member slot k = R stack + member has its entries at 8 k: WellEntries::place)
template <typename T>
static bool stack_value_dictionary(const WellEntries<T> &e, std::vector<int32_t> &pat, std::vector<T> &table) {
  const int64_t nslots = (int64_t)e.meta.size() * e.R;
  pat.assign((size_t)nslots * kWellRows, 0);
  std::unordered_map<std::string, int32_t> seen;         // the tuple's bytes -> its index in `table`
  bool ok = env_int("RLH_SPMM_STACK_PAT", 1) != 0;
  int32_t last_id = -1;
  T last_tup[8];
  for (int64_t k = 0; k < nslots && ok; ++k)
    for (int l = 0; l < kWellRows; ++l) {
      T tup[8];
      for (int t = 0; t < 8; ++t) tup[t] = e.vals[(size_t)well_val_index<T>(8 * k, t, l)];
      if (last_id < 0 || memcmp(last_tup, tup, sizeof(tup))) {          // (a stencil: the same as the row before)
        const auto ins = seen.emplace(std::string(reinterpret_cast<const char *>(tup), sizeof(tup)), (int32_t)(table.size() / 8));
        last_id = ins.first->second;
        if (ins.second) {
          if (last_id >= kStkMaxPatterns) { ok = false; break; }
          table.insert(table.end(), tup, tup + 8);
        }
        memcpy(last_tup, tup, sizeof(tup));
      }
      pat[(size_t)(k * kWellRows + l)] = last_id;
    }
  return ok && !table.empty();
}

// position patterns per member into `dtab`: the positions less the row's index in its block (mod 2^16), the row's pattern
// into the upper half of its word of `pat`; given up (false, `pat` as it was) beyond kStkMaxDeltas per member
template <typename T>
static bool stack_position_dictionary(const StackPlan &p, const WellEntries<T> &e, std::vector<int32_t> &pat, std::vector<uint16_t> &dtab) {
  const int64_t nslots = p.stacks() * kStkR;
  bool dok = true;
  dtab.assign((size_t)nslots * kStkMaxDeltas * 8, 0);
  for (int64_t k = 0; k < nslots && dok; ++k) {
    uint16_t *tab = dtab.data() + (size_t)k * kStkMaxDeltas * 8;
    int used = 0;
    const int64_t mb = p.members[(size_t)k];
    for (int l = 0; l < kWellRows && dok; ++l) {
      if (mb < 0 || p.brow[(size_t)mb] + l >= p.brow[(size_t)mb + 1]) continue;   // no such row: nothing is stored for it, any pattern will do
      uint16_t tup[8];
      for (int t = 0; t < 8; ++t) tup[t] = (uint16_t)(e.idx[(size_t)well_idx_index(8 * k, t, l)] - (uint16_t)l);
      int id = -1;
      for (int c = used - 1; c >= 0; --c)             // (the last one used is the likeliest)
        if (!memcmp(tab + c * 8, tup, sizeof(tup))) { id = c; break; }
      if (id < 0) {
        if (used >= kStkMaxDeltas) { dok = false; break; }
        id = used++;
        memcpy(tab + id * 8, tup, sizeof(tup));
      }
      pat[(size_t)(k * kWellRows + l)] |= id << 16;
    }
  }
  if (!dok)
    for (int32_t &w : pat) w &= 0xffff;
  return dok;
}

// the stacks' arrays onto the device (the launch order laid out by stk_launch.set); pat / table are uploaded where `ok`, dtab where `dok`
template <typename T>
static int stack_upload(rlh_csr *h, const StackPlan &p, const WellEntries<T> &e, std::vector<int32_t> &&order, std::vector<int32_t> &&maxcol,
                        bool ok, bool dok, const std::vector<int32_t> &pat, const std::vector<T> &table, const std::vector<uint16_t> &dtab) {
  const int64_t nst = p.stacks();
  if (int rc = h->stk_launch.set(std::move(order), std::move(maxcol))) return rc;
  if (int rc = h->stk_meta.upload(e.meta.data(), (size_t)nst * sizeof(WellMeta))) return rc;
  std::vector<int32_t> ranges(p.members.size() * 2, 0);                 // (first row, rows) of every member; (0, 0): none
  for (size_t k = 0; k < p.members.size(); ++k)
    if (const int64_t mb = p.members[k]; mb >= 0) {
      ranges[2 * k] = (int32_t)p.brow[(size_t)mb];
      ranges[2 * k + 1] = (int32_t)(p.brow[(size_t)mb + 1] - p.brow[(size_t)mb]);
    }
  if (int rc = h->stk_member.upload(ranges.data(), ranges.size() * sizeof(int32_t))) return rc;
  if (int rc = h->stk_gsrc.upload(e.gsrc.data(), e.gsrc.size() * sizeof(int32_t), sizeof(int32_t))) return rc;
  h->stk_npat = ok ? (int64_t)table.size() / 8 : 0;
  if (dok)
    if (int rc = h->stk_dtab.upload(dtab.data(), dtab.size() * sizeof(uint16_t))) return rc;
  if (ok) {
    if (int rc = h->stk_pat.upload(pat.data(), pat.size() * sizeof(int32_t))) return rc;
    if (int rc = h->stk_table.upload(table.data(), table.size() * sizeof(T))) return rc;
  }
  if (int rc = h->stk_idx.upload(e.idx.get(), e.ne * sizeof(uint16_t))) return rc;
  if (int rc = h->stk_vals.upload(e.vals.get(), e.ne * sizeof(T))) return rc;
  h->device_bytes += nst * (int64_t)sizeof(WellMeta) + h->stk_launch.len * 4 + (int64_t)e.gsrc.size() * 4 + (int64_t)p.members.size() * 8 +
                     (int64_t)e.ne * (2 + (int64_t)sizeof(T)) + (dok ? (int64_t)dtab.size() * 2 : 0) +
                     (ok ? (int64_t)pat.size() * 4 + (int64_t)table.size() * (int64_t)sizeof(T) : 0);
  h->stk_blocks = nst;
  return 0;
}

// Host side of the stacked layout: the stacks by greedy matching on the window-overlap graph of the 1024-row blocks
// (`wins`: their windows), then windows / staging groups / entries per stack exactly as well_build lays them out per block.
// Built only where it stages at least 10 % less than the unstacked layout (RLH_SPMM_STACK=2 builds it regardless, 0 never).
template <int DT>
static int stack_build(rlh_csr *h, const int64_t *indptr, const int32_t *indices, const void *values_, const std::vector<std::vector<Win>> &wins,
                       int64_t staged_unstacked) {
  using T = typename DType<DT>::T;
  constexpr int R = kStkR, BUFG = kStkBufG<DT>;
  const int64_t n = h->n_rows, nblocks = (int64_t)wins.size();
  const int mode = env_int("RLH_SPMM_STACK", 1);
  h->stk_blocks = 0;
  // (fewer than 4 row blocks per CU: halving the number of work units costs more than the staging saves -- lap3d 61^3,
  // 222 blocks: 12.4 us as blocks, 14.1 us as stacks)
  // A complex operator that small (the row shards of BASELINE config 5: 977 / 489 / 245 blocks on 2 / 4 / 8 GPUs) still takes
  // the LDS-DMA kernel -- its alternative is the interleaved layout at 0.6-0.7 of the rate: as pairs while every CU gets a
  // stack (measured on one shard of 2 / 4: product 0.44 / 0.24 ms as pairs, 0.54 / 0.29 as stacks of one, 0.77 / 0.40
  // interleaved), as stacks of ONE block below that (one of 8: 0.15 ms, 0.18 as pairs on half the CUs, 0.19 interleaved;
  // tools/c5_shard_bench.py).  RLH_SPMM_STACK_SINGLE=0: no stacks then, as for the real types.
  bool single = false;
  if (mode == 0 || nblocks < 2) return 0;
  if (mode < 2 && nblocks < 4 * (int64_t)ctx().num_cu) {
    // (below three quarters of a block per CU the interleaved layout's 256-row units fill the chip better: 123 blocks, 50^3:
    // product 0.077 ms interleaved, 0.087 as stacks of one; 256 blocks, 64^3: 0.170 against 0.131)
    if (!DType<DT>::cplx || 4 * nblocks < 3 * (int64_t)ctx().num_cu || env_int("RLH_SPMM_STACK_SINGLE", 1) == 0) return 0;
    single = 4 * nblocks < 7 * (int64_t)ctx().num_cu;
  }
  PhaseClock clk;
  const int64_t nc8 = (h->n_cols + 7) & ~(int64_t)7;
  StackPlan plan{indptr, indices, n, nc8};
  stack_match(plan, wins, single);
  clk.lap("stack: matching");
  plan.analyse();
  stack_recut_by_plane<DT>(plan);
  clk.lap("stack: windows");
  stack_take_apart<DT>(plan);
  const int64_t nst = plan.stacks();
  int64_t staged = 0;
  int32_t gmax = 0;
  for (int64_t sb = 0; sb < nst; ++sb) {
    staged += (int64_t)plan.ngroups[(size_t)sb] * 64;
    gmax = std::max(gmax, plan.ngroups[(size_t)sb]);
  }
  h->stk_staged = (double)staged / (double)(n > 0 ? n : 1);
  h->stk_gmax = gmax;
  if (gmax > BUFG) {                                                     // a stack's image must fit one buffer
    if (clk.on) fprintf(stderr, "csr layout: stack: not built (largest image %d groups of 64 columns, a buffer holds %d)\n", gmax, BUFG);
    return 0;
  }
  // (the complex types: the alternative is the interleaved layout, which re-stages the windows in passes of a few vectors
  // -- config 5's operator at 160^3 in complex64: 1.87 ms there, 0.86 ms here)
  if (mode < 2 && !DType<DT>::cplx && staged * 10 > staged_unstacked * 9) return 0;
  WellEntries<T> e(nst, R);
  if (int rc = stack_fill(plan, (const T *)values_, e, &h->stk_self)) return rc;
  clk.lap("stack: entries");
  int aligned = 0;
  const int64_t overhang = stage_flags(e.gsrc.data(), (int64_t)e.gsrc.size(), 64, h->n_cols, nullptr, &aligned);
  if (overhang > nc8 - h->n_cols) return 0;                               // 16-byte staging needs whole groups
  h->stk_overhang = overhang > 0 ? (int)(nc8 - h->n_cols) : 0;
  h->stk_aligned = aligned;
  std::vector<int32_t> order, maxcol((size_t)nst);
  for (int64_t sb = 0; sb < nst; ++sb) maxcol[(size_t)sb] = plan.swins[(size_t)sb].back().start + plan.swins[(size_t)sb].back().len - 1;
  std::vector<int32_t> granule_owner((size_t)((n + kWellRows - 1) / kWellRows), -1);      // the stack that owns row 1024 c
  const int64_t nblk = (int64_t)plan.brow.size() - 1;
  int64_t blk = 0;
  for (size_t c = 0; c < granule_owner.size(); ++c) {
    while (blk + 1 < nblk && plan.brow[(size_t)blk + 1] <= (int64_t)c * kWellRows) ++blk;
    granule_owner[c] = plan.owner[(size_t)blk];
  }
  well_schedule(plan.swins, nst, n, kWellRows, ctx().num_cu, order, &granule_owner);
  clk.lap("stack: schedule");
  std::vector<int32_t> pat;
  std::vector<T> table;
  std::vector<uint16_t> dtab;
  const bool ok = stack_value_dictionary(e, pat, table);
  clk.lap("stack: value dictionary");
  const bool dok = ok && env_int("RLH_SPMM_STACK_PAT", 1) >= 1 && env_int("RLH_SPMM_STACK_DPAT", 1) != 0 && stack_position_dictionary(plan, e, pat, dtab);
  clk.lap("stack: position dictionary");
  if (int rc = stack_upload(h, plan, e, std::move(order), std::move(maxcol), ok, dok, pat, table, dtab)) return rc;
  clk.lap("stack: upload");
  return 0;
}

// Host side of the 1024-row windowed layout.  Returns 0 with h->well_blocks == 0 when the matrix
// does not qualify (a row longer than 8 entries, a block whose windows do not fit the LDS buffer,
// or too little column locality for the staging to pay).
template <int DT>
static int well_build(rlh_csr *h, const int64_t *indptr, const int32_t *indices, const void *values_, bool force, bool stack_only) {
  using T = typename DType<DT>::T;
  constexpr int SMAX = WellCfg<T>::SMAX;
  const T *values = (const T *)values_;
  const int64_t n = h->n_rows, nblocks = (n + kWellRows - 1) / kWellRows;
  h->well_blocks = 0;
  if (nblocks == 0 || h->nnz == 0) return 0;
  PhaseClock clk;
  // groups per block: a multiple of 8 (one 16-byte load covers 2, 4 or -- bfloat16 -- 8 groups)
  const BlockAnalysis an = analyse_blocks(indptr, indices, n, h->n_cols, kWellRows, 64, 8);
  clk.lap("well: windows");
  h->stage_ratio = an.ratio();
  // (the limit on a block's image is the unstacked kernel's staging buffer: a complex operator never runs that kernel -- its
  // stacks have a ring slot of their own size, checked by stack_build)
  if (an.wmax > 8 || (!stack_only && an.gmax > 16 * SMAX)) {
    if (clk.on) fprintf(stderr, "csr layout: well: not built (longest row %d, largest block image %d groups of 64 columns, limit %d)\n", an.wmax, an.gmax, 16 * SMAX);
    return 0;
  }
  // measured (profiles/r01_spmm_windowed.txt): at 0.65 staged elements per entry slot (5-point
  // stencil) the windowed kernel is 1.27x faster than the sliced one, at 1.06 (a diagonal
  // matrix) 4 % slower
  if (!force && an.staged * 10 > an.slots * 9) {
    if (clk.on) fprintf(stderr, "csr layout: well: not built (%lld staged elements for %lld entry slots)\n", (long long)an.staged, (long long)an.slots);
    return 0;
  }
  h->well_staged = (double)an.staged / (double)n;
  // the complex types: the stacks for rlh_spmm on the whole operator, the interleaved layout for the rest
  if (stack_only) return stack_build<DT>(h, indptr, indices, values_, an.wins, an.staged);
  h->well_wmax = 8;
  WellEntries<T> e(nblocks, 1);                       // every row is stored as 8 slots (16-byte pieces per thread)
  if (int rc = e.place(an.ngroups, &an.width)) return rc;
  parallel_blocks(nblocks, [&](int64_t b) {
    fill_group_sources(an.wins[b], an.ngroups[b], 64, e.gsrc.data() + e.meta[b].goff);
    for (int l = 0; l < kWellRows; ++l)
      fill_row_slots(an.wins[b], indptr, indices, values, b * kWellRows + l, n, e.meta[b].eoff, l, e.idx.get(), e.vals.get());
  });
  clk.lap("well: entries");
  const int64_t goff = (int64_t)e.gsrc.size();
  stage_flags(e.gsrc.data(), goff, 64, h->n_cols, &h->stage_inbounds, &h->stage_aligned);      // what the 16-byte staging path may assume
  std::vector<int32_t> order, maxcol((size_t)nblocks);
  well_schedule(an.wins, nblocks, n, kWellRows, ctx().num_cu, order);
  for (int64_t b = 0; b < nblocks; ++b) maxcol[(size_t)b] = an.wins[b].back().start + an.wins[b].back().len - 1;
  clk.lap("well: schedule");
  if (int rc = h->well_launch.set(std::move(order), std::move(maxcol))) return rc;
  if (int rc = h->well_meta.upload(e.meta.data(), (size_t)nblocks * sizeof(WellMeta))) return rc;
  if (int rc = h->well_gsrc.upload(e.gsrc.data(), (size_t)goff * sizeof(int32_t), sizeof(int32_t))) return rc;
  if (int rc = h->well_idx.upload(e.idx.get(), e.ne * sizeof(uint16_t), sizeof(uint16_t))) return rc;
  if (int rc = h->well_vals.upload(e.vals.get(), e.ne * sizeof(T), sizeof(T))) return rc;
  h->padded = (int64_t)e.ne;
  h->device_bytes = nblocks * (int64_t)sizeof(WellMeta) + h->well_launch.len * 4 + goff * 4 + (int64_t)e.ne * (2 + (int64_t)sizeof(T));
  h->well_blocks = nblocks;
  clk.lap("well: upload");
  if (h->stage_inbounds) return stack_build<DT>(h, indptr, indices, values_, an.wins, an.staged);
  return 0;
}

// The Hermitian operator defined by the UPPER triangle of a square CSR matrix (entries below the diagonal, if the caller
// stores them, are ignored): A = U + U^H - diag(U), what mkl_?csrmm computes with the 'SUNF' / 'HUNF' descriptor the
// reference passes (raleigh/algebra/mkl_wrap.py:211-276).  One counting pass and one fill pass over the entries on the
// host (row i of the result = the mirrored entries (j, i), j < i, in ascending j, then the row's own upper entries:
// sorted if the input rows are), then the ordinary rlh_csr_create.
template <typename T> static inline T conj_of(T v) { return v; }
template <> inline c32 conj_of(c32 v) { return c32{v.re, -v.im}; }
template <> inline c64 conj_of(c64 v) { return c64{v.re, -v.im}; }

template <typename T>
static int csr_from_upper(rlh_csr_t *out, int dtype, int64_t n, const int64_t *indptr, const int32_t *indices, const T *values) {
  PhaseClock clk;
  // counting pass, rows dealt to the host threads: own entries per row, mirrored entries per target row (atomic: two
  // threads may mirror into the same row)
  std::unique_ptr<std::atomic<int64_t>[]> cnt(new std::atomic<int64_t>[(size_t)n + 1]);
  std::vector<int64_t> below((size_t)n, 0);
  std::atomic<int64_t> bad_row{-1};
  std::atomic<int> bad_kind{0};
  host_parallel(64, [&](int t, int nt) {
    for (int64_t i = n * t / nt; i < n * (t + 1) / nt; ++i) cnt[(size_t)i + 1].store(0, std::memory_order_relaxed);
    if (t == 0) cnt[0].store(0, std::memory_order_relaxed);
  });
  host_parallel(64, [&](int t, int nt) {
    for (int64_t i = n * t / nt; i < n * (t + 1) / nt; ++i) {
      int32_t prev = -1;
      int64_t own = 0;
      for (int64_t e = indptr[i]; e < indptr[i + 1]; ++e) {
        const int32_t j = indices[e];
        if (j < 0 || j >= n) { bad_row.store(i); bad_kind.store(1); return; }
        if (j <= prev) { bad_row.store(i); bad_kind.store(2); return; }
        prev = j;
        if (j < i) continue;
        ++own;
        if (j > i) cnt[(size_t)j + 1].fetch_add(1, std::memory_order_relaxed);
      }
      below[(size_t)i] = own;                                   // (own entries for now)
    }
  });
  RLH_REQUIRE(bad_kind.load() != 1, "rlh_csr_create_upper: column index out of range in row %lld", (long long)bad_row.load());
  RLH_REQUIRE(bad_kind.load() != 2, "rlh_csr_create_upper: the column indices of row %lld are not sorted (or repeat)",
              (long long)bad_row.load());
  // A caller that stores BOTH triangles of a Hermitian matrix (what SciPy users hold) has handed over the operator itself:
  // if every entry below the diagonal is the conjugate of its mirror image above it -- checked entry by entry, one binary
  // search each, on the host threads -- and the two triangles have equally many entries, nothing needs mirroring and no
  // second copy of the matrix is allocated (lap3d 215^3: 0.2 s and 0.8 GB less).  Any mismatch: the upper triangle rules.
  {
    int64_t own_total = 0, mirrored_total = 0;
    for (int64_t i = 0; i < n; ++i) { own_total += below[(size_t)i]; mirrored_total += cnt[(size_t)i + 1].load(std::memory_order_relaxed); }
    const int64_t lower_total = indptr[n] - own_total;
    if (lower_total > 0 && lower_total == mirrored_total) {
      std::atomic<int> mismatch{0};
      host_parallel(64, [&](int t, int nt) {
        for (int64_t i = n * t / nt; i < n * (t + 1) / nt && !mismatch.load(std::memory_order_relaxed); ++i)
          for (int64_t e = indptr[i]; e < indptr[i + 1]; ++e) {
            const int32_t j = indices[e];
            if (j >= i) break;                                   // (sorted: the rest of the row is the upper part)
            const int32_t *b0 = indices + indptr[j], *b1 = indices + indptr[j + 1];
            const int32_t *f = std::lower_bound(b0, b1, (int32_t)i);
            if (f == b1 || *f != (int32_t)i) { mismatch.store(1); break; }
            const T up = conj_of(values[f - indices]);
            if (memcmp(&up, &values[e], sizeof(T)) != 0) { mismatch.store(1); break; }
          }
      });
      if (!mismatch.load()) {
        clk.lap("both triangles given and consistent");
        return rlh_csr_create(out, dtype, n, n, indptr, indices, values);
      }
    }
  }
  std::vector<int64_t> rp((size_t)n + 1, 0);
  for (int64_t i = 0; i < n; ++i) {
    const int64_t mirrored = cnt[(size_t)i + 1].load(std::memory_order_relaxed);
    rp[(size_t)i + 1] = rp[(size_t)i] + mirrored + below[(size_t)i];
    below[(size_t)i] = mirrored;
    cnt[(size_t)i].store(rp[(size_t)i], std::memory_order_relaxed);     // where the next mirrored entry of row i goes
  }
  std::vector<int32_t> idx((size_t)rp[(size_t)n]);
  std::vector<T> val((size_t)rp[(size_t)n]);
  host_parallel(64, [&](int t, int nt) {
    for (int64_t i = n * t / nt; i < n * (t + 1) / nt; ++i) {
      int64_t w = rp[(size_t)i] + below[(size_t)i];               // the row's own entries follow its mirrored ones
      for (int64_t e = indptr[i]; e < indptr[i + 1]; ++e) {
        const int32_t j = indices[e];
        if (j < i) continue;
        idx[(size_t)w] = j; val[(size_t)w] = values[e]; ++w;
        if (j > i) {
          const int64_t d = cnt[(size_t)j].fetch_add(1, std::memory_order_relaxed);
          idx[(size_t)d] = (int32_t)i; val[(size_t)d] = conj_of(values[e]);
        }
      }
    }
  });
  // the mirrored entries of a row arrive in whatever order the threads reached them: ascending column order restored
  host_parallel(64, [&](int t, int nt) {
    std::vector<std::pair<int32_t, T>> tmp;
    for (int64_t i = n * t / nt; i < n * (t + 1) / nt; ++i) {
      const int64_t b0 = rp[(size_t)i], m = below[(size_t)i];
      bool sorted = true;
      for (int64_t k = 1; k < m && sorted; ++k) sorted = idx[(size_t)(b0 + k - 1)] < idx[(size_t)(b0 + k)];
      if (sorted) continue;
      tmp.resize((size_t)m);
      for (int64_t k = 0; k < m; ++k) tmp[(size_t)k] = {idx[(size_t)(b0 + k)], val[(size_t)(b0 + k)]};
      std::sort(tmp.begin(), tmp.end(), [](const std::pair<int32_t, T> &x, const std::pair<int32_t, T> &y) { return x.first < y.first; });
      for (int64_t k = 0; k < m; ++k) { idx[(size_t)(b0 + k)] = tmp[(size_t)k].first; val[(size_t)(b0 + k)] = tmp[(size_t)k].second; }
    }
  });
  clk.lap("mirror the upper triangle");
  return rlh_csr_create(out, dtype, n, n, rp.data(), idx.data(), val.data());
}

// fn(std::integral_constant<int, DT>()) for the element type `dtype` (the callers have checked that it is one of the four)
template <typename F>
static int with_dtype(int dtype, F fn) {
  return dtype == RLH_S ? fn(std::integral_constant<int, RLH_S>()) : dtype == RLH_D ? fn(std::integral_constant<int, RLH_D>())
       : dtype == RLH_C ? fn(std::integral_constant<int, RLH_C>()) : fn(std::integral_constant<int, RLH_Z>());
}

}  // namespace rlh

using namespace rlh;

extern "C" {

int rlh_csr_create(rlh_csr_t *out, int dtype, int64_t n_rows, int64_t n_cols, const int64_t *indptr,
                   const int32_t *indices, const void *values) {
  if (int rc = require_ready()) return rc;
  RLH_REQUIRE(out != nullptr, "rlh_csr_create: null handle pointer");
  *out = nullptr;
  RLH_REQUIRE(dtype_valid(dtype), "rlh_csr_create: unknown dtype %d", dtype);
  RLH_REQUIRE(n_rows >= 0 && n_cols >= 0 && n_cols < ((int64_t)1 << 31), "rlh_csr_create: bad shape");
  RLH_REQUIRE(indptr != nullptr, "rlh_csr_create: null indptr");
  PhaseClock clk;
  const int64_t nnz = indptr[n_rows] - indptr[0];
  RLH_REQUIRE(indptr[0] == 0 && nnz >= 0, "rlh_csr_create: indptr must be 0-based and non-decreasing");
  RLH_REQUIRE(nnz == 0 || (indices && values), "rlh_csr_create: null indices/values");
  for (int64_t r = 0; r < n_rows; ++r)
    RLH_REQUIRE(indptr[r + 1] >= indptr[r], "rlh_csr_create: indptr decreases at row %lld", (long long)r);
  for (int64_t e = 0; e < nnz; ++e)
    RLH_REQUIRE(indices[e] >= 0 && indices[e] < n_cols, "rlh_csr_create: column index %d out of range at entry %lld",
                indices[e], (long long)e);
  clk.lap("argument checks");
  rlh_csr *h = new rlh_csr();
  h->dtype = dtype; h->n_rows = n_rows; h->n_cols = n_cols; h->nnz = nnz;
  // Layout (RLH_SPMM_FORMAT=sell|well|wide overrides the choice and the locality test; read per
  // handle so tests can cover all three): rows of at most 8 entries of a real type -> the 1024-row
  // windowed layout; otherwise, or when that one does not qualify -> the 256-row interleaved
  // layout; no column locality at all -> sliced ELL.
  const char *fmt = getenv("RLH_SPMM_FORMAT");
  const bool want_sell = fmt && !strcmp(fmt, "sell"), force_well = fmt && !strcmp(fmt, "well");
  const bool force_wide = fmt && !strcmp(fmt, "wide");
  int rc = 0;
  if (!want_sell && !force_wide)
    rc = with_dtype(dtype, [&](auto dt) {
      constexpr bool cplx = DType<decltype(dt)::value>::cplx;       // (the complex types: stacks only, never forced)
      return well_build<decltype(dt)::value>(h, indptr, indices, values, force_well && !cplx, cplx);
    });
  if (rc == 0 && h->well_blocks == 0 && !want_sell) rc = wide_build(h, indptr, indices, values, force_well || force_wide);
  if (rc == 0 && h->well_blocks == 0 && h->wide_blocks == 0)
    rc = with_dtype(dtype, [&](auto dt) { return csr_build<decltype(dt)::value>(h, indptr, indices, values); });
  if (rc) { rlh_csr_destroy(h); return rc; }
  *out = h;
  return 0;
}

int rlh_csr_create_upper(rlh_csr_t *out, int dtype, int64_t n, const int64_t *indptr, const int32_t *indices,
                         const void *values) {
  if (int rc = require_ready()) return rc;
  RLH_REQUIRE(out != nullptr, "rlh_csr_create_upper: null handle pointer");
  *out = nullptr;
  RLH_REQUIRE(dtype_valid(dtype), "rlh_csr_create_upper: unknown dtype %d", dtype);
  RLH_REQUIRE(n >= 0 && n < ((int64_t)1 << 31) && indptr != nullptr && indptr[0] == 0, "rlh_csr_create_upper: bad matrix");
  for (int64_t r = 0; r < n; ++r)
    RLH_REQUIRE(indptr[r + 1] >= indptr[r], "rlh_csr_create_upper: indptr decreases at row %lld", (long long)r);
  RLH_REQUIRE(indptr[n] == 0 || (indices && values), "rlh_csr_create_upper: null indices/values");
  return with_dtype(dtype, [&](auto dt) {
    using T = typename DType<decltype(dt)::value>::T;
    return csr_from_upper<T>(out, dtype, n, indptr, indices, (const T *)values);
  });
}

}  // extern "C"
