// What fsai.hip (the build, rlh_fsai_*) and fsai_apply.hip (the two-kernel application, rlh_fsapply_*) share: the
// handle of an approximate inverse and the host side of the exclusive scan of device_build.h.
#pragma once

#include "device_build.h"
#include "spmm_data.h"

struct rlh_fsai {
  int dtype = 0;
  int64_t n = 0, nnz = 0, truncated = 0;
  int longest = 0, levels = 1, steps = 0, step_size = 0;
  double setup_seconds = 0;
  double drop = 0;                  // post-filtration: the threshold (0: none) and the entries it removed
  int64_t removed = 0;
  int64_t updates = 0;              // rlh_fsvalues_update*: the successful ones and the device seconds of the last
  double update_seconds = 0;
  rlh_spd_t spd = nullptr;          // G and G^H with their partitions
  rlh::DevBuf<char> work;           // the n x m block between the two products
};

namespace rlh {
namespace {

// out[0 .. n] = exclusive scan of in[0 .. n) on the library stream; bsum: (n + kScanTile - 1) / kScanTile + 1 entries
int exclusive_scan(int64_t n, const int64_t *in, int64_t *bsum, int64_t *out) {
  hipStream_t st = ctx().stream;
  const int64_t nb = (n + kScanTile - 1) / kScanTile;
  hipLaunchKernelGGL(scan_tile_sums, dim3((unsigned)nb), dim3(kBlock), 0, st, n, in, bsum);
  hipLaunchKernelGGL(scan_of_sums, dim3(1), dim3(kBlock), 0, st, nb, bsum);
  hipLaunchKernelGGL(scan_tiles, dim3((unsigned)nb), dim3(kBlock), 0, st, n, nb, in, bsum, out);
  RLH_HIP(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace rlh
