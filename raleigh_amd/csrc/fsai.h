// What fsai.hip (the build, rlh_fsai_*) and fsai_apply.hip (the two-kernel application, rlh_fsapply_*) share: the
// handle of an approximate inverse (both take the exclusive scan from device_build.h).
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
  double prefilter = 0;             // prefiltration: the threshold (0: none) and the lower entries of A it found weak
  int64_t weak = 0;
  int64_t updates = 0;              // rlh_fsvalues_update*: the successful ones and the device seconds of the last
  double update_seconds = 0;
  rlh_spd_t spd = nullptr;          // G and G^H with their partitions
  rlh::DevBuf<char> work;           // the n x m block between the two products
};
