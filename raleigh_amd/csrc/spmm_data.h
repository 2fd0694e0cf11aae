// What other translation units may ask of a sparse data operator (rlh_spd, spmm_data.hip) beyond the C ABI.
#pragma once

#include "common.h"

namespace rlh {

// The CSR arrays of one orientation of the operator in DEVICE memory (transp 0: A, 1: A^H): int64 row pointers,
// int32 columns, values of the operator's type.  They belong to the handle and live as long as it does.
struct SpdArrays {
  int64_t rows = 0, cols = 0, nnz = 0;
  const int64_t *indptr = nullptr;
  const int32_t *idx = nullptr;
  const void *val = nullptr;
};
SpdArrays spd_arrays(const rlh_spd *h, int transp);

}  // namespace rlh
