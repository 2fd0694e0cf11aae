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

// New values on the structure the operator has: d_values (DEVICE memory, nnz values of the operator's type in the
// order of A's entries) are copied into A's value array and their conjugates written to the matching places of A^H --
// the bits rlh_spd_create_device would make from the same A.  Index arrays and partitions are not touched; nothing is
// allocated.  Asynchronous on the library stream: d_values must live until the stream has passed this point.
int spd_set_values(rlh_spd *h, const void *d_values);

}  // namespace rlh
