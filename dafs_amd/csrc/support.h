// dafs_amd/csrc/support.h -- launcher of support.hip (dafs_hip_structure_support)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sparse_view.h"

namespace dafs {

// one row of one alignment; the offsets count entries of the arrays of sup_args
struct sup_row {
  uint64_t mask_off;  // first byte of the row's mask
  uint64_t pos_off;   // first entry of the row's column -> residue map
  uint64_t ss_off;    // first entry of its alignment's structure
  uint32_t len;       // columns of its alignment
  uint32_t seq;       // its sequence
  uint32_t code_off;  // first residue code of that sequence
  uint32_t pad;
};

// All pointers are device memory.
struct sup_args {
  bp_store_dev bp;       // the base-pairing store to read
  const sup_row* rows;   // [nrows]
  const uint8_t* mask;   // 1 = residue; every row checked to place exactly the residues of its sequence
  const uint32_t* ss;    // per alignment: left column -> right column (> left, < len, checked), DAFS_HIP_NONE otherwise
  const uint8_t* codes;  // the context's residue class codes (A C G U T N other)
  uint32_t* pos;         // workspace: per row and column the residue index, DAFS_HIP_NONE for a gap
  uint32_t* both;        // [nrows]
  uint32_t* canonical;   // [nrows]
  uint32_t* half;        // [nrows]
  double* expected;      // [nrows]
  uint32_t nrows;
};

// k_ss_support on st: one wavefront per row
int sup_launch(const sup_args& a, hipStream_t st);

}  // namespace dafs
