// dafs_amd/csrc/reliability.h -- launcher of reliability.hip (dafs_hip_alignment_reliability)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sparse_view.h"

namespace dafs {

// All pointers are device memory.  Rows are in ascending sequence order; residue arrays hold the rows one after another.
struct rel_args {
  mp_store_dev mp;          // the matching store to read (unused with n = 1)
  bp_store_dev bp;          // the base-pairing store to read (unused without ss)
  const uint32_t* seq;      // [n] sequence of each row
  const uint64_t* res_off;  // [n + 1] first residue of each row
  const uint2* blocks;      // [nblocks] (row, first residue) of each block of 64 residues
  const uint32_t* ss;       // [len] left partner -> right column, DAFS_HIP_NONE otherwise; null: no pairs
  uint32_t* pos;            // [n * len] written by k_rel_pos: residue index at each column, DAFS_HIP_NONE for a gap
  uint32_t* col_of;         // [res_off[n]] written by k_rel_pos: column of each residue
  double* res_rel;          // [res_off[n]]
  double* col_rel;          // [len]
  double* pair_rel;         // [len]
  uint32_t* pair_rows;      // [len]
  uint32_t n, len, nblocks;
};

// k_rel_pos from mask ([n * len] bytes, 1 = residue), then k_rel_residue and k_rel_column, all on st
int rel_launch(const rel_args& a, const uint8_t* mask, hipStream_t st);

}  // namespace dafs
