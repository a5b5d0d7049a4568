// dafs_amd/csrc/reliability.h -- launcher of reliability.hip (dafs_hip_alignment_reliabilities)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sparse_view.h"

namespace dafs {

// One alignment of a chunk: where its rows, cells and columns lie in the chunk's arrays.
struct rel_aln {
  uint64_t row0;        // its first row in rows[]
  uint64_t cell0;       // its first cell in mask[] and pos[] (n * len of them, row-major)
  uint64_t col0;        // its first column in ss[], col_rel[], pair_rel[] and pair_rows[]
  uint32_t n, len;
  uint32_t all_wanted;  // every row is wanted: col_rel is computed (otherwise it is NaN)
  uint32_t pad;
};

// One row; the rows of an alignment lie one after another in ascending sequence order.
struct rel_row {
  uint64_t res0;  // its first residue in col_of[]
  uint64_t rel0;  // its first residue in res_rel[], which holds the wanted rows only (unused for another row)
  uint32_t aln;   // its alignment in alns[]
  uint32_t seq;
  uint32_t nres;  // its residues
  uint32_t pad;
};

// All pointers are device memory.
struct rel_args {
  mp_store_dev mp;           // the matching store to read (unused when no alignment has a second row)
  bp_store_dev bp;           // the base-pairing store to read (unused without ss)
  const rel_aln* alns;       // [naln]
  const rel_row* rows;       // [nrows]
  const uint8_t* mask;       // 1 = residue
  const uint2* blocks;       // [nblocks] (row, first residue) of each block of 64 residues of a wanted row
  const uint2* col_blocks;   // [ncol_blocks] (alignment, first column) of each block of 64 columns
  const uint32_t* ss;        // per column: left partner -> right column, DAFS_HIP_NONE otherwise; null: no pairs
  uint32_t* pos;             // written by k_rel_pos: residue index at each cell, DAFS_HIP_NONE for a gap
  uint32_t* col_of;          // written by k_rel_pos: column of each residue
  double* res_rel;
  double* col_rel;
  double* pair_rel;
  uint32_t* pair_rows;
  uint32_t nrows, nblocks, ncol_blocks;
};

// k_rel_pos, then k_rel_residue and k_rel_column, one launch each for the whole chunk, all on st
int rel_launch(const rel_args& a, hipStream_t st);

}  // namespace dafs
