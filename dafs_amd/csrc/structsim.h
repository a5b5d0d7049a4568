// dafs_amd/csrc/structsim.h -- launch interface of the structural pair score (structsim.hip; dafs_hip_structure_scores and
// dafs_hip_similarity_scored in capi_structsim.cpp; the contract, to the bit).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sparse_view.h"

namespace dafs {

// A pair with this many terms or more is refused: below it the sum of terms, each at most 2^40, stays under 2^64.
constexpr uint64_t kStructMaxTerms = 1ull << 24;

constexpr uint32_t kStructThreads = 256;  // both kernels: four wavefronts per workgroup, one task (or sequence) per wavefront
// k_struct_sim: the words of LDS a wavefront has for its copies of the rows of bp[y] and mp[x][y] (10 KiB; 40 KiB a workgroup,
// four workgroups a compute unit).  A pair of 120-nt sequences at the run's thresholds takes about 1 800.
constexpr uint32_t kStructLdsWords = 2560;

// k_struct_sim over the ntasks tasks of a resident un-relaxed matching store: task t holds mp[x][y] of task_xy[t] = {x, y},
// x < y, whatever pair ids the store's shard covers.  out[t] = {T, terms}.  lds_words <= kStructLdsWords: what a wavefront may
// use of its LDS region (0: every row is read where it lies; it changes no result).  No allocation, no wait.
int struct_sim_launch(const mp_store_dev& mp, const bp_store_dev& bp, const uint2* task_xy, uint32_t ntasks, uint32_t lds_words, ulonglong2* out,
                      hipStream_t st);

// k_struct_w: W[x] of every sequence's base-pairing rows.  len: the sequence lengths on the device.
int struct_w_launch(const bp_store_dev& bp, const uint32_t* len, uint32_t nseq, unsigned long long* W, hipStream_t st);

}  // namespace dafs
