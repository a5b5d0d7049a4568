// dafs_amd/csrc/families.h -- the device gather behind dafs_hip_families_from and dafs_hip_pairs_from (families.hip)
#pragma once
#include <stdint.h>

struct dafs_hip_ctx;

namespace dafs {
// dst becomes the nfam families member[first[f] .. first[f + 1]) of src's sequences.  The callers have checked the arguments:
// distinct contexts of one device, no folding in flight, src one family with valid raw stores that hold every pair the
// families need, first / member well-formed (members strictly ascending inside a family), counts within 31 bits.
int families_gather(dafs_hip_ctx* dst, const dafs_hip_ctx* src, uint32_t nfam, const uint32_t* first, const uint32_t* member);
}  // namespace dafs
