// dafs_amd/csrc/mix64.h -- the splitmix64 finaliser of DESIGN.md section 13 and the golden-ratio step that spreads its
// arguments, once for the host and the kernels.  Nothing from HIP unless hipcc compiles it: call_host.h includes it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DAFS_MIX_FN __host__ __device__ __forceinline__
#else
#define DAFS_MIX_FN inline
#endif

namespace dafs {

constexpr uint64_t kMixGolden = 0x9E3779B97F4A7C15ull;

DAFS_MIX_FN uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

}  // namespace dafs

#undef DAFS_MIX_FN
