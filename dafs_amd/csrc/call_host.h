// dafs_amd/csrc/call_host.h -- what the host side of the per-call entry points (capi_*.cpp) shares and needs no device for:
// the layout of a workspace, the environment knobs, the refusal, and the few host computations that a bit-exactness contract
// wants to exist once.  Nothing from HIP: tests/host_call_main.cpp compiles it with a plain compiler.
#pragma once
#include <errno.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <vector>

#include "../../include/dafs_hip.h"
#include "last_error.h"
#include "mix64.h"  // dafs::mix64, the mix the kernels draw with

namespace dafs {

// Offsets of the pieces of one device block, each piece rounded up to 256 bytes; a piece of no bytes takes no room.
struct carve {
  size_t top = 0;
  size_t take(size_t bytes) { const size_t at = top; top += (bytes + 255) & ~(size_t)255; return at; }
  size_t bytes() const { return top; }
  size_t reserve_bytes() const { return top + 256; }  // what a call reserves of c->work: the pieces and one line of slack
};

// An integer knob of tests and tuning: the value of `name` when the whole string is a decimal number in lo..hi, `fallback`
// when it is unset or anything else (empty, a sign, a blank, a trailing letter, out of range).
inline uint64_t env_uint(const char* name, uint64_t lo, uint64_t hi, uint64_t fallback) {
  const char* e = getenv(name);
  if (!e || *e < '0' || *e > '9') return fallback;
  char* end = nullptr;
  errno = 0;
  const unsigned long long v = strtoull(e, &end, 10);
  return *end || errno == ERANGE || v < lo || v > hi ? fallback : (uint64_t)v;
}
// A form that NAME=0 switches off; every other value leaves it on.
inline bool env_off(const char* name) { return env_uint(name, 0, 0, 1) == 0; }
// A non-negative real knob (DAFS_NJ_BOOT_GUARD)
inline double env_double(const char* name, double fallback) {
  if (const char* e = getenv(name)) {
    char* end = nullptr;
    const double v = strtod(e, &end);
    if (end != e && v >= 0.0) return v;
  }
  return fallback;
}

inline int refuse(const char* what) {
  set_last_error(what);
  return DAFS_HIP_EINVAL;
}

// A structure over L columns: left column -> right column, DAFS_HIP_NONE elsewhere, each column in at most one pair.
inline bool structure_ok(const uint32_t* ss, uint32_t L, std::vector<uint8_t>& used) {
  used.assign(L, 0);
  for (uint32_t col = 0; col < L; ++col) {
    const uint32_t p = ss[col];
    if (p == DAFS_HIP_NONE) continue;
    if (p <= col || p >= L || used[col] || used[p]) return false;
    used[col] = used[p] = 1;
  }
  return true;
}

// DESIGN.md section 22, "Distances from an alignment": the distance of two rows with `mism` differing of `comp` compared
// columns.  The Jukes-Cantor value is quantised to 2^-20 the way LNQ is in section 13, so that an ulp of log() cannot move a
// bit: it would have to carry -0.75 * log(x) * 2^20 + 0.5 across an integer.
inline double nj_pair_distance(int model, uint32_t mism, uint32_t comp) {
  const double kQ = 1048576.0, kCapK = 3.0 * 1048576.0;
  if (model == DAFS_NJ_P) return comp ? (double)mism / (double)comp : 1.0;
  if (comp == 0 || 4 * (uint64_t)mism >= 3 * (uint64_t)comp) return 3.0;
  const double x = 1.0 - (4.0 * (double)mism) / (3.0 * (double)comp);
  double k = floor(-0.75 * log(x) * kQ + 0.5);
  if (!(k < kCapK)) k = kCapK;
  return k / kQ;
}

}  // namespace dafs
