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

// DESIGN.md section 5.1, "Sweep 2p": the cut of the pair-HMM kernel's candidate pick.  pair_cut(th) is a value c <= -0.5
// such that every float v with -16 < v < c has EXP(v) <= th, EXP being the reference's quartic pieces (ScoreType.h:37-57,
// pc_math.h: evaluated in double, narrowed to float; 0 for v <= -16).  The pieces are not known to be monotone across their
// seams, so the bound is computed, not assumed: on the grid g_k = -16 + k / 1024 (every seam is a grid point, and an interval
// (g_k-1, g_k] lies in one piece) the piece's quartic P obeys  max over [a, b] of P <= max(P(a), P(b)) + max|P''| (b - a)^2 / 8,
// with |P''| bounded term by term (and max = P(b) where a term-by-term lower bound of P' is positive, which makes the cut
// -0.5 for every th above EXP(-0.5)); M[k] is the running maximum of those bounds plus 1e-12 for the rounding of the double
// Horner form (narrowing to float is monotone, and th is a float).  The cut is the largest g_k <= -0.5 with M[k] <= th:
// at most 1/1024 and the bound's slack (< 3e-7 in EXP) below the best possible one.
inline float pair_cut(float th) {
  static const std::vector<double> M = [] {
    static const double e[5][5] = {  // pieces (-1, -1/2], (-2, -1], (-4, -2], (-8, -4], (-16, -8]: k4 .. k0
        {0.01973899026052090000, 0.13822379685007000000, 0.48056651562365000000, 0.99326940370383500000, 0.99906756856399500000},
        {0.00940528203591384000, 0.09414963667859410000, 0.40825793595877300000, 0.93933625499130400000, 0.98369508190545300000},
        {0.00217245711583303000, 0.03484829428350620000, 0.22118199801337800000, 0.67049462206469500000, 0.83556950223398500000},
        {0.00012398771025456900, 0.00349155785951272000, 0.03727721426017900000, 0.17974997741536900000, 0.33249299994217400000},
        {0.00000051741713416603, 0.00002721456879608080, 0.00053418601865636800, 0.00464101989351936000, 0.01507447981459420000}};
    const int n = (16 * 1024) - 512;  // grid points above -16 up to -0.5
    std::vector<double> m((size_t)n + 1, 0.0);
    const double h = 1.0 / 1024.0;
    for (int k = 1; k <= n; ++k) {
      const double a = -16.0 + (k - 1) * h, b = -16.0 + k * h;
      const double* q = e[b <= -8.0 ? 4 : b <= -4.0 ? 3 : b <= -2.0 ? 2 : b <= -1.0 ? 1 : 0];  // the piece of (a, b]
      const double pa = (((q[0] * a + q[1]) * a + q[2]) * a + q[3]) * a + q[4];
      const double pb = (((q[0] * b + q[1]) * b + q[2]) * b + q[3]) * b + q[4];
      const double x = -a;  // the largest |v| of the interval
      const double d2 = 12.0 * q[0] * x * x + 6.0 * q[1] * x + 2.0 * q[2];
      const double d1 = q[3] - 2.0 * q[2] * x - 4.0 * q[0] * x * x * x;  // P' >= d1 on [a, b]: where d1 > 0, P rises to P(b)
      const double bound = (d1 > 0.0 ? pb : (pa > pb ? pa : pb) + d2 * h * h / 8.0) + 1e-12;
      m[(size_t)k] = bound > m[(size_t)k - 1] ? bound : m[(size_t)k - 1];
    }
    return m;
  }();
  size_t lo = 0, hi = M.size() - 1;  // the largest k with M[k] <= th (M[0] = 0; th < 0 or NaN: -16, every cell a candidate)
  if (!(M[hi] <= (double)th)) {
    while (hi - lo > 1) {
      const size_t mid = (lo + hi) / 2;
      if (M[mid] <= (double)th) lo = mid; else hi = mid;
    }
    hi = lo;
  }
  return (float)(-16.0 + (double)hi / 1024.0);
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
