// dafs_amd/csrc/nj_steps.h -- the steps of one neighbour join on the device, each stated once (the contract, to the bit, in
// DESIGN.md section 22; tests/nj_ref.py is the plain restatement).  nj.hip runs them as launches in stream order with R, node
// and the rows' tuples in global memory, k_nj_batch (nj_boot.hip) as a loop between __syncthreads() with them in LDS; the
// arithmetic of a join, its comparisons and its orders of summation are here and nowhere else.  The functions are inlined
// and take plain pointers: what a kernel knows of its own arguments (__restrict__ in nj.hip, none for k_nj_batch's working
// copy and LDS state) stays what it was.
//
// A retired slot b keeps R[b] = NaN: Q(i, b) is then NaN, which no comparison prefers, so the scan reads no activity flag.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dafs {
namespace nj {

constexpr uint32_t kNone = 0xFFFFFFFFu;

__device__ __forceinline__ double pos_inf() { return __longlong_as_double(0x7FF0000000000000ll); }
__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7FF8000000000000ll); }
__device__ __forceinline__ uint32_t nonfinite(double v) {
  return ((unsigned long long)__double_as_longlong(v) & 0x7FF0000000000000ull) == 0x7FF0000000000000ull ? 1u : 0u;
}

// (value ascending, key ascending); a NaN is never better, and (+inf, kNone) is "no candidate"
__device__ __forceinline__ bool better(double v1, uint32_t k1, double v2, uint32_t k2) { return v1 < v2 || (v1 == v2 && k1 < k2); }

__device__ __forceinline__ void wave_best(double& v, uint32_t& k) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const double ov = __shfl_xor(v, d, 64);
    const uint32_t ok = __shfl_xor(k, d, 64);
    if (better(ov, ok, v, k)) { v = ov; k = ok; }
  }
}

// the best tuple of a workgroup of WAVES wavefronts, in wavefront 0 (one __syncthreads())
template <uint32_t WAVES>
__device__ __forceinline__ void group_best(double& v, uint32_t& k, double* red_v, uint32_t* red_k) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  wave_best(v, k);
  if (lane == 0) { red_v[wave] = v; red_k[wave] = k; }
  __syncthreads();
  if (wave == 0) {
    v = lane < WAVES ? red_v[lane] : pos_inf();
    k = lane < WAVES ? red_k[lane] : kNone;
    wave_best(v, k);
  }
}

// lane l's value in every lane (l is a constant after unrolling: two v_readlane_b32)
__device__ __forceinline__ double lane_value(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

// A wavefront's row of the symmetric working copy D from the upper triangle of `in` (0 on the diagonal); the lane's count of
// non-finite entries, each counted once, from the row that owns it.
__device__ __forceinline__ uint32_t sym_row(uint32_t n, uint32_t row, uint32_t lane, const double* in, double* D) {
  double* out = D + (size_t)row * n;
  uint32_t bad = 0;
  for (uint32_t j = lane; j < n; j += 64) {
    double v = 0.0;
    if (j > row) {
      v = in[(size_t)row * n + j];
      bad += nonfinite(v);
    } else if (j < row) {
      v = in[(size_t)j * n + row];
    }
    out[j] = v;
  }
  return bad;
}

// slot i as a leaf, its length and that of join node n + i zeroed (the root's stays)
__device__ __forceinline__ void leaf(uint32_t n, uint32_t i, int32_t* node, int32_t* left, int32_t* right, double* length) {
  node[i] = (int32_t)i;
  left[i] = -1;
  right[i] = -1;
  length[i] = 0.0;
  if (i + 1 < n) length[n + i] = 0.0;
}

// R[k] at the start: the running sum of column k of D in ascending row order (D is symmetric, so the threads of a wavefront
// read neighbouring words; the diagonal's +0 leaves every bit of the sum alone)
__device__ __forceinline__ double column_sum(uint32_t n, uint32_t k, const double* D) {
  double s = 0.0;
#pragma unroll 8
  for (uint32_t j = 0; j < n; ++j) s += D[(size_t)j * n + k];
  return s;
}

// A wavefront's scan of row i: Q(i, j) over j > i with c = others(m), into the lane's tuple so far, which it returns (by
// value: a tuple passed by reference cost k_nj_pick two registers).  j ascends within a lane and `<` is strict, so the first
// of equals stays.  The key a lane keeps is j, or i << 16 | j for a caller that scans several rows into one tuple (PAIR_KEY).
struct best {
  double q;
  uint32_t k;
};
// m - 2 of Q and of the branch lengths, for m active slots
__device__ __forceinline__ double others(uint32_t m) { return (double)(m - 2); }
template <int UNROLL, bool PAIR_KEY>
__device__ __forceinline__ best scan_row(uint32_t n, uint32_t i, uint32_t lane, double c, const double* D, const double* R, best b) {
  const double* Di = D + (size_t)i * n;
  const double Ri = R[i];
#pragma unroll UNROLL
  for (uint32_t j = i + 1 + lane; j < n; j += 64) {
    const double q = (c * Di[j] - Ri) - R[j];  // NaN at a retired j: never below anything
    if (q < b.q) { b.q = q; b.k = PAIR_KEY ? (i << 16) | j : j; }
  }
  return b;
}

// The pair as picked, settled by one thread.  a >= n says that no Q lay below +inf: the pair is then the candidate the scan
// starts from, the first two active slots.  Whatever could index beyond the arrays becomes (kNone, kNone).
struct slots {
  uint32_t a, b;
};
__device__ __forceinline__ slots settle_pair(uint32_t n, const int32_t* node, uint32_t a, uint32_t b) {
  if (a >= n) {
    a = b = kNone;
    for (uint32_t i = 0; i < n && b == kNone; ++i) {
      if (node[i] < 0) continue;
      if (a == kNone) a = i; else b = i;
    }
  }
  if (a >= n || b >= n || a >= b || node[a] < 0 || node[b] < 0) a = b = kNone;
  return {a, b};
}

// Row and column a of D and R[k] after the join of (a, b), for the slots k that take part, by a workgroup of THREADS threads;
// a wavefront takes whole chunks of 64 slots.  row_u gets per slot the new D(a, k), +0 where k takes no part, row_part per
// chunk the mask of the slots that do.  The thread's count of non-finite values written.
template <uint32_t THREADS>
__device__ __forceinline__ uint32_t update_row(uint32_t n, uint32_t a, uint32_t b, double dab, double* D, double* R, const int32_t* node,
                                               double* row_u, unsigned long long* row_part) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double* Da = D + (size_t)a * n;
  const double* Db = D + (size_t)b * n;
  uint32_t bad = 0;
  for (uint32_t base = wave * 64; base < n; base += THREADS) {
    const uint32_t k = base + lane;
    const bool part = k < n && k != a && k != b && node[k] >= 0;
    double u = 0.0;
    if (part) {
      const double p = Da[k], q = Db[k];
      u = 0.5 * ((p + q) - dab);
      const double r = ((R[k] - p) - q) + u;
      R[k] = r;
      Da[k] = u;
      D[(size_t)k * n + a] = u;
      bad += nonfinite(u) + nonfinite(r);
    }
    row_u[k] = u;
    const unsigned long long m_part = __ballot(part);
    if (lane == 0) row_part[base >> 6] = m_part;
  }
  return bad;
}

// The join itself, by one thread, with R and node still as before the join: the two branch lengths and the children of join
// node n + t; m = n - t slots are active.  The count of non-finite lengths.
__device__ __forceinline__ uint32_t join_pair(uint32_t n, uint32_t t, uint32_t m, uint32_t a, uint32_t b, double dab, const double* R,
                                              const int32_t* node, int32_t* left, int32_t* right, double* length) {
  double la = 0.5 * dab;
  if (m > 2) la = la + (R[a] - R[b]) / (2.0 * others(m));
  const double lb = dab - la;
  const int32_t na = node[a], nb = node[b];
  length[na] = la;
  length[nb] = lb;
  left[n + t] = na;
  right[n + t] = nb;
  return nonfinite(la) + nonfinite(lb);
}

// R[a]: the running sum of the new row a over the remaining active k, ascending: a chain of dependent additions, the one part
// of a join that no second thread can help with.  One wavefront walks the row in LDS, a chunk of 64 slots per step with the
// next one already on its way; every lane carries the same sum.  A well-filled chunk adds all 64 lanes' values in turn (a slot
// that takes no part holds +0, which changes no bit of a sum that started at +0), a sparse one only the slots of its mask.
__device__ __forceinline__ double row_sum(uint32_t chunks, uint32_t lane, const double* row_u, const unsigned long long* row_part) {
  double s = 0.0;
  double v = row_u[lane];
  unsigned long long m_part = row_part[0];
  for (uint32_t c = 0; c < chunks; ++c) {
    const double v_next = row_u[(size_t)(c + 1) * 64 + lane];  // the array ends in one chunk of padding
    const unsigned long long m_next = row_part[c + 1];
    unsigned long long todo = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(m_part >> 32)) << 32) |
                              (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)m_part);
    if (__popcll(todo) >= 24) {
#pragma unroll
      for (int l = 0; l < 64; ++l) s += lane_value(v, l);
    } else {
      while (todo) {
        const int l = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        s += lane_value(v, l);
      }
    }
    v = v_next;
    m_part = m_next;
  }
  return s;
}

// slot a becomes join node n + t with R[a] = s, slot b retires; 1 when s is not finite
__device__ __forceinline__ uint32_t retire(uint32_t n, uint32_t t, uint32_t a, uint32_t b, double s, double* R, int32_t* node) {
  R[a] = s;
  R[b] = quiet_nan();
  node[a] = (int32_t)(n + t);
  node[b] = -1;
  return nonfinite(s);
}

}  // namespace nj
}  // namespace dafs
