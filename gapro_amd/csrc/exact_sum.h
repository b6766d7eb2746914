// Exact, order-independent sums: every term is converted to a 64-bit integer at one scale 2^k, the terms
// are added with integer atomics (any order gives the same bits), and the mean is taken once in float64.  The rule for
// k, the conversion and the mean exist here and nowhere else on the device; oracle/gen_ps_oracle.py:fixed_point_shift
// is the same rule as the spec.  Also the eight-lanes-per-point feature accumulation of the pooling kernels
// (partition.hip k_pool / k_pool_lds, trainset.hip k_ts_accum) and their box test.
#pragma once
#include <math.h>

#include <hip/hip_runtime.h>

// Exponent k with |rint(x 2^k)| n < 2^61 for n terms of magnitude <= absmax: 61 - e - ceil(log2 n), absmax = m 2^e with
// m in [0.5, 1), held to +-1000 (ldexp stays far from overflow).  0 for an absmax that is zero, negative or not finite.
__host__ __device__ inline int fixed_point_shift(double absmax, long long n) {
  if (!(absmax > 0.0) || !isfinite(absmax)) return 0;
  int e;
  (void)frexp(absmax, &e);
  const int lg = n > 1 ? 64 - __builtin_clzll((unsigned long long)(n - 1)) : 0;
  const int k = 61 - e - lg;
  return k < -1000 ? -1000 : (k > 1000 ? 1000 : k);
}

// one term: x 2^k rounded to the nearest integer, ties to even (x finite and inside the rule above)
__host__ __device__ inline long long to_fixed(double x, int k) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __double2ll_rn(ldexp(x, k));
#else
  return llrint(ldexp(x, k));  // the host's default rounding mode
#endif
}

// the mean of `count` terms summed at scale 2^k, in float64: the caller rounds it once to float32
__host__ __device__ inline double fixed_mean(long long sum, int k, double count) { return ldexp((double)sum, -k) / count; }

// ---- feature accumulation: eight lanes per point ------------------------------------------------------------------
// Lane lane_k of a point's eight adds features lane_k, lane_k + 8, ... of the point to dst_row (LDS or global: the
// address space follows the caller's pointer once inlined); lane d % 8 adds the point count at the call site.
constexpr int kLanesPerPoint = 8;

__device__ __forceinline__ void accumulate_features(unsigned long long* dst_row, const float* f, int d, int lane_k,
                                                    int shift) {
  for (int c = lane_k; c < d; c += kLanesPerPoint)
    atomicAdd(&dst_row[c], (unsigned long long)to_fixed((double)f[c], shift));
}

// The same when the wave's eight points share dst_row: the terms are summed across the eight point groups by shuffles
// and the `head` lanes (0 .. 7 of the wave) issue one atomic per feature instead of eight to the same address.  Every
// lane of the wave must call it.
__device__ __forceinline__ void accumulate_features_wave8(unsigned long long* dst_row, const float* f, int d, int lane_k,
                                                          int shift, bool head) {
  for (int c0 = 0; c0 < d; c0 += kLanesPerPoint) {
    const int c = c0 + lane_k;
    long long q = c < d ? to_fixed((double)f[c], shift) : 0ll;
    q += __shfl_down(q, 8, 64);
    q += __shfl_down(q, 16, 64);
    q += __shfl_down(q, 32, 64);
    if (head && c < d) atomicAdd(&dst_row[c], (unsigned long long)q);
  }
}

// 1 for a point (x, y, z) inside the closed box bx = {lo xyz, hi xyz}, else 0 (an int: the wave-folded callers add it)
__device__ __forceinline__ int in_box(const double* bx, double x, double y, double z) {
  return (x >= bx[0]) & (y >= bx[1]) & (z >= bx[2]) & (x <= bx[3]) & (y <= bx[4]) & (z <= bx[5]);
}
