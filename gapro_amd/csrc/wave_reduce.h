// Wave-level reductions of the integer kernels: every one is a width-64 xor butterfly with offsets 32 .. 1, so every lane
// ends with the result.  The float64 sum's order is part of the consumer losses' bits (consumer.hip); the integer forms
// and min / max do not depend on the order.  Also the workgroup fold of the scene statistics (partition.hip).
#pragma once
#include <math.h>

#include <hip/hip_runtime.h>

template <typename T>
__device__ inline T wave_sum(T v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ inline long long wave_sum(long long v) {  // wraps like the integer atomic behind it would
  for (int o = 32; o > 0; o >>= 1) v = (long long)((unsigned long long)v + (unsigned long long)__shfl_xor(v, o, 64));
  return v;
}

template <typename T>
__device__ inline T wave_min(T v) {
  for (int o = 32; o > 0; o >>= 1) {
    const T t = __shfl_xor(v, o, 64);
    v = t < v ? t : v;
  }
  return v;
}
template <typename T>
__device__ inline T wave_max(T v) {
  for (int o = 32; o > 0; o >>= 1) {
    const T t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}
// the floating-point forms drop a NaN, as fmin / fmax do
__device__ inline double wave_min(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ inline double wave_max(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ inline float wave_max(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ inline int wave_or(int v) {
  for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
  return v;
}

// ---- scene statistics (partition.hip k_stats / k_stats_final) ------------------------------------------------------
struct StatsPartial {
  double mn[3], mx[3];
  long long smin, smax;
  float fabsmax;
  int pad;
};

__device__ inline StatsPartial stats_identity() {
  return {{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}, 0x7fffffffffffffffLL,
          -0x7fffffffffffffffLL - 1, 0.f, 0};
}

__device__ inline void stats_merge(StatsPartial& p, const StatsPartial& q) {
  for (int k = 0; k < 3; ++k) { p.mn[k] = fmin(p.mn[k], q.mn[k]); p.mx[k] = fmax(p.mx[k], q.mx[k]); }
  p.smin = q.smin < p.smin ? q.smin : p.smin;
  p.smax = q.smax > p.smax ? q.smax : p.smax;
  p.fabsmax = fmaxf(p.fabsmax, q.fabsmax);
}

// every thread's partial of a workgroup of kThreads threads -> the workgroup's, returned in thread 0 (only there)
template <int kThreads>
__device__ inline StatsPartial stats_block_fold(StatsPartial p) {
  __shared__ StatsPartial sh[kThreads / 64];
  for (int k = 0; k < 3; ++k) { p.mn[k] = wave_min(p.mn[k]); p.mx[k] = wave_max(p.mx[k]); }
  p.smin = wave_min(p.smin); p.smax = wave_max(p.smax); p.fabsmax = wave_max(p.fabsmax);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = p;
  __syncthreads();
  if (threadIdx.x == 0) {
    p = sh[0];
    for (int j = 1; j < kThreads / 64; ++j) stats_merge(p, sh[j]);
  }
  return p;
}
