// What the row walks of the two criteria share (match_loss.hip: ISBNet's; spf_loss.hip: SPFormer's): the workgroup sum
// in wave order, the float32 box test of the level-set term and the overflow-free sigmoid.  A workgroup is four waves.
#pragma once
#include <hip/hip_runtime.h>

#include "wave_reduce.h"

constexpr int kLossThreads = 256, kLossWaves = 4;

// every thread's partial -> the workgroup's sum in every thread: the butterfly, then the waves in their order
__device__ inline double block_sum(double v, double* slot /* [kLossWaves] in LDS, this quantity's own */) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = slot[0];
#pragma unroll
  for (int k = 1; k < kLossWaves; ++k) s += slot[k];
  return s;
}
__device__ inline int block_sum(int v, int* slot) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
  __syncthreads();
  return slot[0] + slot[1] + slot[2] + slot[3];
}

struct BoxTest {  // criterion.py:196-198 (SPFormer's loss.py:354-356) in float32: the padded faces of one label box
  float lo[3], hi[3];
};
__device__ inline BoxTest box_test(const float* __restrict__ g) {
  BoxTest bt;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    bt.lo[k] = g[k] - 0.005f;
    bt.hi[k] = g[k + 3] + 0.005f;
  }
  return bt;
}
__device__ inline bool inside(const BoxTest& bt, const float* __restrict__ c) {  // a NaN coordinate is outside
  bool in = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) in = in && c[k] >= bt.lo[k] && c[k] <= bt.hi[k];
  return in;
}

struct Sig {
  double sig, e;
};
__device__ inline Sig sigmoid_of(double x) {
  const double e = exp(-fabs(x));  // in (0, 1]: no overflow on either side
  return {(x >= 0.0 ? 1.0 : e) / (1.0 + e), e};
}
