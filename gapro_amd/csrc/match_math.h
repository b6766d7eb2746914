// What the matcher's cost kernel (match_cost.hip) and the matched losses (match_loss.hip) share: the class label read
// and torch's NaN-propagating min / max / clamp, which the reference's box terms go through.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/gapro_hip.h"

__device__ inline long long cls_at(const void* cls, int type, int i) {
  return type == GAPRO_LABEL_I32 ? (long long)((const int*)cls)[i] : ((const long long*)cls)[i];
}

__device__ inline double nan_min(double a, double b) { return (a < b || a != a) ? a : b; }  // torch.min: a NaN wins
__device__ inline double nan_max(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ inline double clamp0(double v) { return v < 0.0 ? 0.0 : v; }                     // clamp(min=0) keeps a NaN
