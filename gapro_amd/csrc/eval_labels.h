// Label access shared by the evaluation kernels (eval_batch.hip, eval_ap.hip): labels stay in their file dtypes,
// one template instance per GAPRO_LABEL_* code.
#pragma once
#include "common.h"
#include "label_types.h"

#include <cstdint>

namespace {

template <class T>
__device__ inline long long label_at(const T* a, long long i) {
  return (long long)a[i];  // float64 labels: truncation, as the reference's .int()
}

// reference main() :196-197 (and gen_ps --eval_pslabel): sem[sem != -100] -= 2; sem[sem in (-1, -2)] = 18
__device__ inline long long remap_gt(long long s, int remap) {
  if (!remap || s == -100) return s;
  s -= 2;
  return (s == -1 || s == -2) ? 18 : s;
}

// the probability thresholds of a launch (ascending) and the bin of a point: b = #{j : prob >= thresholds[j]}, so
// row t of a result (the points with prob >= thresholds[t - 1]) is the bins t..K
struct Thresholds {
  float t[GAPRO_EVAL_MAX_THRESHOLDS];
};
__device__ inline int prob_bin(const Thresholds& thr, int K, float pr) {
  int b = 0;
  for (int j = 0; j < K; ++j) b += pr >= thr.t[j] ? 1 : 0;
  return b;
}

// dtype code -> template instance: the ground truth goes through with_label_type (label_types.h); the pseudo labels
// are integers
template <class F>
bool with_ps_type(int code, F&& f) {
  switch (code) {
    case GAPRO_LABEL_I32: f((const int32_t*)nullptr); return true;
    case GAPRO_LABEL_I64: f((const int64_t*)nullptr); return true;
    default: return false;
  }
}

}  // namespace
