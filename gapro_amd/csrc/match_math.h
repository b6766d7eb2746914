// What the matcher's cost kernel (match_cost.hip), the two criteria (match_loss.hip, spf_loss.hip) and the point-wise
// losses (point_loss.hip) share: the class label read, the refusal head of a workspace with the status words it ends
// as, the overflow-free sigmoid and softplus of a logit, torch's NaN-propagating min / max / clamp, which the
// reference's box terms go through, and the GIoU loss of one pair of boxes with its derivative.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/gapro_hip.h"

__device__ inline long long cls_at(const void* cls, int type, int i) {
  return type == GAPRO_LABEL_I32 ? (long long)((const int*)cls)[i] : ((const long long*)cls)[i];
}

struct RefusalHead {  // the first 64 bytes of a workspace; uploaded with the tables, so zero before the first kernel
  int flags;          // what the kernels refused, one bit per reason: atomicOr
  int bad;            // the first sample or task with a reason: atomicMin from kNoBad
  int reserved[14];
};
static_assert(sizeof(RefusalHead) == 64, "RefusalHead is the first 64 bytes of the workspace");
constexpr int kNoBad = 0x7fffffff;

// the GAPRO_MATCH_STATUS_WORDS of a call, by one thread, once every kernel that refuses has run
__device__ inline void write_status(int* __restrict__ status, const RefusalHead& s) {
  status[0] = s.flags ? GAPRO_ERR_BAD_ARG : GAPRO_OK;
  status[1] = s.flags ? s.bad : -1;
  status[2] = s.flags;
  status[3] = 0;
}

struct Sig {
  double sig, e;  // sigmoid(x) and exp(-|x|)
};
__device__ inline Sig sigmoid_of(double x) {
  const double e = exp(-fabs(x));  // in (0, 1]: no overflow on either side
  return {(x >= 0.0 ? 1.0 : e) / (1.0 + e), e};
}
__device__ inline double softplus_of(double x, const Sig& sg) { return (x > 0.0 ? x : 0.0) + log1p(sg.e); }

__device__ inline double nan_min(double a, double b) { return (a < b || a != a) ? a : b; }  // torch.min: a NaN wins
__device__ inline double nan_max(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ inline double clamp0(double v) { return v < 0.0 ? 0.0 : v; }                     // clamp(min=0) keeps a NaN

// model_utils.py:277-306 (and :416-444, the same per pair) for one pair in float64: 1 - GIoU, with `grad` its derivative
// by the predicted box, with `iou_out` the IoU; T is float (the stored boxes) or double (boxes formed in float64)
template <typename T>
__device__ inline double giou_loss_of(const T* __restrict__ p, const T* __restrict__ g, double* grad,
                                       double* iou_out = nullptr) {
  double iw[3], pw[3], bw[3];
  double inter = 1.0, pv = 1.0, gv = 1.0, bound = 1.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double a0 = p[k], a1 = p[k + 3], b0 = g[k], b1 = g[k + 3];
    iw[k] = clamp0(nan_min(a1, b1) - nan_max(a0, b0));
    pw[k] = clamp0(a1 - a0);
    bw[k] = clamp0(nan_max(a1, b1) - nan_min(a0, b0));
    inter *= iw[k];
    pv *= pw[k];
    gv *= clamp0(b1 - b0);
    bound *= bw[k];
  }
  const double uni = gv + pv - inter;
  const double iou = inter / (uni + 1e-6);
  if (iou_out) *iou_out = iou;
  const double giou = iou - (bound - uni) / (bound + 1e-6);
  if (grad) {
    // d giou by inter, by the predicted volume and by the bounding volume (uni = gv + pv - inter)
    const double d_uni = -inter / ((uni + 1e-6) * (uni + 1e-6)) + 1.0 / (bound + 1e-6);
    const double g_inter = 1.0 / (uni + 1e-6) - d_uni, g_pv = d_uni;
    const double g_bound = -(uni + 1e-6) / ((bound + 1e-6) * (bound + 1e-6));
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
      const double a0 = p[k], a1 = p[k + 3], b0 = g[k], b1 = g[k + 3];
      // torch: clamp(min=0) passes the gradient where its argument is >= 0; min / max share it at a tie
      const double ci = (nan_min(a1, b1) - nan_max(a0, b0)) >= 0.0 ? g_inter * iw[k1] * iw[k2] : 0.0;
      const double cp = (a1 - a0) >= 0.0 ? g_pv * pw[k1] * pw[k2] : 0.0;
      const double cb = (nan_max(a1, b1) - nan_min(a0, b0)) >= 0.0 ? g_bound * bw[k1] * bw[k2] : 0.0;
      const double up_a = a1 < b1 ? 1.0 : (a1 == b1 ? 0.5 : 0.0), lo_a = a0 > b0 ? 1.0 : (a0 == b0 ? 0.5 : 0.0);
      const double ub_a = a1 > b1 ? 1.0 : (a1 == b1 ? 0.5 : 0.0), lb_a = a0 < b0 ? 1.0 : (a0 == b0 ? 0.5 : 0.0);
      grad[k + 3] = -(ci * up_a + cp + cb * ub_a);
      grad[k] = ci * lo_a + cp + cb * lb_a;
    }
  }
  return 1.0 - giou;
}
