// The criterion's four point-wise losses over every voxel of a batch (include/gapro_hip.h, "Point-wise losses"):
// ISBNet's Criterion.cal_point_wise_loss (isbnet/model/criterion.py:136-191) in two launches forward and one backward,
// with no host read.
//   partial   workgroups of four waves, each over its own run of kRun points in rounds of 256: a wave takes 64 points a
//             round.  The wave's block of the scores (64 rows of C floats, contiguous when the rows are packed) is
//             loaded with adjacent lanes on adjacent addresses into LDS rows of an ODD pitch (C | 1), so that lane t
//             walking row t meets 64 different banks; the 6- and 3-wide arrays go the same way (pitches 7, 7 and 3).
//             Lane t then forms point t's terms: float64 partials of the five sums (weighted nll, weight, L1, 1 - GIoU,
//             squared confidence error), the integer count n and the lowest refused point.  wave_reduce.h's butterfly,
//             then the waves through LDS in wave order: one record per workgroup.
//   finish    one workgroup: thread t folds the records t, t + 256, .., a butterfly and the waves in their order;
//             thread 0 writes f32[4], the normalisers (weight sum, n) and the status.
//   backward  the grid and the tiles of `partial`, element-wise: lse again per point, the gradient rows formed in the
//             LDS tile and stored with adjacent lanes on adjacent addresses; every element of every array is written
//             (zeros for an ignored label, outside P, and after a refusal).
// Arithmetic: every term in float64 from the float32 inputs, every sum in float64 in the order this layout
// fixes, one rounding to float32.  No atomics at all, no workgroup waits for another, no scratch; a lane past N forms no
// address.  min / max / clamp hand a NaN on, as torch's.
#include "common.h"
#include "launch_util.h"
#include "match_math.h"
#include "wave_reduce.h"

#include <cmath>
#include <cstdint>

namespace {

constexpr int kThreads = 256, kWaves = 4, kRound = kThreads;
constexpr int kRun = GAPRO_POINT_LOSS_RUN, kFold = GAPRO_POINT_LOSS_FOLD;
constexpr int kMinC = GAPRO_POINT_LOSS_MIN_CLASSES, kMaxC = GAPRO_POINT_LOSS_MAX_CLASSES;
constexpr long long kMaxN = 0x7fffffffLL, kNoPoint = 0x7fffffffffffffffLL;
constexpr int kBoxPitch = 7, kXyzPitch = 3, kSideFloats = 2 * kBoxPitch + kXyzPitch;  // per point: c, l, x
static_assert(kRun % kRound == 0 && kFold == kThreads, "the run is whole rounds; finish folds one record a thread");
enum { kFlagLabel = 1 };

struct PointRec {  // one per workgroup of `partial`
  double nll, wsum, l1, giou, conf;
  long long n, bad;  // bad: the lowest refused point or kNoPoint
  long long pad;
};
static_assert(sizeof(PointRec) == 64, "a record");

struct PointHead {  // the first 64 bytes of the workspace: written by `finish`, read by `backward`
  double wsum;
  long long n;
  int flags;
  int pad[11];
};
static_assert(sizeof(PointHead) == 64, "PointHead is the first 64 bytes of the workspace");

struct PointArgs {
  const float* z;
  long long ld;
  const void *sem, *inst;
  int sem_type, inst_type;
  const float *corners, *conf, *labels, *xyz, *weight;
  long long ignore, N;
  int C, pitch;
  double l1_scale;  // voxel_scale / 50
};

inline long long n_records(long long N) { return (N + kRun - 1) / kRun; }
inline int score_pitch(int C) { return C | 1; }
inline size_t lds_bytes(int C) { return (size_t)kWaves * 64 * (score_pitch(C) + kSideFloats) * sizeof(float); }

// rows [0, rows) of a [*, width] array with row stride ld  <->  tile[row * pitch + col]: lane t takes the elements
// t, t + 64, .. of the block in row-major order, so adjacent lanes are on adjacent addresses; no division in the loop
template <bool kStore, typename Src, typename Dst>
__device__ inline void move_rows(Dst* __restrict__ dst, const Src* __restrict__ src, long long ld, int width, int pitch,
                                 int rows, int lane) {
  int row = lane / width, col = lane % width;
  const int dr = 64 / width, dc = 64 % width;
  while (row < rows) {
    if (kStore)
      dst[(size_t)row * (size_t)ld + col] = src[row * pitch + col];
    else
      dst[row * pitch + col] = src[(size_t)row * (size_t)ld + col];
    row += dr;
    col += dc;
    if (col >= width) {
      col -= width;
      ++row;
    }
  }
}
__device__ inline void load_rows(float* tile, const float* src, long long ld, int width, int pitch, int rows, int lane) {
  move_rows<false>(tile, src, ld, width, pitch, rows, lane);
}
__device__ inline void store_rows(float* dst, const float* tile, long long ld, int width, int pitch, int rows, int lane) {
  move_rows<true>(dst, tile, ld, width, pitch, rows, lane);
}

// the max-shifted log-sum-exp of one LDS row; a NaN logit makes it NaN
__device__ inline double lse_of(const float* row, int C) {
  float m = row[0];
  for (int c = 1; c < C; ++c) m = fmaxf(m, row[c]);
  double sum = 0.0;
  for (int c = 0; c < C; ++c) sum += exp((double)row[c] - (double)m);
  return (double)m + log(sum);
}

// the point's two boxes in float64: a = c + [x, x], b = l + [x, x]
__device__ inline void boxes_of(const float* c, const float* l, const float* x, double* a, double* b) {
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    a[k] = (double)c[k] + (double)x[k % 3];
    b[k] = (double)l[k] + (double)x[k % 3];
  }
}

// ---- partial -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_point_partial(PointArgs a, PointRec* __restrict__ recs) {
  extern __shared__ float lds[];
  __shared__ PointRec s_rec[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* tile = lds + (size_t)wave * 64 * a.pitch;
  float* side = lds + (size_t)kWaves * 64 * a.pitch + (size_t)wave * 64 * kSideFloats;
  float *t_c = side, *t_l = side + 64 * kBoxPitch, *t_x = side + 128 * kBoxPitch;
  const long long base = (long long)blockIdx.x * kRun;

  double nll = 0.0, wsum = 0.0, l1 = 0.0, giou = 0.0, conf = 0.0;
  long long n = 0, bad = kNoPoint;
  for (int r = 0; r < kRun / kRound && base + (long long)r * kRound < a.N; ++r) {  // uniform over the workgroup
    const long long p0 = base + (long long)r * kRound + wave * 64;
    const long long left = a.N - p0;
    const int rows = left >= 64 ? 64 : (left > 0 ? (int)left : 0);
    if (rows > 0) {
      load_rows(tile, a.z + (size_t)p0 * (size_t)a.ld, a.ld, a.C, a.pitch, rows, lane);
      load_rows(t_c, a.corners + (size_t)p0 * 6, 6, 6, kBoxPitch, rows, lane);
      load_rows(t_l, a.labels + (size_t)p0 * 6, 6, 6, kBoxPitch, rows, lane);
      load_rows(t_x, a.xyz + (size_t)p0 * 3, 3, 3, kXyzPitch, rows, lane);
    }
    __syncthreads();
    if (lane < rows) {
      const long long p = p0 + lane;
      const long long y = cls_at(a.sem, a.sem_type, (int)p);
      if (y != a.ignore) {
        if (y < 0 || y >= a.C) {
          bad = p < bad ? p : bad;
        } else {
          const float* row = tile + lane * a.pitch;
          const double wt = a.weight ? (double)a.weight[y] : 1.0;
          nll += wt * (lse_of(row, a.C) - (double)row[y]);
          wsum += wt;
        }
      }
      if (cls_at(a.inst, a.inst_type, (int)p) != a.ignore) {
        const float *c = t_c + lane * kBoxPitch, *l = t_l + lane * kBoxPitch;
        double pa[6], pb[6], iou;
        boxes_of(c, l, t_x + lane * kXyzPitch, pa, pb);
#pragma unroll
        for (int k = 0; k < 6; ++k) l1 += fabs((double)c[k] - (double)l[k]);
        giou += giou_loss_of(pa, pb, nullptr, &iou);
        const double e = (double)a.conf[p] - iou;
        conf += e * e;
        ++n;
      }
    }
    __syncthreads();
  }

  nll = wave_sum(nll);
  wsum = wave_sum(wsum);
  l1 = wave_sum(l1);
  giou = wave_sum(giou);
  conf = wave_sum(conf);
  n = wave_sum(n);
  bad = wave_min(bad);
  if (lane == 0) s_rec[wave] = PointRec{nll, wsum, l1, giou, conf, n, bad, 0};
  __syncthreads();
  if (threadIdx.x != 0) return;
  PointRec t = s_rec[0];
#pragma unroll
  for (int k = 1; k < kWaves; ++k) {  // wave order
    const PointRec& q = s_rec[k];
    t.nll += q.nll;
    t.wsum += q.wsum;
    t.l1 += q.l1;
    t.giou += q.giou;
    t.conf += q.conf;
    t.n += q.n;
    t.bad = q.bad < t.bad ? q.bad : t.bad;
  }
  recs[blockIdx.x] = t;
}

// ---- finish --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_point_finish(PointHead* __restrict__ head, const PointRec* __restrict__ recs,
                                                           long long n_recs, double l1_scale, float* __restrict__ losses,
                                                           int* __restrict__ status) {
  __shared__ PointRec s_rec[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  PointRec t{0.0, 0.0, 0.0, 0.0, 0.0, 0, kNoPoint, 0};
  for (long long k = threadIdx.x; k < n_recs; k += kFold) {  // record order
    const PointRec q = recs[k];
    t.nll += q.nll;
    t.wsum += q.wsum;
    t.l1 += q.l1;
    t.giou += q.giou;
    t.conf += q.conf;
    t.n += q.n;
    t.bad = q.bad < t.bad ? q.bad : t.bad;
  }
  t.nll = wave_sum(t.nll);
  t.wsum = wave_sum(t.wsum);
  t.l1 = wave_sum(t.l1);
  t.giou = wave_sum(t.giou);
  t.conf = wave_sum(t.conf);
  t.n = wave_sum(t.n);
  t.bad = wave_min(t.bad);
  if (lane == 0) s_rec[wave] = t;
  __syncthreads();
  if (threadIdx.x != 0) return;
  t = s_rec[0];
#pragma unroll
  for (int k = 1; k < kWaves; ++k) {
    const PointRec& q = s_rec[k];
    t.nll += q.nll;
    t.wsum += q.wsum;
    t.l1 += q.l1;
    t.giou += q.giou;
    t.conf += q.conf;
    t.n += q.n;
    t.bad = q.bad < t.bad ? q.bad : t.bad;
  }
  const int flags = t.bad != kNoPoint ? kFlagLabel : 0;
  head->wsum = t.wsum;
  head->n = t.n;
  head->flags = flags;
  status[0] = flags ? GAPRO_ERR_BAD_ARG : GAPRO_OK;
  status[1] = flags ? (int)(t.bad > 0x7fffffffLL ? 0x7fffffffLL : t.bad) : -1;
  status[2] = flags;
  status[3] = 0;
  if (flags) {
#pragma unroll
    for (int k = 0; k < GAPRO_POINT_LOSS_N; ++k) losses[k] = NAN;
    return;
  }
  const double n = (double)t.n;
  losses[0] = (float)(t.nll / t.wsum);  // every label ignored: 0 / 0, NaN as F.cross_entropy
  losses[1] = t.n ? (float)(l1_scale * t.l1 / n) : 0.0f;
  losses[2] = t.n ? (float)(t.giou / n) : 0.0f;
  losses[3] = t.n ? (float)(t.conf / n) : 0.0f;
}

// ---- backward ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_point_backward(PointArgs a, const PointHead* __restrict__ head,
                                                             const float* __restrict__ upstream,
                                                             float* __restrict__ g_z, float* __restrict__ g_c,
                                                             float* __restrict__ g_conf) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* tile = lds + (size_t)wave * 64 * a.pitch;
  float* side = lds + (size_t)kWaves * 64 * a.pitch + (size_t)wave * 64 * kSideFloats;
  float *t_c = side, *t_l = side + 64 * kBoxPitch, *t_x = side + 128 * kBoxPitch;
  const long long base = (long long)blockIdx.x * kRun;
  const bool live = head->flags == 0;  // a refused call: zeros
  const bool boxes = live && head->n > 0 && (g_c || g_conf);
  const double n = (double)head->n;
  const double k_sem = (double)upstream[0] / head->wsum;
  const double k_l1 = (double)upstream[1] * a.l1_scale / n, k_gi = (double)upstream[2] / n;
  const double k_cf = (double)upstream[3] * 2.0 / n;

  for (int r = 0; r < kRun / kRound && base + (long long)r * kRound < a.N; ++r) {  // uniform over the workgroup
    const long long p0 = base + (long long)r * kRound + wave * 64;
    const long long left = a.N - p0;
    const int rows = left >= 64 ? 64 : (left > 0 ? (int)left : 0);
    if (rows > 0) {
      if (g_z && live) load_rows(tile, a.z + (size_t)p0 * (size_t)a.ld, a.ld, a.C, a.pitch, rows, lane);
      if (boxes) {
        load_rows(t_c, a.corners + (size_t)p0 * 6, 6, 6, kBoxPitch, rows, lane);
        load_rows(t_l, a.labels + (size_t)p0 * 6, 6, 6, kBoxPitch, rows, lane);
        load_rows(t_x, a.xyz + (size_t)p0 * 3, 3, 3, kXyzPitch, rows, lane);
      }
    }
    __syncthreads();
    if (lane < rows) {
      const long long p = p0 + lane;
      if (g_z) {
        float* row = tile + lane * a.pitch;
        const long long y = live ? cls_at(a.sem, a.sem_type, (int)p) : a.ignore;  // inside [0, C) or ignored: no flag
        if (y == a.ignore) {
          for (int c = 0; c < a.C; ++c) row[c] = 0.0f;
        } else {
          const double lse = lse_of(row, a.C);
          const double k = k_sem * (a.weight ? (double)a.weight[y] : 1.0);
          for (int c = 0; c < a.C; ++c) {
            const double dz = (double)row[c] - lse;
            row[c] = (float)(k * (c == y ? expm1(dz) : exp(dz)));  // softmax - onehot, no cancellation at p -> 1
          }
        }
      }
      const bool pos = boxes && cls_at(a.inst, a.inst_type, (int)p) != a.ignore;
      float* c = t_c + lane * kBoxPitch;
      if (pos) {
        const float* l = t_l + lane * kBoxPitch;
        double pa[6], pb[6], gg[6], iou;
        boxes_of(c, l, t_x + lane * kXyzPitch, pa, pb);
        giou_loss_of(pa, pb, gg, &iou);
        if (g_conf) g_conf[p] = (float)(k_cf * ((double)a.conf[p] - iou));
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          const double diff = (double)c[k] - (double)l[k];
          const double sgn = diff > 0.0 ? 1.0 : (diff < 0.0 ? -1.0 : diff);  // sign(0) = 0; a NaN stays
          c[k] = (float)(k_l1 * sgn + k_gi * gg[k]);
        }
      } else {
        if (g_conf) g_conf[p] = 0.0f;
#pragma unroll
        for (int k = 0; k < 6; ++k) c[k] = 0.0f;
      }
    }
    __syncthreads();
    if (rows > 0) {
      if (g_z) store_rows(g_z + (size_t)p0 * (size_t)a.C, tile, a.C, a.C, a.pitch, rows, lane);
      if (g_c) store_rows(g_c + (size_t)p0 * 6, t_c, 6, 6, kBoxPitch, rows, lane);
    }
    __syncthreads();
  }
}

int check_args(gapro_ctx* ctx, const char* who, int64_t N, int32_t C, const float* z, int64_t ld, const void* sem,
               int32_t sem_type, const void* inst, int32_t inst_type, const float* corners, const float* conf,
               const float* labels, const float* xyz, double voxel_scale, const void* ws, size_t ws_bytes) {
  if (!z || !sem || !inst || !corners || !conf || !labels || !xyz || !ws)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: bad argument", who);
  if (N < 1 || N > kMaxN) return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: n_points outside [1, 2^31 - 1]", who);
  if (C < kMinC || C > kMaxC) return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: n_classes outside [%d, %d]", who, kMinC, kMaxC);
  if (ld < C) return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: ld_scores < n_classes", who);
  for (int32_t t : {sem_type, inst_type})
    if (t != GAPRO_LABEL_I32 && t != GAPRO_LABEL_I64) return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: unknown label type", who);
  if (!std::isfinite(voxel_scale)) return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: voxel_scale is not finite", who);
  if (ws_bytes < gapro_point_loss_workspace_bytes(N, C))
    return gapro_fail(ctx, GAPRO_ERR_WORKSPACE, "%s: workspace too small", who);
  return GAPRO_OK;
}

template <typename K>
int allow_lds(gapro_ctx* ctx, K kern, size_t lds) {
  if (lds > 48 * 1024)
    GAPRO_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return GAPRO_OK;
}

}  // namespace

extern "C" {

size_t gapro_point_loss_workspace_bytes(int64_t n_points, int32_t n_classes) {
  if (n_points < 1 || n_points > kMaxN || n_classes < kMinC || n_classes > kMaxC) return 0;
  return align_up(sizeof(PointHead) + (size_t)n_records(n_points) * sizeof(PointRec), 256);
}

int gapro_point_loss_forward(gapro_ctx* ctx, void* stream_, int64_t n_points, int32_t n_classes,
                             const float* d_semantic_scores, int64_t ld_scores, const void* d_semantic_labels,
                             int32_t semantic_type, const void* d_instance_labels, int32_t instance_type,
                             const float* d_corners_offset, const float* d_box_conf,
                             const float* d_corners_offset_labels, const float* d_coords_float,
                             const float* d_semantic_weight, int64_t ignore_label, double voxel_scale,
                             void* d_workspace, size_t workspace_bytes, float* d_losses, int32_t* d_status,
                             int32_t* h_status_pinned) {
  const char* who = "gapro_point_loss_forward";
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  if (!d_losses || !d_status) return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: bad argument", who);
  if (int rc = check_args(ctx, who, n_points, n_classes, d_semantic_scores, ld_scores, d_semantic_labels, semantic_type,
                          d_instance_labels, instance_type, d_corners_offset, d_box_conf, d_corners_offset_labels,
                          d_coords_float, voxel_scale, d_workspace, workspace_bytes))
    return rc;
  const PointArgs a{d_semantic_scores, (long long)ld_scores, d_semantic_labels, d_instance_labels, semantic_type,
                    instance_type, d_corners_offset, d_box_conf, d_corners_offset_labels, d_coords_float,
                    d_semantic_weight, (long long)ignore_label, (long long)n_points, n_classes,
                    score_pitch(n_classes), voxel_scale / 50.0};
  PointHead* head = (PointHead*)d_workspace;
  PointRec* recs = (PointRec*)(head + 1);
  const long long g = n_records(n_points);
  const size_t lds = lds_bytes(n_classes);
  hipStream_t stream = (hipStream_t)stream_;
  if (int rc = allow_lds(ctx, k_point_partial, lds)) return rc;
  hipLaunchKernelGGL(k_point_partial, dim3((unsigned)g), dim3(kThreads), lds, stream, a, recs);
  hipLaunchKernelGGL(k_point_finish, dim3(1), dim3(kThreads), 0, stream, head, recs, g, a.l1_scale, d_losses,
                     (int*)d_status);
  GAPRO_LAUNCH_CHECK(ctx);
  if (h_status_pinned)
    GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(h_status_pinned, d_status, GAPRO_MATCH_STATUS_WORDS * sizeof(int32_t),
                                        hipMemcpyDeviceToHost, stream));
  return GAPRO_OK;
}

int gapro_point_loss_backward(gapro_ctx* ctx, void* stream_, int64_t n_points, int32_t n_classes,
                              const float* d_semantic_scores, int64_t ld_scores, const void* d_semantic_labels,
                              int32_t semantic_type, const void* d_instance_labels, int32_t instance_type,
                              const float* d_corners_offset, const float* d_box_conf,
                              const float* d_corners_offset_labels, const float* d_coords_float,
                              const float* d_semantic_weight, int64_t ignore_label, double voxel_scale,
                              const void* d_workspace, size_t workspace_bytes, const float* d_grad_losses,
                              float* d_grad_semantic_scores, float* d_grad_corners_offset, float* d_grad_box_conf) {
  const char* who = "gapro_point_loss_backward";
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  if (!d_grad_losses) return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: bad argument", who);
  if (int rc = check_args(ctx, who, n_points, n_classes, d_semantic_scores, ld_scores, d_semantic_labels, semantic_type,
                          d_instance_labels, instance_type, d_corners_offset, d_box_conf, d_corners_offset_labels,
                          d_coords_float, voxel_scale, d_workspace, workspace_bytes))
    return rc;
  if (!d_grad_semantic_scores && !d_grad_corners_offset && !d_grad_box_conf) return GAPRO_OK;
  const PointArgs a{d_semantic_scores, (long long)ld_scores, d_semantic_labels, d_instance_labels, semantic_type,
                    instance_type, d_corners_offset, d_box_conf, d_corners_offset_labels, d_coords_float,
                    d_semantic_weight, (long long)ignore_label, (long long)n_points, n_classes,
                    score_pitch(n_classes), voxel_scale / 50.0};
  const size_t lds = lds_bytes(n_classes);
  if (int rc = allow_lds(ctx, k_point_backward, lds)) return rc;
  hipLaunchKernelGGL(k_point_backward, dim3((unsigned)n_records(n_points)), dim3(kThreads), lds, (hipStream_t)stream_, a,
                     (const PointHead*)d_workspace, d_grad_losses, d_grad_semantic_scores, d_grad_corners_offset,
                     d_grad_box_conf);
  GAPRO_LAUNCH_CHECK(ctx);
  return GAPRO_OK;
}

}  // extern "C"
