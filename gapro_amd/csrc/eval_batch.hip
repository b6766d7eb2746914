// Pseudo-label quality evaluation: the reference's get_miou_scene / cal_iou (eval_ps_labels.py:35-42,100-147) and
// get_scene_sem_conf (:150-172) over a batch of scenes laid out back to back, with K probability thresholds in the
// same pass (main()'s certain_cond filter, :214-220).  A single scene is a batch of one without thresholds.
//
// A point of a scene falls in bin b = #{j : prob >= thresholds[j]} (thresholds ascending; bin 0 without thresholds).
// One histogram pass over the points tallies per (scene, bin) the (gt + 1, ps + 1) pair counts (the intersections
// of the reference's one-hot matrix product, :36), the first point of every id, the confusion bins and the point
// count.  Row t of the result keeps the points with bin >= t, so a suffix sum (counts) / suffix min (first points)
// over the bins turns the bin tables into the row tables, and the finalize step computes the IoUs from them.
// Integer atomics only, floats only in the finalize: every row is bit-identical to the reference on the filtered
// scene, whatever the batch composition.  Without instance arrays only the confusion and the counts are tallied.
#include "common.h"
#include "eval_labels.h"
#include "launch_util.h"

#include <algorithm>
#include <type_traits>

namespace {

constexpr int kThreads = 256;
constexpr int kLdsIds = 512;    // (bin, id) first-point entries kept in LDS per table
constexpr int kPairLds = 8192;  // (bin, gt, ps) pair-count bins kept in LDS
constexpr int kConfLds = 2048;  // (bin, gt class, ps class) confusion bins kept in LDS (C = 19: five bins)
constexpr int kMaxBins = GAPRO_EVAL_MAX_THRESHOLDS + 1;
constexpr unsigned long long kKeyMax = ~0ull;


// one scene's tables in the workspace: B bins (rows after the suffix pass) of each
struct SceneTables {
  unsigned long long* first_gt;  // [B][cap_gt] first point (scene-local index) of a gt id
  unsigned long long* first_ps;  // [B][cap_ps]
  int* pair;                     // [B][(cap_gt + 1) * (cap_ps + 1)] counts of (gt + 1, ps + 1) pairs, 0 = no id
  int* ps_n;                     // [B][cap_ps] points of a pseudo id (after the suffix pass)
  int cap_gt, cap_ps, W;
  long long nbin;
};

__host__ __device__ inline size_t scene_bytes(int cap_gt, int cap_ps, int B) {
  const size_t nbin = (size_t)(cap_gt + 1) * (size_t)(cap_ps + 1);
  return align_up((size_t)B * ((size_t)cap_gt + cap_ps) * sizeof(unsigned long long) +
                      (size_t)B * (nbin + (size_t)cap_ps) * sizeof(int), 256);
}

__device__ inline SceneTables scene_tables(void* ws, const gapro_eval_scene& s, int B) {
  SceneTables t;
  t.cap_gt = s.max_gt;
  t.cap_ps = s.max_ps;
  t.W = s.max_ps + 1;
  t.nbin = (long long)(s.max_gt + 1) * t.W;
  unsigned long long* p = (unsigned long long*)((char*)ws + s.ws_offset);
  t.first_gt = p;
  t.first_ps = p + (size_t)B * t.cap_gt;
  t.pair = (int*)(t.first_ps + (size_t)B * t.cap_ps);
  t.ps_n = t.pair + (size_t)B * t.nbin;
  return t;
}

__global__ __launch_bounds__(kThreads) void k_evb_init(const gapro_eval_scene* __restrict__ scenes, void* ws, int B) {
  const gapro_eval_scene s = scenes[blockIdx.y];
  SceneTables t = scene_tables(ws, s, B);
  const long long n_first = (long long)B * (t.cap_gt + t.cap_ps);
  const long long n_int = (long long)B * (t.nbin + t.cap_ps);
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n_first; i += stride) t.first_gt[i] = kKeyMax;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n_int; i += stride) t.pair[i] = 0;
}

// the point pass: one histogram pass per scene (blockIdx.y), LDS-privatised when the scene's tables are small;
// inst_gt == NULL (then inst_ps too): a confusion-only launch, no pair or first-point tallies
template <class TGS, class TGI, class TPS, class TPI>
__global__ __launch_bounds__(kThreads) void k_evb_points(const gapro_eval_scene* __restrict__ scenes,
                                                         const TGS* __restrict__ sem_gt, const TGI* __restrict__ inst_gt,
                                                         const TPS* __restrict__ sem_ps, const TPI* __restrict__ inst_ps,
                                                         const float* __restrict__ prob, Thresholds thr, int K,
                                                         int remap, int C, void* ws, long long* __restrict__ conf,
                                                         long long* __restrict__ kept, int* __restrict__ status) {
  const int scene = blockIdx.y;
  const gapro_eval_scene s = scenes[scene];
  const long long n = s.n_points, off = s.point_offset;
  if ((long long)blockIdx.x * kThreads >= n) return;  // the whole workgroup: nothing of this scene left for it
  const int B = K + 1;
  SceneTables t = scene_tables(ws, s, B);
  __shared__ int s_pair[kPairLds];
  __shared__ unsigned long long s_fg[kLdsIds], s_fp[kLdsIds];
  __shared__ int s_conf[kConfLds];
  __shared__ int s_kept[kMaxBins];
  const bool lds_pair = (long long)B * t.nbin <= kPairLds;
  const int CC = C * C;
  const bool lds_conf = B * CC <= kConfLds;
  const bool pairs = inst_gt != nullptr;
  for (int j = threadIdx.x; j < kLdsIds; j += kThreads) {
    s_fg[j] = kKeyMax;
    s_fp[j] = kKeyMax;
  }
  if (lds_pair)
    for (int j = threadIdx.x; j < (int)(B * t.nbin); j += kThreads) s_pair[j] = 0;
  if (lds_conf)
    for (int j = threadIdx.x; j < B * CC; j += kThreads) s_conf[j] = 0;
  if (threadIdx.x < kMaxBins) s_kept[threadIdx.x] = 0;
  __syncthreads();
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
    const long long gi_ = off + i;
    const int b = K ? prob_bin(thr, K, prob[gi_]) : 0;
    atomicAdd(&s_kept[b], 1);
    // get_scene_sem_conf (eval_ps_labels.py:150-172): unlabeled pseudo points count as a wrong class (:157-161)
    const long long sg = remap_gt(label_at(sem_gt, gi_), remap);
    if (sg != -100) {
      long long sp = label_at(sem_ps, gi_);
      if (sp == -100) sp = sg < 18 ? sg + 1 : sg - 1;
      const long long x = sp + (long long)C * sg;
      if (x >= 0 && x < CC) {
        if (lds_conf) atomicAdd(&s_conf[b * CC + (int)x], 1);
        else atomicAdd((unsigned long long*)&conf[(long long)b * CC + x], 1ull);
      }
    }
    if (!pairs) continue;
    // get_miou_scene's pair counts and first points (eval_ps_labels.py:101-124); an id < 0 counts as none (:118,124)
    const long long g = label_at(inst_gt, gi_), p = label_at(inst_ps, gi_);
    if (g >= t.cap_gt || p >= t.cap_ps) {
      atomicExch(&status[scene], GAPRO_ERR_BAD_ARG);
      continue;
    }
    const int gi = g < 0 ? 0 : (int)g + 1, pi = p < 0 ? 0 : (int)p + 1;
    const long long cell = (long long)b * t.nbin + (long long)gi * t.W + pi;
    if (lds_pair) atomicAdd(&s_pair[cell], 1);
    else atomicAdd(&t.pair[cell], 1);
    if (g >= 0) {
      const long long f = (long long)b * t.cap_gt + g;
      if (f < kLdsIds) atomicMin(&s_fg[f], (unsigned long long)i);
      else atomicMin(&t.first_gt[f], (unsigned long long)i);
    }
    if (p >= 0) {
      const long long f = (long long)b * t.cap_ps + p;
      if (f < kLdsIds) atomicMin(&s_fp[f], (unsigned long long)i);
      else atomicMin(&t.first_ps[f], (unsigned long long)i);
    }
  }
  __syncthreads();
  if (lds_pair)
    for (int j = threadIdx.x; j < (int)(B * t.nbin); j += kThreads)
      if (s_pair[j]) atomicAdd(&t.pair[j], s_pair[j]);
  for (int j = threadIdx.x; j < kLdsIds; j += kThreads) {
    if (j < (long long)B * t.cap_gt && s_fg[j] != kKeyMax) atomicMin(&t.first_gt[j], s_fg[j]);
    if (j < (long long)B * t.cap_ps && s_fp[j] != kKeyMax) atomicMin(&t.first_ps[j], s_fp[j]);
  }
  if (lds_conf)
    for (int j = threadIdx.x; j < B * CC; j += kThreads)
      if (s_conf[j]) atomicAdd((unsigned long long*)&conf[j], (unsigned long long)s_conf[j]);
  if (threadIdx.x < B && s_kept[threadIdx.x])
    atomicAdd((unsigned long long*)&kept[(long long)scene * B + threadIdx.x], (unsigned long long)s_kept[threadIdx.x]);
}

// bins -> rows: row t = bins t..B-1 (suffix min of the first points, suffix sum of the pair counts)
__global__ __launch_bounds__(kThreads) void k_evb_suffix(const gapro_eval_scene* __restrict__ scenes, void* ws, int B) {
  const gapro_eval_scene s = scenes[blockIdx.y];
  SceneTables t = scene_tables(ws, s, B);
  const long long n_gt = t.cap_gt, n_ps = t.cap_ps, n_cells = n_gt + n_ps + t.nbin;
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long c = (long long)blockIdx.x * kThreads + threadIdx.x; c < n_cells; c += stride) {
    if (c < n_gt + n_ps) {
      unsigned long long* a = c < n_gt ? t.first_gt + c : t.first_ps + (c - n_gt);
      const long long w = c < n_gt ? n_gt : n_ps;
      for (int b = B - 2; b >= 0; --b) a[b * w] = a[(b + 1) * w] < a[b * w] ? a[(b + 1) * w] : a[b * w];
    } else {
      int* a = t.pair + (c - n_gt - n_ps);
      for (int b = B - 2; b >= 0; --b) a[b * t.nbin] += a[(b + 1) * t.nbin];
    }
  }
}

// the batch-wide confusion [B][C*C] and the point counts [scene][B], bins -> rows
__global__ __launch_bounds__(kThreads) void k_evb_suffix_counts(long long* __restrict__ conf, int CC,
                                                                long long* __restrict__ kept, int n_scenes, int B) {
  const long long n_cells = (long long)CC + n_scenes;
  for (long long c = (long long)blockIdx.x * kThreads + threadIdx.x; c < n_cells; c += (long long)gridDim.x * kThreads) {
    if (c < CC)
      for (int b = B - 2; b >= 0; --b) conf[(long long)b * CC + c] += conf[(long long)(b + 1) * CC + c];
    else
      for (int b = B - 2; b >= 0; --b) kept[(c - CC) * B + b] += kept[(c - CC) * B + b + 1];
  }
}

// |ps| per row and pseudo id: the column sums of the pair table (eval_ps_labels.py:38)
__global__ __launch_bounds__(kThreads) void k_evb_ps_count(const gapro_eval_scene* __restrict__ scenes, void* ws, int B) {
  const gapro_eval_scene s = scenes[blockIdx.y];
  SceneTables t = scene_tables(ws, s, B);
  const long long n_items = (long long)B * t.cap_ps;
  for (long long it = (long long)blockIdx.x * kThreads + threadIdx.x; it < n_items; it += (long long)gridDim.x * kThreads) {
    const long long r = it / t.cap_ps, p = it % t.cap_ps;
    const int* pr = t.pair + r * t.nbin;
    int ps_n = 0;
    for (int q = 0; q <= t.cap_gt; ++q) ps_n += pr[(long long)q * t.W + p + 1];
    t.ps_n[it] = ps_n;
  }
}

// per (scene, row, gt id): the largest inter / (|gt| + |ps| - inter + 1e-4) over the pseudo instances of the same
// class, float32 in the reference's operation order (:36-40,131-136); class = label of the first point or -1
template <class TGS, class TPS>
__global__ __launch_bounds__(kThreads) void k_evb_finalize(const gapro_eval_scene* __restrict__ scenes,
                                                           const TGS* __restrict__ sem_gt, const TPS* __restrict__ sem_ps,
                                                           int remap, void* ws, int B, float* __restrict__ max_iou,
                                                           float* __restrict__ gt_cls) {
  const gapro_eval_scene s = scenes[blockIdx.y];
  SceneTables t = scene_tables(ws, s, B);
  const long long n_items = (long long)B * t.cap_gt;
  for (long long it = (long long)blockIdx.x * kThreads + threadIdx.x; it < n_items; it += (long long)gridDim.x * kThreads) {
    const long long r = it / t.cap_gt, g = it % t.cap_gt;
    const unsigned long long fg = t.first_gt[it];
    const float cg = fg == kKeyMax ? -1.0f : (float)remap_gt(label_at(sem_gt, s.point_offset + (long long)fg), remap);
    float best = 0.0f;  // no pseudo instance at all: every IoU is 0
    if (cg >= 0.0f) {   // rows of class < 0 are dropped by the caller (:139)
      const int* row = t.pair + r * t.nbin + (g + 1) * t.W;
      long long gt_n = 0;
      for (int p = 0; p <= t.cap_ps; ++p) gt_n += row[p];
      for (int p = 0; p < t.cap_ps; ++p) {
        const unsigned long long fp = t.first_ps[r * t.cap_ps + p];
        const float cp = fp == kKeyMax ? -1.0f : (float)label_at(sem_ps, s.point_offset + (long long)fp);
        const long long ps_n = t.ps_n[r * t.cap_ps + p];
        const float inter = (float)row[p + 1];
        const float iou = inter / ((float)gt_n + (float)ps_n - inter + 1e-4f);
        const float v = iou * (cg == cp ? 1.0f : 0.0f);
        best = (p == 0 || v > best) ? v : best;
      }
    }
    max_iou[s.row_offset + it] = best;
    gt_cls[s.row_offset + it] = cg;
  }
}

}  // namespace

extern "C" {

size_t gapro_eval_batch_workspace_bytes(gapro_eval_scene* h_scenes, int32_t n_scenes, int32_t n_thresholds) {
  if (!h_scenes || n_scenes < 1 || n_thresholds < 0 || n_thresholds > GAPRO_EVAL_MAX_THRESHOLDS) return 0;
  const int B = n_thresholds + 1;
  size_t bytes = 0;
  long long rows = 0;
  for (int i = 0; i < n_scenes; ++i) {
    gapro_eval_scene& s = h_scenes[i];
    if (s.max_gt < 1 || s.max_ps < 1) return 0;
    s.ws_offset = (int64_t)bytes;
    s.row_offset = rows;
    bytes += scene_bytes(s.max_gt, s.max_ps, B);
    rows += (long long)B * s.max_gt;
  }
  return bytes;
}

int gapro_eval_batch(gapro_ctx* ctx, void* stream_, int32_t n_scenes, const gapro_eval_scene* h_scenes,
                     gapro_eval_scene* d_scenes, int64_t n_total_points, int32_t sem_gt_dtype, const void* d_sem_gt,
                     int32_t inst_gt_dtype, const void* d_inst_gt, int32_t sem_ps_dtype, const void* d_sem_ps,
                     int32_t inst_ps_dtype, const void* d_inst_ps, const float* d_prob, int32_t n_thresholds,
                     const float* h_thresholds, int32_t scannet_remap, int32_t num_classes, void* d_workspace,
                     size_t workspace_bytes, float* d_max_iou, float* d_gt_cls, int64_t* d_conf, int64_t* d_kept,
                     int32_t* d_status) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  const int K = n_thresholds, B = K + 1;
  const bool pairs = d_inst_gt || d_inst_ps;  // false: confusion-only, the instance dtype codes are ignored
  if (!pairs) inst_gt_dtype = inst_ps_dtype = GAPRO_LABEL_I64;
  if (n_scenes < 1 || n_scenes > 65535 || !h_scenes || !d_scenes || n_total_points < 0 || K < 0 ||
      K > GAPRO_EVAL_MAX_THRESHOLDS || (K > 0 && (!h_thresholds || (n_total_points > 0 && !d_prob))) ||
      num_classes < 1 || num_classes > 128 || !d_workspace || (pairs && (!d_max_iou || !d_gt_cls)) || !d_conf ||
      !d_kept || !d_status ||
      (n_total_points > 0 && (!d_sem_gt || !d_sem_ps || (pairs && (!d_inst_gt || !d_inst_ps)))))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_eval_batch: bad argument");
  if (!with_label_type(sem_gt_dtype, [](auto) {}) || !with_label_type(inst_gt_dtype, [](auto) {}) ||
      !with_ps_type(sem_ps_dtype, [](auto) {}) || !with_ps_type(inst_ps_dtype, [](auto) {}))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_eval_batch: unsupported label dtype code");
  Thresholds thr = {};
  for (int j = 0; j < K; ++j) {
    thr.t[j] = h_thresholds[j];
    if (!(thr.t[j] == thr.t[j]) || (j > 0 && !(thr.t[j] >= thr.t[j - 1])))
      return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_eval_batch: thresholds must be ascending and not NaN");
  }
  // the scenes must be laid out as gapro_eval_batch_workspace_bytes planned them and lie inside the arrays
  size_t bytes = 0;
  long long rows = 0, n_max = 0, gt_max = 0, ps_max = 0, cells_max = 0;
  for (int i = 0; i < n_scenes; ++i) {
    const gapro_eval_scene& s = h_scenes[i];
    if (s.n_points < 0 || s.point_offset < 0 || s.point_offset > n_total_points ||
        s.n_points > n_total_points - s.point_offset || s.max_gt < 1 || s.max_ps < 1 || s.ws_offset != (int64_t)bytes ||
        s.row_offset != rows)
      return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_eval_batch: scene %d: bad descriptor", i);
    bytes += scene_bytes(s.max_gt, s.max_ps, B);
    rows += (long long)B * s.max_gt;
    n_max = std::max<long long>(n_max, s.n_points);
    gt_max = std::max<long long>(gt_max, s.max_gt);
    ps_max = std::max<long long>(ps_max, s.max_ps);
    cells_max = std::max<long long>(cells_max, (long long)s.max_gt + s.max_ps + (long long)(s.max_gt + 1) * (s.max_ps + 1));
  }
  if (workspace_bytes < bytes) return gapro_fail(ctx, GAPRO_ERR_WORKSPACE, "gapro_eval_batch: workspace too small");
  hipStream_t stream = (hipStream_t)stream_;
  const int C = num_classes, CC = num_classes * num_classes;
  GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(d_scenes, h_scenes, (size_t)n_scenes * sizeof(gapro_eval_scene),
                                      hipMemcpyHostToDevice, stream));
  GAPRO_HIP_CHECK(ctx, hipMemsetAsync(d_conf, 0, (size_t)B * CC * sizeof(int64_t), stream));
  GAPRO_HIP_CHECK(ctx, hipMemsetAsync(d_kept, 0, (size_t)n_scenes * B * sizeof(int64_t), stream));
  GAPRO_HIP_CHECK(ctx, hipMemsetAsync(d_status, 0, (size_t)n_scenes * sizeof(int32_t), stream));
  const long long words_max = (long long)B * std::max<long long>(gt_max + ps_max, (gt_max + 1) * (ps_max + 1) + ps_max);
  hipLaunchKernelGGL(k_evb_init, dim3(grid_for(words_max, 4, 256), n_scenes), dim3(kThreads), 0, stream, d_scenes,
                     d_workspace, B);
  if (n_max > 0)
    with_label_type(sem_gt_dtype, [&](auto sgt) {
      with_label_type(inst_gt_dtype, [&](auto igt) {
        with_ps_type(sem_ps_dtype, [&](auto sps) {
          with_ps_type(inst_ps_dtype, [&](auto ips) {
            using TGS = std::remove_const_t<std::remove_pointer_t<decltype(sgt)>>;
            using TGI = std::remove_const_t<std::remove_pointer_t<decltype(igt)>>;
            using TPS = std::remove_const_t<std::remove_pointer_t<decltype(sps)>>;
            using TPI = std::remove_const_t<std::remove_pointer_t<decltype(ips)>>;
            hipLaunchKernelGGL((k_evb_points<TGS, TGI, TPS, TPI>), dim3(grid_for(n_max, 4, 128), n_scenes),
                               dim3(kThreads), 0, stream, d_scenes, (const TGS*)d_sem_gt, (const TGI*)d_inst_gt,
                               (const TPS*)d_sem_ps, (const TPI*)d_inst_ps, d_prob, thr, K, (int)(scannet_remap != 0),
                               C, d_workspace, (long long*)d_conf, (long long*)d_kept, (int*)d_status);
          });
        });
      });
    });
  if (B > 1) {
    hipLaunchKernelGGL(k_evb_suffix, dim3(grid_for(cells_max, 4, 256), n_scenes), dim3(kThreads), 0, stream, d_scenes,
                       d_workspace, B);
    hipLaunchKernelGGL(k_evb_suffix_counts, dim3(grid_for((long long)CC + n_scenes, 1, 64)), dim3(kThreads), 0, stream,
                       (long long*)d_conf, CC, (long long*)d_kept, (int)n_scenes, B);
  }
  if (d_max_iou && d_gt_cls) {
    hipLaunchKernelGGL(k_evb_ps_count, dim3(grid_for((long long)B * ps_max, 1, 64), n_scenes), dim3(kThreads), 0,
                       stream, d_scenes, d_workspace, B);
    with_label_type(sem_gt_dtype, [&](auto sgt) {
      with_ps_type(sem_ps_dtype, [&](auto sps) {
        using TGS = std::remove_const_t<std::remove_pointer_t<decltype(sgt)>>;
        using TPS = std::remove_const_t<std::remove_pointer_t<decltype(sps)>>;
        hipLaunchKernelGGL((k_evb_finalize<TGS, TPS>), dim3(grid_for((long long)B * gt_max, 1, 64), n_scenes),
                           dim3(kThreads), 0, stream, d_scenes, (const TGS*)d_sem_gt, (const TPS*)d_sem_ps,
                           (int)(scannet_remap != 0), d_workspace, B, d_max_iou, d_gt_cls);
      });
    });
  }
  GAPRO_LAUNCH_CHECK(ctx);
  return GAPRO_OK;
}

}  // extern "C"
