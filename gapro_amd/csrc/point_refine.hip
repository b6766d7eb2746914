// Point-level labels inside GP-labelled superpoints (include/gapro_hip.h, "Point-level labels"): the two memory-bound
// passes on either side of the batch's one gapro_svgp_predict_batch launch.
//   gather  every point of a refined superpoint -> a row of the launch's row table (its features, its point index)
//   apply   mu / var broadcast for every point, then the predict outputs of every row -> the row's point
//   expand  ("compete") the row list of the predict launch: a gathered row once per fit that tested its superpoint
//   compete ("compete") the ordered merge replayed per point over those fits' outputs -> the row's point
// No reference counterpart: the reference labels whole superpoints (gen_ps_utils.py:438-480).  Batched over the scenes of
// a batch like gapro_broadcast_labels_batch (grid.y = scene), with a per-scene struct of its own.
#include "common.h"

#include <algorithm>

namespace {

constexpr int kThreads = 256;
constexpr long long kMaxRows = 0x7fffffffLL;  // row indices are int32 (the predict ABI)
constexpr int kMaxGridY = 65535;

inline int grid_for(long long n, int cap) {
  long long g = (n + kThreads - 1) / kThreads;
  if (g < 1) g = 1;
  return (int)(g > cap ? cap : g);
}

__global__ __launch_bounds__(kThreads) void k_refine_clear(const gapro_point_refine_scene* __restrict__ scenes) {
  const gapro_point_refine_scene& t = scenes[blockIdx.y];
  int* __restrict__ cursor = t.cursor;
  const int S = t.n_spps;
  for (int s = blockIdx.x * kThreads + threadIdx.x; s < S; s += gridDim.x * kThreads) cursor[s] = 0;
}

// A workgroup takes runs of kThreads consecutive points.  Phase 1, one thread per point: the point's row (block start +
// the block's next free position) or -1, kept in LDS.  Phase 2, the whole workgroup: the features of the run are read
// as ONE contiguous stretch of kThreads * d floats (point-major, coalesced) and every float goes to its point's row;
// the d floats of a row are consecutive lanes, so the stores are d-float segments.
// The cursor atomics are NOT aggregated per wave: neighbouring points often share a superpoint and then hit one
// address, which the L2 serialises.  An aggregation (one atomic per run of equal superpoints in a wave) is left for the
// day the gather span of tools/bench_point_refine.py shows that it matters.
__global__ __launch_bounds__(kThreads) void k_refine_gather(const gapro_point_refine_scene* __restrict__ scenes, int d,
                                                            long long n_rows, float* __restrict__ row_feats,
                                                            int* __restrict__ row_point) {
  const gapro_point_refine_scene& t = scenes[blockIdx.y];
  const long long n = t.n_points;
  const int S = t.n_spps;
  const int* __restrict__ spp_inv = t.spp_inv;
  const float* __restrict__ feats = t.feats;
  const long long* __restrict__ sp_row = (const long long*)t.sp_row;
  int* __restrict__ cursor = t.cursor;
  __shared__ long long s_row[kThreads];
  for (long long base = (long long)blockIdx.x * kThreads; base < n; base += (long long)gridDim.x * kThreads) {
    const long long i = base + threadIdx.x;
    long long row = -1;
    if (i < n) {
      const int sp = spp_inv[i];
      if (sp >= 0 && sp < S) {
        const long long first = sp_row[sp];
        if (first >= 0) {
          row = first + atomicAdd(&cursor[sp], 1);
          if (row >= n_rows) row = -1;  // a plan that does not match the point counts: dropped, never written
        }
      }
      if (row >= 0) row_point[row] = (int)i;
    }
    s_row[threadIdx.x] = row;
    __syncthreads();
    const long long left = n - base;
    const int pts = left < kThreads ? (int)left : kThreads;
    const float* __restrict__ src = feats + base * d;
    for (int j = threadIdx.x; j < pts * d; j += kThreads) {
      const int p = j / d;
      const long long r = s_row[p];
      if (r >= 0) row_feats[r * d + (j - p * d)] = src[j];
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kThreads) void k_refine_mu_var(const gapro_point_refine_scene* __restrict__ scenes) {
  const gapro_point_refine_scene& t = scenes[blockIdx.y];
  const long long n = t.n_points;
  const int* __restrict__ spp_inv = t.spp_inv;
  const float* __restrict__ mu_spp = t.mu_spp;
  const float* __restrict__ var_spp = t.var_spp;
  float* __restrict__ mu = t.mu;
  float* __restrict__ var = t.var;
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
    const int r = spp_inv[i];
    mu[i] = mu_spp[r];
    var[i] = var_spp[r];
  }
}

// grid.y = model: the rows of a model are read in order (coalesced); the five values go to the row's point
__global__ __launch_bounds__(kThreads) void k_refine_apply(const gapro_point_refine_scene* __restrict__ scenes,
                                                           const gapro_point_refine_model* __restrict__ models,
                                                           long long n_rows, const int* __restrict__ row_point,
                                                           const float* __restrict__ probs_new,
                                                           const unsigned char* __restrict__ labels,
                                                           const float* __restrict__ mu_r, const float* __restrict__ var_r,
                                                           const int* __restrict__ status) {
  const gapro_point_refine_model m = models[blockIdx.y];
  if (status && status[blockIdx.y] != 0) return;  // the scene is given up on the host; its rows may hold nothing
  const gapro_point_refine_scene& t = scenes[m.scene];
  const long long n = t.n_points;
  int* __restrict__ sem = t.sem;
  int* __restrict__ inst = t.inst;
  float* __restrict__ prob = t.prob;
  float* __restrict__ mu = t.mu;
  float* __restrict__ var = t.var;
  for (int k = blockIdx.x * kThreads + threadIdx.x; k < m.t; k += gridDim.x * kThreads) {
    const long long r = m.row_offset + k;
    if (r < 0 || r >= n_rows) continue;
    const long long i = row_point[r];
    if (i < 0 || i >= n) continue;
    const bool second = labels[r] != 0;
    sem[i] = second ? m.sem2 : m.sem1;
    inst[i] = second ? m.inst2 : m.inst1;
    prob[i] = probs_new[r];
    mu[i] = mu_r[r];
    var[i] = var_r[r];
  }
}

// "compete": the block that holds gathered row r, by bisection over the blocks' first rows (ascending, disjoint: checked
// on the host), or -1 for a row between two blocks.  A block has 1 to a few hundred rows, so rows, not blocks, are
// dealt to the lanes: consecutive lanes take consecutive rows and the reads of a segment are contiguous.
__device__ __forceinline__ int block_of_row(const gapro_point_refine_block* __restrict__ blocks, int n_blocks,
                                            long long r) {
  int lo = 0, hi = n_blocks;  // the last block with row_start <= r lies in [lo, hi)
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (blocks[mid].row_start <= r) lo = mid; else hi = mid;
  }
  const long long first = blocks[lo].row_start;
  return (r >= first && r - first < blocks[lo].n_rows) ? lo : -1;
}

__global__ __launch_bounds__(kThreads) void k_refine_expand(const gapro_point_refine_block* __restrict__ blocks,
                                                            int n_blocks,
                                                            const gapro_point_refine_segment* __restrict__ segs,
                                                            long long n_rows, long long n_rows2,
                                                            int* __restrict__ rows) {
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long r = (long long)blockIdx.x * kThreads + threadIdx.x; r < n_rows; r += stride) {
    const int b = block_of_row(blocks, n_blocks, r);
    if (b < 0) continue;
    const gapro_point_refine_block blk = blocks[b];
    const long long j = r - blk.row_start;
    for (int s = 0; s < blk.n_seg; ++s) {
      const long long o = segs[blk.seg_start + s].out_start + j;
      if (o >= 0 && o < n_rows2) rows[o] = (int)r;
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_refine_compete(
    const gapro_point_refine_scene* __restrict__ scenes, const gapro_point_refine_model* __restrict__ models,
    const gapro_point_refine_block* __restrict__ blocks, int n_blocks,
    const gapro_point_refine_segment* __restrict__ segs, long long n_rows, long long n_rows2,
    const int* __restrict__ row_point, const float* __restrict__ probs_new, const unsigned char* __restrict__ labels,
    const float* __restrict__ mu_r, const float* __restrict__ var_r, const int* __restrict__ status,
    int* __restrict__ row_model) {
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long r = (long long)blockIdx.x * kThreads + threadIdx.x; r < n_rows; r += stride) {
    const int b = block_of_row(blocks, n_blocks, r);
    int took = -1;
    long long at = -1;
    long long i = -1;
    if (b >= 0) {
      const gapro_point_refine_block blk = blocks[b];
      const long long j = r - blk.row_start;
      float best = 0.0f;  // the merge's start for a superpoint in several boxes (gen_ps_utils.py:367)
      for (int s = 0; s < blk.n_seg; ++s) {
        const gapro_point_refine_segment sg = segs[blk.seg_start + s];
        if (status && status[sg.model] != 0) continue;  // its rows may hold nothing
        const long long o = sg.out_start + j;
        if (o < 0 || o >= n_rows2) continue;
        const float p = probs_new[o];
        if (best < p) {  // strict, float32: the first maximum; a NaN never wins
          best = p;
          took = sg.model;
          at = o;
        }
      }
      if (took >= 0) {
        const gapro_point_refine_scene& t = scenes[blk.scene];
        i = row_point[r];
        if (i < 0 || i >= t.n_points) {
          took = -1;
        } else {
          const gapro_point_refine_model m = models[took];
          const bool second = labels[at] != 0;
          t.sem[i] = second ? m.sem2 : m.sem1;
          t.inst[i] = second ? m.inst2 : m.inst1;
          t.prob[i] = best;
          t.mu[i] = mu_r[at];
          t.var[i] = var_r[at];
        }
      }
    }
    if (row_model) row_model[r] = took;
  }
}

// the checks expand and compete share: blocks ascending and disjoint inside [0, n_rows), segments inside [0, n_rows2)
const char* check_blocks(int n_blocks, const gapro_point_refine_block* h_blocks, int n_segs,
                         const gapro_point_refine_segment* h_segs, long long n_rows, long long n_rows2, int n_scenes,
                         int n_models) {
  long long end = 0;
  for (int b = 0; b < n_blocks; ++b) {
    const gapro_point_refine_block& k = h_blocks[b];
    if (k.n_rows <= 0 || k.row_start < end || k.row_start > n_rows - k.n_rows)
      return "a block outside the rows or out of order";
    end = k.row_start + k.n_rows;
    if (k.n_seg < 0 || k.seg_start < 0 || k.seg_start > n_segs - k.n_seg)
      return "a block's segments outside the segments";
    if (n_scenes >= 0 && (k.scene < 0 || k.scene >= n_scenes)) return "a block of no scene";
    for (int s = 0; s < k.n_seg; ++s) {
      const gapro_point_refine_segment& g = h_segs[k.seg_start + s];
      if (g.out_start < 0 || g.out_start > n_rows2 - k.n_rows) return "a segment outside the expanded rows";
      if (n_models >= 0 && (g.model < 0 || g.model >= n_models)) return "a segment of no model";
    }
  }
  return nullptr;
}

}  // namespace

extern "C" {

int gapro_point_refine_gather(gapro_ctx* ctx, void* stream_, int32_t n_scenes, int32_t feat_dim,
                              const gapro_point_refine_scene* h_scenes, gapro_point_refine_scene* d_scenes,
                              int64_t n_rows, float* d_row_feats, int32_t* d_row_point) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  if (n_scenes < 0 || n_scenes > kMaxGridY || feat_dim <= 0 || n_rows < 0 || n_rows > kMaxRows)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_point_refine_gather: bad argument (%d scenes, %lld rows)",
                      (int)n_scenes, (long long)n_rows);
  if (n_scenes == 0 || n_rows == 0) return GAPRO_OK;
  if (!h_scenes || !d_scenes || !d_row_feats || !d_row_point)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_point_refine_gather: null argument");
  long long n_max = 0;
  int s_max = 0;
  for (int i = 0; i < n_scenes; ++i) {
    const gapro_point_refine_scene& t = h_scenes[i];
    if (t.n_points <= 0 || t.n_spps <= 0 || !t.spp_inv || !t.feats || !t.sp_row || !t.cursor)
      return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_point_refine_gather: scene %d: bad argument", i);
    n_max = std::max<long long>(n_max, t.n_points);
    s_max = std::max(s_max, (int)t.n_spps);
  }
  hipStream_t stream = (hipStream_t)stream_;
  GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(d_scenes, h_scenes, (size_t)n_scenes * sizeof(gapro_point_refine_scene),
                                      hipMemcpyHostToDevice, stream));
  const unsigned ny = (unsigned)n_scenes;
  hipLaunchKernelGGL(k_refine_clear, dim3(grid_for(s_max, 256), ny), dim3(kThreads), 0, stream, d_scenes);
  hipLaunchKernelGGL(k_refine_gather, dim3(grid_for(n_max, n_scenes >= 8 ? 256 : 2048), ny), dim3(kThreads), 0, stream,
                     d_scenes, (int)feat_dim, (long long)n_rows, d_row_feats, d_row_point);
  GAPRO_LAUNCH_CHECK(ctx);
  return GAPRO_OK;
}

int gapro_point_refine_apply(gapro_ctx* ctx, void* stream_, int32_t n_scenes, const gapro_point_refine_scene* h_scenes,
                             gapro_point_refine_scene* d_scenes, int32_t n_models,
                             const gapro_point_refine_model* h_models, gapro_point_refine_model* d_models,
                             int64_t n_rows, const int32_t* d_row_point, const float* d_probs_new,
                             const uint8_t* d_labels, const float* d_mu, const float* d_var,
                             const int32_t* d_model_status) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  if (n_scenes < 0 || n_scenes > kMaxGridY || n_models < 0 || n_rows < 0 || n_rows > kMaxRows)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_point_refine_apply: bad argument (%d scenes, %d models, %lld rows)",
                      (int)n_scenes, (int)n_models, (long long)n_rows);
  if (n_scenes == 0) return GAPRO_OK;
  if (!h_scenes || !d_scenes)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_point_refine_apply: null argument");
  if (n_models > 0 && (!h_models || !d_models || !d_row_point || !d_probs_new || !d_labels || !d_mu || !d_var))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_point_refine_apply: null argument");
  long long n_max = 0;
  for (int i = 0; i < n_scenes; ++i) {
    const gapro_point_refine_scene& t = h_scenes[i];
    if (t.n_points <= 0 || t.n_spps <= 0 || !t.spp_inv || !t.mu_spp || !t.var_spp || !t.sem || !t.inst || !t.prob ||
        !t.mu || !t.var)
      return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_point_refine_apply: scene %d: bad argument", i);
    n_max = std::max<long long>(n_max, t.n_points);
  }
  int t_max = 0;
  for (int k = 0; k < n_models; ++k) {
    const gapro_point_refine_model& m = h_models[k];
    if (m.t < 0 || m.row_offset < 0 || m.row_offset + m.t > n_rows || m.scene < 0 || m.scene >= n_scenes)
      return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_point_refine_apply: model %d: rows [%lld, +%d) of %lld, scene %d", k,
                        (long long)m.row_offset, (int)m.t, (long long)n_rows, (int)m.scene);
    t_max = std::max(t_max, (int)m.t);
  }
  hipStream_t stream = (hipStream_t)stream_;
  GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(d_scenes, h_scenes, (size_t)n_scenes * sizeof(gapro_point_refine_scene),
                                      hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(k_refine_mu_var, dim3(grid_for(n_max, n_scenes >= 8 ? 256 : 2048), (unsigned)n_scenes),
                     dim3(kThreads), 0, stream, d_scenes);
  if (n_models > 0 && t_max > 0) {
    GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(d_models, h_models, (size_t)n_models * sizeof(gapro_point_refine_model),
                                        hipMemcpyHostToDevice, stream));
    const int gx = grid_for(t_max, n_models >= 64 ? 64 : 1024);
    for (int lo = 0; lo < n_models; lo += kMaxGridY) {  // grid.y holds at most 65535 models per launch
      const int ny = std::min(kMaxGridY, n_models - lo);
      hipLaunchKernelGGL(k_refine_apply, dim3(gx, (unsigned)ny), dim3(kThreads), 0, stream, d_scenes, d_models + lo,
                         (long long)n_rows, d_row_point, d_probs_new, d_labels, d_mu, d_var,
                         d_model_status ? d_model_status + lo : nullptr);
    }
  }
  GAPRO_LAUNCH_CHECK(ctx);
  return GAPRO_OK;
}

int gapro_point_refine_expand(gapro_ctx* ctx, void* stream_, int32_t n_blocks, const gapro_point_refine_block* h_blocks,
                              gapro_point_refine_block* d_blocks, int32_t n_segs,
                              const gapro_point_refine_segment* h_segs, gapro_point_refine_segment* d_segs,
                              int64_t n_rows, int64_t n_rows2, int32_t* d_rows) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  if (n_blocks < 0 || n_segs < 0 || n_rows < 0 || n_rows > kMaxRows || n_rows2 < 0 || n_rows2 > kMaxRows)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG,
                      "gapro_point_refine_expand: bad argument (%d blocks, %d segments, %lld -> %lld rows)", (int)n_blocks, (int)n_segs, (long long)n_rows, (long long)n_rows2);
  if (n_blocks == 0 || n_segs == 0) return GAPRO_OK;
  if (!h_blocks || !d_blocks || !h_segs || !d_segs || !d_rows)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_point_refine_expand: null argument");
  if (const char* why = check_blocks(n_blocks, h_blocks, n_segs, h_segs, n_rows, n_rows2, -1, -1))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_point_refine_expand: %s", why);
  hipStream_t stream = (hipStream_t)stream_;
  GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(d_blocks, h_blocks, (size_t)n_blocks * sizeof(gapro_point_refine_block),
                                      hipMemcpyHostToDevice, stream));
  GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(d_segs, h_segs, (size_t)n_segs * sizeof(gapro_point_refine_segment),
                                      hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(k_refine_expand, dim3(grid_for(n_rows, 2048)), dim3(kThreads), 0, stream, d_blocks, (int)n_blocks,
                     d_segs, (long long)n_rows, (long long)n_rows2, d_rows);
  GAPRO_LAUNCH_CHECK(ctx);
  return GAPRO_OK;
}

int gapro_point_refine_compete(gapro_ctx* ctx, void* stream_, int32_t n_scenes, const gapro_point_refine_scene* h_scenes,
                               gapro_point_refine_scene* d_scenes, int32_t n_models,
                               const gapro_point_refine_model* h_models, gapro_point_refine_model* d_models,
                               int32_t n_blocks, const gapro_point_refine_block* h_blocks,
                               gapro_point_refine_block* d_blocks, int32_t n_segs,
                               const gapro_point_refine_segment* h_segs, gapro_point_refine_segment* d_segs,
                               int64_t n_rows, int64_t n_rows2, const int32_t* d_row_point, const float* d_probs_new,
                               const uint8_t* d_labels, const float* d_mu, const float* d_var,
                               const int32_t* d_model_status, int32_t* d_row_model) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  if (n_scenes < 0 || n_models < 0 || n_blocks < 0 || n_segs < 0 || n_rows < 0 || n_rows > kMaxRows || n_rows2 < 0 ||
      n_rows2 > kMaxRows)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG,
                      "gapro_point_refine_compete: bad argument (%d scenes, %d models, %d blocks, %d segments, "
                      "%lld -> %lld rows)",
                      (int)n_scenes, (int)n_models, (int)n_blocks, (int)n_segs, (long long)n_rows, (long long)n_rows2);
  if (n_scenes == 0 || n_blocks == 0) return GAPRO_OK;
  if (!h_scenes || !d_scenes || !h_blocks || !d_blocks || !d_row_point)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_point_refine_compete: null argument");
  if (n_segs > 0 && (!h_segs || !d_segs || !h_models || !d_models || n_models == 0 || !d_probs_new || !d_labels ||
                     !d_mu || !d_var))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_point_refine_compete: null argument");
  for (int i = 0; i < n_scenes; ++i) {
    const gapro_point_refine_scene& t = h_scenes[i];
    if (t.n_points <= 0 || !t.sem || !t.inst || !t.prob || !t.mu || !t.var)
      return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_point_refine_compete: scene %d: bad argument", i);
  }
  for (int k = 0; k < n_models; ++k)
    if (h_models[k].scene < 0 || h_models[k].scene >= n_scenes)
      return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_point_refine_compete: model %d: scene %d", k,
                        (int)h_models[k].scene);
  if (const char* why = check_blocks(n_blocks, h_blocks, n_segs, h_segs, n_rows, n_rows2, n_scenes, n_models))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_point_refine_compete: %s", why);
  hipStream_t stream = (hipStream_t)stream_;
  GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(d_scenes, h_scenes, (size_t)n_scenes * sizeof(gapro_point_refine_scene),
                                      hipMemcpyHostToDevice, stream));
  GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(d_blocks, h_blocks, (size_t)n_blocks * sizeof(gapro_point_refine_block),
                                      hipMemcpyHostToDevice, stream));
  if (n_segs > 0) {
    GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(d_models, h_models, (size_t)n_models * sizeof(gapro_point_refine_model),
                                        hipMemcpyHostToDevice, stream));
    GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(d_segs, h_segs, (size_t)n_segs * sizeof(gapro_point_refine_segment),
                                        hipMemcpyHostToDevice, stream));
  }
  hipLaunchKernelGGL(k_refine_compete, dim3(grid_for(n_rows, 2048)), dim3(kThreads), 0, stream, d_scenes, d_models,
                     d_blocks, (int)n_blocks, d_segs, (long long)n_rows, (long long)n_rows2, d_row_point, d_probs_new,
                     d_labels, d_mu, d_var, d_model_status, d_row_model);
  GAPRO_LAUNCH_CHECK(ctx);
  return GAPRO_OK;
}

}  // extern "C"
