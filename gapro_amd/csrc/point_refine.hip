// Point-level labels inside GP-labelled superpoints (include/gapro_hip.h, "Point-level labels"): the two memory-bound
// passes on either side of the batch's one gapro_svgp_predict_batch launch.
//   gather  every point of a refined superpoint -> a row of the launch's row table (its features, its point index)
//   apply   mu / var broadcast for every point, then the predict outputs of every row -> the row's point
//   expand  ("compete") the row list of the predict launch: a gathered row once per fit that tested its superpoint
//   compete ("compete") the ordered merge replayed per point over those fits' outputs -> the row's point
// No reference counterpart: the reference labels whole superpoints (gen_ps_utils.py:438-480).  Batched over the scenes of
// a batch like gapro_broadcast_labels_batch (grid.y = scene), with a per-scene struct of its own.
#include "common.h"
#include "exact_sum.h"
#include "launch_util.h"
#include "wave_reduce.h"

#include <algorithm>

namespace {

constexpr int kThreads = 256;
constexpr long long kMaxRows = 0x7fffffffLL;  // row indices are int32 (the predict ABI)
constexpr int kMaxGridY = 65535;

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

// The merge replayed for gathered row j of a block ("compete" and "vote"): best = 0.0f (the merge's start for a superpoint
// in several boxes, gen_ps_utils.py:367); the block's segments in tester order, those of a model with non-zero status
// skipped (its rows may hold nothing); strict float32 <: the first maximum, a NaN never wins.  Returns the position of
// the taking segment inside the block (-1: none took the row), its output row in *at and its probability in *best.
__device__ __forceinline__ int take_row(const gapro_point_refine_block& blk, long long j,
                                        const gapro_point_refine_segment* __restrict__ segs, long long n_rows2,
                                        const float* __restrict__ probs_new, const int* __restrict__ status,
                                        float* best_out, long long* at_out) {
  float best = 0.0f;
  int took = -1;
  long long at = -1;
  for (int s = 0; s < blk.n_seg; ++s) {
    const gapro_point_refine_segment sg = segs[blk.seg_start + s];
    if (status && status[sg.model] != 0) continue;
    const long long o = sg.out_start + j;
    if (o < 0 || o >= n_rows2) continue;
    const float p = probs_new[o];
    if (best < p) {
      best = p;
      took = s;
      at = o;
    }
  }
  *best_out = best;
  *at_out = at;
  return took;
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
    long long i = -1;
    if (b >= 0) {
      const gapro_point_refine_block blk = blocks[b];
      float best;
      long long at;
      const int s = take_row(blk, r - blk.row_start, segs, n_rows2, probs_new, status, &best, &at);
      if (s >= 0) {
        took = segs[blk.seg_start + s].model;
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

// "vote": one workgroup per block (= refined superpoint), its rows dealt to the lanes in strides.  A CANDIDATE is a
// (segment, label) pair, 2 n_seg per block: s_cnt[2 s + label] counts the rows that segment s took with that label and
// s_box holds the box it argues for.  Integer LDS atomics only; the three sums are int64 fixed point, so neither the
// gather order nor the order of the lanes reaches a result bit.
constexpr int kVoteMaxSeg = 2048;  // 2 * 2 * kVoteMaxSeg ints of dynamic LDS = 32 KiB at most

// the shift of a block's exact sums (exact_sum.h) from the bits of the largest finite magnitude among its voting rows
__device__ __forceinline__ int vote_shift(unsigned absmax_bits, int n) {
  return fixed_point_shift((double)__uint_as_float(absmax_bits), n);
}

__device__ __forceinline__ float vote_mean(long long sum, int k, int count, bool poisoned) {
  if (poisoned) return __uint_as_float(0x7fc00000u);
  return (float)fixed_mean(sum, k, (double)count);
}

__global__ __launch_bounds__(kThreads) void k_refine_vote(
    const gapro_point_refine_vote_scene* __restrict__ scenes, const gapro_point_refine_model* __restrict__ models,
    const int* __restrict__ model_boxes, const gapro_point_refine_block* __restrict__ blocks, int n_blocks,
    const int* __restrict__ block_spp, const gapro_point_refine_segment* __restrict__ segs, int max_seg,
    long long n_rows2, const float* __restrict__ probs_new, const unsigned char* __restrict__ labels,
    const float* __restrict__ mu_r, const float* __restrict__ var_r, const int* __restrict__ status,
    int* __restrict__ block_out) {
  extern __shared__ int s_dyn[];
  int* s_cnt = s_dyn;
  int* s_box = s_dyn + 2 * max_seg;
  __shared__ unsigned s_amax[3];             // bits of the largest finite |p_new|, |mu|, |var| among the voting rows
  __shared__ unsigned long long s_key[2];    // (votes, ~box) of the winner box; (voters, ~segment) of its representative
  __shared__ unsigned long long s_sum[3];
  __shared__ int s_poison;
  const int tid = threadIdx.x;
  for (int b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const gapro_point_refine_block blk = blocks[b];
    const int nc = 2 * blk.n_seg;
    for (int c = tid; c < nc; c += kThreads) {
      s_cnt[c] = 0;
      s_box[c] = model_boxes[2 * segs[blk.seg_start + (c >> 1)].model + (c & 1)];
    }
    if (tid < 3) { s_amax[tid] = 0u; s_sum[tid] = 0ull; }
    if (tid < 2) s_key[tid] = 0ull;
    if (tid == 0) s_poison = 0;
    __syncthreads();
    // 1. take: every row votes for the box of the segment that took it
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int j = tid; j < blk.n_rows; j += kThreads) {
      float best;
      long long at;
      const int s = take_row(blk, j, segs, n_rows2, probs_new, status, &best, &at);
      if (s < 0) continue;
      atomicAdd(&s_cnt[2 * s + (labels[at] != 0 ? 1 : 0)], 1);
      const float m = mu_r[at], v = var_r[at];
      if (isfinite(best)) a0 = fmaxf(a0, best);
      if (isfinite(m)) a1 = fmaxf(a1, fabsf(m));
      if (isfinite(v)) a2 = fmaxf(a2, fabsf(v));
    }
    {  // one atomic per wave; every lane is here (the row loop has ended): non-negative floats order like their bits
      const unsigned m0 = wave_max(__float_as_uint(a0)), m1 = wave_max(__float_as_uint(a1)),
                     m2 = wave_max(__float_as_uint(a2));
      if ((tid & 63) == 0) {
        if (m0) atomicMax(&s_amax[0], m0);
        if (m1) atomicMax(&s_amax[1], m1);
        if (m2) atomicMax(&s_amax[2], m2);
      }
    }
    __syncthreads();
    // 2. the box with the most votes, the lowest index among equals
    for (int c = tid; c < nc; c += kThreads) {
      if (s_cnt[c] == 0) continue;
      const int box = s_box[c];
      unsigned votes = 0;
      for (int e = 0; e < nc; ++e) votes += s_box[e] == box ? (unsigned)s_cnt[e] : 0u;
      atomicMax(&s_key[0], ((unsigned long long)votes << 32) | (0xffffffffu - (unsigned)box));
    }
    __syncthreads();
    const unsigned long long key_x = s_key[0];
    if (key_x == 0ull) {  // 5. nobody voted: the merge's values stay (uniform over the workgroup)
      if (tid == 0 && block_out) { block_out[3 * b] = -1; block_out[3 * b + 1] = -1; block_out[3 * b + 2] = 0; }
      __syncthreads();
      continue;
    }
    const int X = (int)(0xffffffffu - (unsigned)(key_x & 0xffffffffull));
    // 3. the fit that took the most voters for X, the earliest tester among equals
    for (int c = tid; c < nc; c += kThreads)
      if (s_cnt[c] > 0 && s_box[c] == X)
        atomicMax(&s_key[1], ((unsigned long long)(unsigned)s_cnt[c] << 32) | (0xffffffffu - (unsigned)(c >> 1)));
    __syncthreads();
    const unsigned long long key_f = s_key[1];
    const int sf = (int)(0xffffffffu - (unsigned)(key_f & 0xffffffffull));
    const int nf = (int)(key_f >> 32);
    const int k0 = vote_shift(s_amax[0], blk.n_rows), k1 = vote_shift(s_amax[1], blk.n_rows),
              k2 = vote_shift(s_amax[2], blk.n_rows);
    // 4. exact sums: p_new over every voter for X, mu and var over those the representative took.  take_row runs a
    // second time per row (n_seg reads) instead of keeping every row's verdict: a block has no bound on its rows
    long long q0 = 0, q1 = 0, q2 = 0;
    int poison = 0;
    for (int j = tid; j < blk.n_rows; j += kThreads) {
      float best;
      long long at;
      const int s = take_row(blk, j, segs, n_rows2, probs_new, status, &best, &at);
      if (s < 0 || s_box[2 * s + (labels[at] != 0 ? 1 : 0)] != X) continue;
      if (isfinite(best)) q0 += to_fixed((double)best, k0); else poison |= 1;
      if (s != sf) continue;
      const float m = mu_r[at], v = var_r[at];
      if (isfinite(m)) q1 += to_fixed((double)m, k1); else poison |= 2;
      if (isfinite(v)) q2 += to_fixed((double)v, k2); else poison |= 4;
    }
    q0 = wave_sum(q0); q1 = wave_sum(q1); q2 = wave_sum(q2);
    poison = wave_or(poison);
    if ((tid & 63) == 0) {
      if (q0) atomicAdd(&s_sum[0], (unsigned long long)q0);
      if (q1) atomicAdd(&s_sum[1], (unsigned long long)q1);
      if (q2) atomicAdd(&s_sum[2], (unsigned long long)q2);
      if (poison) atomicOr(&s_poison, poison);
    }
    __syncthreads();
    if (tid == 0) {
      const gapro_point_refine_vote_scene& t = scenes[blk.scene];
      const int sp = block_spp[b];
      const int model = segs[blk.seg_start + sf].model;
      const gapro_point_refine_model m = models[model];
      const bool second = s_box[2 * sf] != X;
      t.sem_spp[sp] = second ? m.sem2 : m.sem1;
      t.inst_spp[sp] = second ? m.inst2 : m.inst1;
      t.prob_spp[sp] = vote_mean((long long)s_sum[0], k0, blk.n_rows, s_poison & 1);
      t.mu_spp[sp] = vote_mean((long long)s_sum[1], k1, nf, s_poison & 2);
      t.var_spp[sp] = vote_mean((long long)s_sum[2], k2, nf, s_poison & 4);
      if (block_out) { block_out[3 * b] = model; block_out[3 * b + 1] = X; block_out[3 * b + 2] = (int)(key_x >> 32); }
    }
    __syncthreads();
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
  hipLaunchKernelGGL(k_refine_clear, dim3(grid_for(s_max, 1, 256), ny), dim3(kThreads), 0, stream, d_scenes);
  hipLaunchKernelGGL(k_refine_gather, dim3(grid_for(n_max, 1, n_scenes >= 8 ? 256 : 2048), ny), dim3(kThreads), 0, stream,
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
  hipLaunchKernelGGL(k_refine_mu_var, dim3(grid_for(n_max, 1, n_scenes >= 8 ? 256 : 2048), (unsigned)n_scenes),
                     dim3(kThreads), 0, stream, d_scenes);
  if (n_models > 0 && t_max > 0) {
    GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(d_models, h_models, (size_t)n_models * sizeof(gapro_point_refine_model),
                                        hipMemcpyHostToDevice, stream));
    const int gx = grid_for(t_max, 1, n_models >= 64 ? 64 : 1024);
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
  hipLaunchKernelGGL(k_refine_expand, dim3(grid_for(n_rows, 1, 2048)), dim3(kThreads), 0, stream, d_blocks, (int)n_blocks,
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
  hipLaunchKernelGGL(k_refine_compete, dim3(grid_for(n_rows, 1, 2048)), dim3(kThreads), 0, stream, d_scenes, d_models,
                     d_blocks, (int)n_blocks, d_segs, (long long)n_rows, (long long)n_rows2, d_row_point, d_probs_new,
                     d_labels, d_mu, d_var, d_model_status, d_row_model);
  GAPRO_LAUNCH_CHECK(ctx);
  return GAPRO_OK;
}

int gapro_point_refine_vote(gapro_ctx* ctx, void* stream_, int32_t n_scenes,
                            const gapro_point_refine_vote_scene* h_scenes, gapro_point_refine_vote_scene* d_scenes,
                            int32_t n_models, const gapro_point_refine_model* h_models,
                            gapro_point_refine_model* d_models, const int32_t* h_model_boxes, int32_t* d_model_boxes,
                            int32_t n_blocks, const gapro_point_refine_block* h_blocks,
                            gapro_point_refine_block* d_blocks, const int32_t* h_block_spp, int32_t* d_block_spp,
                            int32_t n_segs, const gapro_point_refine_segment* h_segs,
                            gapro_point_refine_segment* d_segs, int64_t n_rows, int64_t n_rows2,
                            const float* d_probs_new, const uint8_t* d_labels, const float* d_mu, const float* d_var,
                            const int32_t* d_model_status, int32_t* d_block_out) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  if (n_scenes < 0 || n_models < 0 || n_blocks < 0 || n_segs < 0 || n_rows < 0 || n_rows > kMaxRows || n_rows2 < 0 ||
      n_rows2 > kMaxRows)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG,
                      "gapro_point_refine_vote: bad argument (%d scenes, %d models, %d blocks, %d segments, "
                      "%lld -> %lld rows)",
                      (int)n_scenes, (int)n_models, (int)n_blocks, (int)n_segs, (long long)n_rows, (long long)n_rows2);
  if (n_scenes == 0 || n_blocks == 0) return GAPRO_OK;
  if (!h_scenes || !d_scenes || !h_blocks || !d_blocks || !h_block_spp || !d_block_spp)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_point_refine_vote: null argument");
  if (n_segs > 0 && (!h_segs || !d_segs || !h_models || !d_models || !h_model_boxes || !d_model_boxes ||
                     n_models == 0 || !d_probs_new || !d_labels || !d_mu || !d_var))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_point_refine_vote: null argument");
  for (int i = 0; i < n_scenes; ++i) {
    const gapro_point_refine_vote_scene& t = h_scenes[i];
    if (t.n_spps <= 0 || !t.sem_spp || !t.inst_spp || !t.prob_spp || !t.mu_spp || !t.var_spp)
      return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_point_refine_vote: scene %d: bad argument", i);
  }
  // equal boxes: both labels of a segment would argue for one box, two candidates where rule 3 counts one
  for (int k = 0; k < n_models; ++k)
    if (h_models[k].scene < 0 || h_models[k].scene >= n_scenes || h_model_boxes[2 * k] < 0 ||
        h_model_boxes[2 * k + 1] < 0 || h_model_boxes[2 * k] == h_model_boxes[2 * k + 1])
      return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_point_refine_vote: model %d: scene %d, boxes %d, %d", k,
                        (int)h_models[k].scene, (int)h_model_boxes[2 * k], (int)h_model_boxes[2 * k + 1]);
  if (const char* why = check_blocks(n_blocks, h_blocks, n_segs, h_segs, n_rows, n_rows2, n_scenes, n_models))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_point_refine_vote: %s", why);
  int max_seg = 1;
  for (int b = 0; b < n_blocks; ++b) {
    if (h_block_spp[b] < 0 || h_block_spp[b] >= h_scenes[h_blocks[b].scene].n_spps)
      return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_point_refine_vote: block %d: superpoint %d of scene %d", b,
                        (int)h_block_spp[b], (int)h_blocks[b].scene);
    max_seg = std::max(max_seg, (int)h_blocks[b].n_seg);
  }
  if (max_seg > kVoteMaxSeg)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_point_refine_vote: a block of %d segments, %d at most", max_seg,
                      kVoteMaxSeg);
  hipStream_t stream = (hipStream_t)stream_;
  GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(d_scenes, h_scenes, (size_t)n_scenes * sizeof(gapro_point_refine_vote_scene),
                                      hipMemcpyHostToDevice, stream));
  GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(d_blocks, h_blocks, (size_t)n_blocks * sizeof(gapro_point_refine_block),
                                      hipMemcpyHostToDevice, stream));
  GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(d_block_spp, h_block_spp, (size_t)n_blocks * sizeof(int32_t),
                                      hipMemcpyHostToDevice, stream));
  if (n_segs > 0) {
    GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(d_models, h_models, (size_t)n_models * sizeof(gapro_point_refine_model),
                                        hipMemcpyHostToDevice, stream));
    GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(d_model_boxes, h_model_boxes, (size_t)n_models * 2 * sizeof(int32_t),
                                        hipMemcpyHostToDevice, stream));
    GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(d_segs, h_segs, (size_t)n_segs * sizeof(gapro_point_refine_segment),
                                        hipMemcpyHostToDevice, stream));
  }
  const size_t lds = (size_t)4 * max_seg * sizeof(int);
  hipLaunchKernelGGL(k_refine_vote, dim3((unsigned)std::min(n_blocks, 1 << 18)), dim3(kThreads), lds, stream, d_scenes,
                     d_models, d_model_boxes, d_blocks, (int)n_blocks, d_block_spp, d_segs, max_seg,
                     (long long)n_rows2, d_probs_new, d_labels, d_mu, d_var, d_model_status, d_block_out);
  GAPRO_LAUNCH_CHECK(ctx);
  return GAPRO_OK;
}

}  // extern "C"
