// The consumer's inference post-processing (include/gapro_hip.h, "Predicted instances"): ISBNet.get_instance
// (isbnet/model/isbnet.py:887-1005) with its nms (model_utils.py:77-169), custom_scatter_mean, superpoint_align and
// rle_encode_gpu_batch (isbnet/util/rle.py:47-69), without the float products of bit masks and without a host round trip
// per proposal.
// gapro_proposals_count:
//   score    a thread per query: softmax, clamp, product and square root in float64, rounded once
//   select   one workgroup: radix select of the pre_topk largest (score, lowest flat index first), sorted
//   pack     a wave per run of words of a row: the ballot of `logit >= thresh` over 64 voxels is the word; popcounts;
//            the sem2ins rows
//   points   one pass over the points: the ranges of v2p_map and spps, n(s)
//   filter   one workgroup: the status, the candidates with npoints >= npoint_thresh, in order
//   inter    a wave per same-class pair: sum of popcount(A & B), one float32 division
//   decay    matrix NMS, twice: a wave per candidate: the column maxima c, then the float64 decay, rounded once
//   nms      one workgroup: matrix (the updated scores sorted and cut) or standard (greedy, suppressed bitmap in LDS)
//   tally    c(k, s): one integer atomic per set bit of a point's voxel
//   trans    a workgroup per (row, chunk of points): transitions and points of m(k, .) in the chunk, no atomics
//   chunks   a wave per row: the transitions before each chunk, the row's transitions and points
//   finish   one workgroup: the rows with enough points and their run offsets by a prefix, the header
// gapro_proposals_fill:
//   rows     conf, label, box, query, run offsets
//   runs     the positions of the transitions in order (and the masks); then `lengths` turns every second into a length
// Integer atomics only, so every result is the same bits for every grid and every run.  The kernel boundaries on the
// stream are the only ordering.  A refusal is a status word written by `filter`: every later kernel returns at once.
// The softmax, the select / sort and the chunked run lengths (stages 1 and 7) are select_runs.h's, shared with
// spf_predict.hip; this file supplies its point bit (`mask_at`) and its row indexing: the chunk cells of a row belong
// to the row k before the last filter, which `final_row` gives for output row r.
#include "common.h"
#include "label_types.h"
#include "launch_util.h"
#include "select_runs.h"
#include "wave_reduce.h"

#include <cmath>
#include <cstdint>

namespace {

constexpr int kMaxSem = GAPRO_PROPOSALS_MAX_SEM2INS;
constexpr int kMaxRows = kMaxTopk + kMaxSem;
constexpr int kPackWords = 32, kPackUnroll = 4;  // words of a wave's run of `pack`, and of them in flight
constexpr int kTallyGridX = 256;   // workgroups along the points of one row of `tally`

enum { kFlagScore = 1, kFlagMask = 2, kFlagV2p = 4, kFlagVoxelSpp = 8, kFlagSpp = 16 };

struct PrScalars {  // the first 64 bytes of the workspace
  int flags;
  int status;      // set by k_pr_filter
  int n_cand;      // after `select`
  int n_np;        // after `filter`
  int n_nms;       // after `nms`
  int n_pre;       // rows into stage 5: the sem2ins rows and n_nms
  int n_rows;      // rows out
  int reserved;
  long long total_trans;  // 2 * total_runs
  long long pad[3];
};
static_assert(sizeof(PrScalars) == 64, "PrScalars is the first 64 bytes of the workspace");

struct PrDims {
  long long Q, V, N;   // rows of the mask input, voxels, points
  long long W;         // 64-bit words of a row of voxel bits
  long long chunk_len; // points of a chunk of `trans` / `runs`
  int C, S, Sv;        // classes, superpoint ids, columns of mask_logits (0: V)
  int P;               // candidates kept by `select`
  int R;               // rows, at most
  int n_sem, mode, nchunks;
  __host__ __device__ long long bit_rows() const { return mode == GAPRO_PROPOSALS_RLE ? 0 : Q + n_sem; }
  __host__ __device__ long long n_scores() const { return mode == GAPRO_PROPOSALS_FULL ? Q * C : 0; }
  __host__ __device__ long long spp_cells() const { return mode == GAPRO_PROPOSALS_FULL ? (long long)R * S : 0; }
};

struct PrWs {
  PrScalars* s;
  // cleared by the count's memset, up to `zero_end`
  unsigned* npoints;    // [Q + n_sem] set bits of a row
  int* rowbad;          // [Q] a non-finite value was read for the row
  unsigned* ntab;       // [S] points of a superpoint
  unsigned* chunk_ones; // [R][nchunks] points of a row's refined mask in a chunk
  unsigned* chunk_cnt;  // [R][nchunks] transitions of a chunk; after `finish` the transitions before it
  unsigned* row_trans;  // [R] transitions of a row
  unsigned* row_ones;   // [R] points of a row's refined mask
  unsigned* ctab;       // [R][S] c(k, s)
  char* zero_end;
  float* score;         // [Q * C]
  int* cand_q;          // [P] query, class and score of the candidates, sorted
  int* cand_cls;
  float* cand_score;
  int* surv_q;          // [P] ... of those with enough voxels
  int* surv_cls;
  float* surv_score;
  float* iou;           // [P][P], a < b of one class only
  float* comp;          // [P] matrix NMS: c_j
  float* new_score;     // [P] matrix NMS: the updated scores
  int* row_src;         // [R] row of `bits`
  int* row_label;       // [R]
  int* row_query;       // [R]
  float* row_conf;      // [R]
  int* final_row;       // [R] the row k of output row r
  long long* run_off;   // [R + 1] transitions before output row r
  unsigned long long* bits;  // [Q + n_sem][W]
};

__host__ __device__ inline size_t pr_ws(void* base, const PrDims& d, PrWs* w) {
  char* p = (char*)base;
  auto take = [&](size_t bytes) {
    char* q = p;
    p += (bytes + 15) & ~(size_t)15;
    return q;
  };
  const size_t P = (size_t)d.P, R = (size_t)d.R;
  w->s = (PrScalars*)take(sizeof(PrScalars));
  w->npoints = (unsigned*)take((size_t)d.bit_rows() * 4);
  w->rowbad = (int*)take((size_t)d.Q * 4);
  w->ntab = (unsigned*)take((size_t)d.S * 4);
  w->chunk_ones = (unsigned*)take(R * (size_t)d.nchunks * 4);
  w->chunk_cnt = (unsigned*)take(R * (size_t)d.nchunks * 4);
  w->row_trans = (unsigned*)take(R * 4);
  w->row_ones = (unsigned*)take(R * 4);
  w->ctab = (unsigned*)take((size_t)d.spp_cells() * 4);
  w->zero_end = p;
  w->score = (float*)take((size_t)d.n_scores() * 4);
  w->cand_q = (int*)take(P * 4);
  w->cand_cls = (int*)take(P * 4);
  w->cand_score = (float*)take(P * 4);
  w->surv_q = (int*)take(P * 4);
  w->surv_cls = (int*)take(P * 4);
  w->surv_score = (float*)take(P * 4);
  w->iou = (float*)take(P * P * 4);
  w->comp = (float*)take(P * 4);
  w->new_score = (float*)take(P * 4);
  w->row_src = (int*)take(R * 4);
  w->row_label = (int*)take(R * 4);
  w->row_query = (int*)take(R * 4);
  w->row_conf = (float*)take(R * 4);
  w->final_row = (int*)take(R * 4);
  w->run_off = (long long*)take((R + 1) * 8);
  w->bits = (unsigned long long*)take((size_t)d.bit_rows() * (size_t)d.W * 8);
  return (size_t)(p - (char*)base);
}

struct PrPar {  // gapro_proposals_params as the kernels read it
  int type_nms, topk, npoint_thresh, label_shift;
  float logit_thresh, final_score_thresh, nms_threshold;
  int sem[kMaxSem];
};

// ---- stage 1 -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_pr_score(void* base, PrDims d, const float* __restrict__ cls,
                                                       const float* __restrict__ conf) {
  PrWs w;
  pr_ws(base, d, &w);
  const int C = d.C;
  int bad = 0;
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long q = (long long)blockIdx.x * kThreads + threadIdx.x; q < d.Q; q += stride) {
    const float* row = cls + q * (C + 1);
    const RowSoftmax sm = row_softmax(row, C);
    if (!(sm.ok && isfinite(conf[q]))) {
      bad = kFlagScore;
      for (int c = 0; c < C; ++c) w.score[q * C + c] = 0.f;
      continue;
    }
    const double cf = conf[q] < 0.f ? 0.0 : (conf[q] > 1.f ? 1.0 : (double)conf[q]);
    for (int c = 0; c < C; ++c) w.score[q * C + c] = (float)sqrt(sm.times(row[c], cf)) + 0.f;  // + 0: never -0.0
  }
  if (bad) atomicOr(&w.s->flags, bad);
}

// One workgroup: the d.P largest (score, lowest index first), sorted, as candidates.
__global__ __launch_bounds__(kThreads) void k_pr_select(void* base, PrDims d, const float* __restrict__ nms_scores,
                                                        const int* __restrict__ nms_classes) {
  PrWs w;
  pr_ws(base, d, &w);
  __shared__ unsigned long long s_key[kMaxTopk];
  const int t = threadIdx.x;
  const bool full = d.mode == GAPRO_PROPOSALS_FULL;
  const float* __restrict__ score = full ? w.score : nms_scores;
  const unsigned n = (unsigned)(full ? d.Q * d.C : d.Q);
  if (!full) {  // the caller's scores
    int bad = 0;
    for (unsigned i = t; i < n; i += kThreads)
      if (!isfinite(score[i])) bad = kFlagScore;
    if (bad) atomicOr(&w.s->flags, bad);
  }
  select_topk(score, n, d.P, s_key);
  for (int j = t; j < d.P; j += kThreads) {
    const unsigned i = key_index(s_key[j]);
    w.cand_q[j] = full ? (int)(i / (unsigned)d.C) : (int)i;
    w.cand_cls[j] = full ? (int)(i % (unsigned)d.C) : nms_classes[i];
    w.cand_score[j] = score[i];
  }
  if (t == 0) w.s->n_cand = d.P;
}

// ---- stage 2 -----------------------------------------------------------------------------------------------------
struct PrMaskIn {
  const void* mask;        // f32[Q][Sv or V] or u8[Q][V]
  int mask_type;
  const void* voxel_spps;  // with Sv > 0
  int voxel_spps_i64;
  const void* sem;         // semantic_preds, with n_sem > 0
  int sem_i64;
};

// Bit (row, v) for v < V; the causes it meets go to *flags, a non-finite value read to *nf.
__device__ inline bool mask_bit(const PrDims& d, const PrMaskIn& in, const PrPar& par, long long row, long long v,
                                int* flags, bool* nf) {
  if (row >= d.Q) return idx_at(in.sem, in.sem_i64, v) == (long long)par.sem[row - d.Q];
  if (in.mask_type == GAPRO_PROPOSALS_MASK_U8) return ((const unsigned char*)in.mask)[row * d.V + v] != 0;
  long long col = v;
  if (d.Sv > 0) {
    col = idx_at(in.voxel_spps, in.voxel_spps_i64, v);
    if (col < 0 || col >= d.Sv) {
      *flags |= kFlagVoxelSpp;
      return false;
    }
  }
  const float x = ((const float*)in.mask)[row * (d.Sv > 0 ? d.Sv : d.V) + col];
  *nf = *nf || !isfinite(x);
  return x >= par.logit_thresh;
}

// A wave per run of kPackWords words of one row, kPackUnroll words (independent loads) at a time; one atomic per run
// for the row's popcount.  The loops are uniform over the wave: every lane reaches the ballots.
__global__ __launch_bounds__(kThreads) void k_pr_pack(void* base, PrDims d, PrMaskIn in, PrPar par) {
  PrWs w;
  pr_ws(base, d, &w);
  const int lane = threadIdx.x & 63;
  const long long runs = (d.W + kPackWords - 1) / kPackWords, tasks = d.bit_rows() * runs;
  const long long n_waves = (long long)gridDim.x * (kThreads / 64);
  int flags = 0;
  for (long long t = (long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); t < tasks; t += n_waves) {
    const long long row = t / runs, w0 = (t % runs) * kPackWords, w1 = min(w0 + kPackWords, d.W);
    unsigned pop = 0u;
    bool nf = false;
    for (long long wd = w0; wd < w1; wd += kPackUnroll) {
      bool bit[kPackUnroll];
#pragma unroll
      for (int k = 0; k < kPackUnroll; ++k) {
        const long long v = (wd + k) * 64 + lane;
        bit[k] = wd + k < w1 && v < d.V && mask_bit(d, in, par, row, v, &flags, &nf);
      }
#pragma unroll
      for (int k = 0; k < kPackUnroll; ++k) {
        const unsigned long long word = __ballot(bit[k]);
        if (lane == 0 && wd + k < w1) w.bits[row * d.W + wd + k] = word;
        pop += (unsigned)__popcll(word);
      }
    }
    const unsigned long long any_nf = __ballot(nf);
    if (lane == 0) {
      if (pop) atomicAdd(&w.npoints[row], pop);
      if (any_nf) atomicOr(&w.rowbad[row], 1);
    }
  }
  flags = wave_or(flags);
  if (flags && lane == 0) atomicOr(&w.s->flags, flags);
}

__global__ __launch_bounds__(kThreads) void k_pr_points(void* base, PrDims d, const void* __restrict__ v2p, int v2p_i64,
                                                        const void* __restrict__ spps, int spps_i64) {
  PrWs w;
  pr_ws(base, d, &w);
  int flags = 0;
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < d.N; p += stride) {
    const long long v = idx_at(v2p, v2p_i64, p), s = idx_at(spps, spps_i64, p);
    if (v < 0 || v >= d.V) flags |= kFlagV2p;
    if (s < 0 || s >= d.S) flags |= kFlagSpp;
    else atomicAdd(&w.ntab[s], 1u);
  }
  if (flags) atomicOr(&w.s->flags, flags);
}

// One workgroup: the status, then the candidates with enough voxels, in order.  Thread t owns kMaxTopk / kThreads
// consecutive candidates.
__global__ __launch_bounds__(kThreads) void k_pr_filter(void* base, PrDims d, PrPar par) {
  PrWs w;
  pr_ws(base, d, &w);
  __shared__ int s_cnt[kThreads];
  __shared__ int s_status;
  const int t = threadIdx.x;
  const bool full = d.mode == GAPRO_PROPOSALS_FULL;
  int bad = 0;
  for (int j = t; j < d.P; j += kThreads)
    if (w.rowbad[w.cand_q[j]]) bad = kFlagMask;
  s_cnt[t] = bad;
  __syncthreads();
  if (t == 0) {
    int flags = w.s->flags;
    for (int j = 0; j < kThreads; ++j) flags |= s_cnt[j];
    const int status = (flags & (kFlagScore | kFlagMask)) ? GAPRO_ERR_NOT_FINITE
                       : (flags & (kFlagV2p | kFlagVoxelSpp)) ? GAPRO_ERR_BAD_ARG
                       : (flags & kFlagSpp) ? GAPRO_ERR_SPP_RANGE : GAPRO_OK;
    w.s->flags = flags;
    w.s->status = status;
    s_status = status;
  }
  __syncthreads();
  if (s_status != GAPRO_OK) {  // uniform over the workgroup
    if (t == 0) w.s->n_np = 0;
    return;
  }
  constexpr int kPer = kMaxTopk / kThreads;
  const int j0 = t * kPer;
  bool keep[kPer];
  int c = 0;
  for (int k = 0; k < kPer; ++k) {
    const int j = j0 + k;
    keep[k] = j < d.P && (!full || w.npoints[w.cand_q[j]] >= (unsigned)par.npoint_thresh);
    c += keep[k];
  }
  int total, at = block_sum_before(s_cnt, c, &total);
  for (int k = 0; k < kPer; ++k)
    if (keep[k]) {
      w.surv_q[at] = w.cand_q[j0 + k];
      w.surv_cls[at] = w.cand_cls[j0 + k];
      w.surv_score[at] = w.cand_score[j0 + k];
      ++at;
    }
  if (t == 0) w.s->n_np = total;
}

// ---- stage 3 -----------------------------------------------------------------------------------------------------
// A wave per pair a < b of one class (the only pairs stage 4 reads).
__global__ __launch_bounds__(kThreads) void k_pr_inter(void* base, PrDims d) {
  PrWs w;
  pr_ws(base, d, &w);
  const int n = w.s->n_np, lane = threadIdx.x & 63;
  const long long n_waves = (long long)gridDim.x * (kThreads / 64), tasks = (long long)n * n;
  for (long long t = (long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); t < tasks; t += n_waves) {
    const int a = (int)(t / n), b = (int)(t % n);
    if (a >= b || w.surv_cls[a] != w.surv_cls[b]) continue;  // uniform over the wave
    const int qa = w.surv_q[a], qb = w.surv_q[b];
    const unsigned long long* __restrict__ A = w.bits + (long long)qa * d.W;
    const unsigned long long* __restrict__ B = w.bits + (long long)qb * d.W;
    int inter = 0;
    for (long long i = lane; i < d.W; i += 64) inter += __popcll(A[i] & B[i]);
    inter = wave_sum(inter);
    if (lane == 0) {
      const unsigned uni = w.npoints[qa] + w.npoints[qb] - (unsigned)inter;
      w.iou[(size_t)a * d.P + b] = uni > 0u ? __fdiv_rn((float)inter, (float)uni) : 0.f;
    }
  }
}

// ---- stage 4 -----------------------------------------------------------------------------------------------------
// Matrix NMS, a wave per column j.  First pass: c_j = max_k d_kj.  Second pass: coef_j and the updated score.  The terms
// with d_ij = 0 are 1 / exp(-2 c_i^2) >= 1, and i = 0 has c_0 = 0: the minimum over all i is the minimum of 1 and the
// terms of i < j of j's class.  Maxima and minima do not depend on the order the lanes are folded in.
__global__ __launch_bounds__(kThreads) void k_pr_decay(void* base, PrDims d, int second) {
  PrWs w;
  pr_ws(base, d, &w);
  const int n = w.s->n_np, lane = threadIdx.x & 63;
  const int n_waves = gridDim.x * (kThreads / 64);
  for (int j = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); j < n; j += n_waves) {
    const int cls = w.surv_cls[j];
    if (!second) {
      float c = 0.f;
      for (int k = lane; k < j; k += 64)
        if (w.surv_cls[k] == cls) c = fmaxf(c, w.iou[(size_t)k * d.P + j]);
      c = wave_max(c);
      if (lane == 0) w.comp[j] = c;
    } else {
      double coef = 1.0;
      for (int i = lane; i < j; i += 64)
        if (w.surv_cls[i] == cls) {
          const double dd = (double)w.iou[(size_t)i * d.P + j], cc = (double)w.comp[i];
          coef = fmin(coef, exp(-2.0 * (dd * dd)) / exp(-2.0 * (cc * cc)));
        }
      coef = wave_min(coef);
      if (lane == 0) w.new_score[j] = (float)((double)w.surv_score[j] * coef);
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_pr_nms(void* base, PrDims d, PrPar par) {
  PrWs w;
  pr_ws(base, d, &w);
  __shared__ unsigned long long s_key[kMaxTopk];
  __shared__ int s_cls[kMaxTopk];
  __shared__ float s_new[kMaxTopk];
  __shared__ unsigned char s_supp[kMaxTopk];
  __shared__ int s_keep;
  const int t = threadIdx.x, n = w.s->n_np, P = d.P;
  const int n_sem = d.mode == GAPRO_PROPOSALS_FULL ? d.n_sem : 0;
  for (int r = t; r < n_sem; r += kThreads) {
    w.row_src[r] = (int)d.Q + r;
    w.row_label[r] = par.sem[r] + 1;
    w.row_query[r] = -1;
    w.row_conf[r] = 1.0f;
  }
  for (int j = t; j < kMaxTopk; j += kThreads) {
    s_cls[j] = j < n ? w.surv_cls[j] : -1;
    s_key[j] = 0ull;
    s_supp[j] = 0;
  }
  if (t == 0) s_keep = 0;
  __syncthreads();
  if (par.type_nms == GAPRO_PROPOSALS_NMS_MATRIX) {
    for (int j = t; j < n; j += kThreads) {  // k_pr_decay's
      const float nw = w.new_score[j];
      s_new[j] = nw;
      s_key[j] = sort_key(nw, (unsigned)j);
    }
    sort_desc(s_key);
    int keep = 0;
    if (par.topk >= 0) {
      keep = par.topk < n ? par.topk : n;
    } else {
      for (int j = t; j < n; j += kThreads)
        if (s_new[j] >= par.final_score_thresh) atomicAdd(&s_keep, 1);
      __syncthreads();
      keep = s_keep;
    }
    for (int r = t; r < keep; r += kThreads) {
      const int j = (int)key_index(s_key[r]);
      w.row_src[n_sem + r] = w.surv_q[j];
      w.row_label[n_sem + r] = s_cls[j] + par.label_shift;
      w.row_query[n_sem + r] = w.surv_q[j];
      w.row_conf[n_sem + r] = s_new[j];
    }
    if (t == 0) {
      w.s->n_nms = keep;
      w.s->n_pre = n_sem + keep;
    }
    return;
  }
  // standard: a kept pivot suppresses every later candidate of its class with iou > threshold
  for (int i = 0; i < n; ++i) {
    __syncthreads();
    if (s_supp[i]) continue;  // uniform over the workgroup
    for (int j = i + 1 + t; j < n; j += kThreads)
      if (s_cls[j] == s_cls[i] && w.iou[(size_t)i * P + j] > par.nms_threshold) s_supp[j] = 1;
  }
  __syncthreads();
  if (t == 0) {
    int r = 0;
    for (int j = 0; j < n; ++j) {
      if (s_supp[j]) continue;
      w.row_src[n_sem + r] = w.surv_q[j];
      w.row_label[n_sem + r] = s_cls[j] + par.label_shift;
      w.row_query[n_sem + r] = w.surv_q[j];
      w.row_conf[n_sem + r] = w.surv_score[j];
      ++r;
    }
    w.s->n_nms = r;
    w.s->n_pre = n_sem + r;
  }
}

// ---- stages 5 and 7 ------------------------------------------------------------------------------------------------
__device__ inline int rows_in(const PrWs& w, const PrDims& d) {
  if (w.s->status != GAPRO_OK) return 0;
  return d.mode == GAPRO_PROPOSALS_RLE ? (int)d.Q : w.s->n_pre;
}

// blockIdx.y = row.  `filter` found every v2p_map entry and superpoint id in range, or the status is set.
__global__ __launch_bounds__(kThreads) void k_pr_tally(void* base, PrDims d, const void* __restrict__ v2p, int v2p_i64,
                                                       const void* __restrict__ spps, int spps_i64) {
  PrWs w;
  pr_ws(base, d, &w);
  const int k = blockIdx.y;
  if (k >= rows_in(w, d)) return;
  const unsigned long long* __restrict__ row = w.bits + (long long)w.row_src[k] * d.W;
  unsigned* __restrict__ c = w.ctab + (size_t)k * d.S;
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < d.N; p += stride) {
    const long long v = idx_at(v2p, v2p_i64, p);
    if ((row[v >> 6] >> (v & 63)) & 1ull) atomicAdd(&c[idx_at(spps, spps_i64, p)], 1u);
  }
}

struct PrPointIn {
  const void* spps;
  int spps_i64;
  const unsigned char* masks;  // RLE: u8[Q][N]
};

// m(k, .) of row k as select_runs.h's `bit`: m(k, p) for p in [0, N); 0 outside
__device__ inline auto mask_at(const PrWs& w, const PrDims& d, const PrPointIn& in, int k) {
  return [=](long long p) -> int {
    if (p < 0 || p >= d.N) return 0;
    if (d.mode == GAPRO_PROPOSALS_RLE) return in.masks[(long long)k * d.N + p] != 0;
    const long long s = idx_at(in.spps, in.spps_i64, p);
    return 2ull * w.ctab[(size_t)k * d.S + s] >= (unsigned long long)w.ntab[s];
  };
}

// blockIdx = (chunk, row): the transitions at the positions [chunk * chunk_len, ...) of [0, N] and the row's points.
__global__ __launch_bounds__(kThreads) void k_pr_trans(void* base, PrDims d, PrPointIn in) {
  PrWs w;
  pr_ws(base, d, &w);
  const int k = blockIdx.y;
  if (k >= rows_in(w, d)) return;
  const ChunkTally c = chunk_tally(d.chunk_len, d.N, mask_at(w, d, in, k));
  if (threadIdx.x == 0) {  // the cells are this workgroup's alone
    w.chunk_cnt[(size_t)k * d.nchunks + blockIdx.x] = c.trans;
    w.chunk_ones[(size_t)k * d.nchunks + blockIdx.x] = c.ones;
  }
}

// A wave per row: the chunk counts become the counts before the chunk; the row's transitions and points.
__global__ __launch_bounds__(kThreads) void k_pr_chunks(void* base, PrDims d) {
  PrWs w;
  pr_ws(base, d, &w);
  const int n_pre = rows_in(w, d), lane = threadIdx.x & 63;
  const int n_waves = gridDim.x * (kThreads / 64);
  for (int k = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); k < n_pre; k += n_waves) {
    const unsigned* o = w.chunk_ones + (size_t)k * d.nchunks;
    const unsigned trans = scan_chunks(w.chunk_cnt + (size_t)k * d.nchunks, d.nchunks);
    unsigned ones = 0u;
    for (int j = lane; j < d.nchunks; j += 64) ones += o[j];
    ones = wave_sum(ones);
    if (lane == 0) {
      w.row_trans[k] = trans;
      w.row_ones[k] = ones;
    }
  }
}

// One workgroup.  Thread t owns kRowsPer consecutive rows: which of them stay, and by a prefix over the threads their
// place and the transitions before them; the header.
__global__ __launch_bounds__(kThreads) void k_pr_finish(void* base, PrDims d, PrPar par,
                                                        gapro_proposals_header* __restrict__ header) {
  PrWs w;
  pr_ws(base, d, &w);
  constexpr int kRowsPer = (kMaxRows + kThreads - 1) / kThreads;
  __shared__ unsigned s_rows[kThreads];
  __shared__ unsigned long long s_sum[kThreads];
  const int n_pre = rows_in(w, d), t = threadIdx.x;
  const bool full = d.mode == GAPRO_PROPOSALS_FULL;
  const int n_sem = full ? d.n_sem : 0, k0 = t * kRowsPer;
  bool keep[kRowsPer];
  unsigned trans[kRowsPer], rows = 0u;
  unsigned long long sum = 0ull;
  for (int i = 0; i < kRowsPer; ++i) {
    const int k = k0 + i;
    trans[i] = k < n_pre ? w.row_trans[k] : 0u;
    keep[i] = k < n_pre && !(full && k >= n_sem && w.row_ones[k] < (unsigned)par.npoint_thresh);
    rows += keep[i];
    sum += keep[i] ? trans[i] : 0u;
  }
  unsigned n_rows, r = block_sum_before(s_rows, rows, &n_rows);
  unsigned long long total, off = block_sum_before(s_sum, sum, &total);
  int* counts = (int*)(header + 1);
  for (int i = 0; i < kRowsPer; ++i)
    if (keep[i]) {
      w.final_row[r] = k0 + i;
      w.run_off[r] = (long long)off;
      counts[r] = (int)(trans[i] / 2u);
      off += trans[i];
      ++r;
    }
  if (t != 0) return;
  w.run_off[n_rows] = (long long)total;
  w.s->n_rows = (int)n_rows;
  w.s->total_trans = (long long)total;
  const bool ok = w.s->status == GAPRO_OK;
  header->status = w.s->status;
  header->flags = w.s->flags;
  header->n_rows = (int)n_rows;
  header->n_sem2ins = ok ? n_sem : 0;
  header->total_runs = (long long)(total / 2);
  header->n_candidates = ok && d.mode != GAPRO_PROPOSALS_RLE ? w.s->n_cand : 0;
  header->n_after_npoints = ok ? w.s->n_np : 0;
  header->n_after_nms = ok ? w.s->n_nms : 0;
  header->n_after_refine = ok && full ? (int)n_rows - n_sem : 0;
}

// ---- fill --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_pr_fill_rows(void* base, PrDims d, const unsigned* __restrict__ box_in,
                                                           long long cap_rows, long long cap_runs,
                                                           float* __restrict__ conf, int* __restrict__ label,
                                                           unsigned* __restrict__ box, int* __restrict__ query,
                                                           long long* __restrict__ run_offsets,
                                                           gapro_proposals_header* __restrict__ header) {
  PrWs w;
  pr_ws(base, d, &w);
  if (!fill_ok(*w.s, cap_rows, cap_runs)) {
    if (header && blockIdx.x == 0 && threadIdx.x == 0 && w.s->status == GAPRO_OK) header->status = GAPRO_ERR_WORKSPACE;
    return;
  }
  const int n = w.s->n_rows;
  for (int r = blockIdx.x * kThreads + threadIdx.x; r <= n; r += gridDim.x * kThreads) {
    if (run_offsets) run_offsets[r] = w.run_off[r] / 2;
    if (r == n || d.mode == GAPRO_PROPOSALS_RLE) continue;
    const int k = w.final_row[r], q = w.row_query[k];
    if (conf) conf[r] = w.row_conf[k];
    if (label) label[r] = w.row_label[k];
    if (query) query[r] = q;
    if (box)
      for (int j = 0; j < 6; ++j) box[6 * (size_t)r + j] = q >= 0 && box_in ? box_in[6 * (size_t)q + j] : 0u;
  }
}

// blockIdx = (chunk, output row): the positions of the chunk's transitions, 1-based, in order; the mask bytes.
__global__ __launch_bounds__(kThreads) void k_pr_fill_runs(void* base, PrDims d, PrPointIn in, long long cap_rows,
                                                           long long cap_runs, long long* __restrict__ runs,
                                                           unsigned char* __restrict__ masks) {
  PrWs w;
  pr_ws(base, d, &w);
  if (!fill_ok(*w.s, cap_rows, cap_runs)) return;
  const int r = blockIdx.y;
  if (r >= w.s->n_rows) return;
  const int k = w.final_row[r];
  emit_runs(d.chunk_len, d.N, mask_at(w, d, in, k), w.run_off[r] + w.chunk_cnt[(size_t)k * d.nchunks + blockIdx.x], runs,
            masks ? masks + (long long)r * d.N : nullptr);
}

__global__ __launch_bounds__(kThreads) void k_pr_fill_lengths(void* base, PrDims d, long long cap_rows, long long cap_runs,
                                                              long long* __restrict__ runs) {
  PrWs w;
  pr_ws(base, d, &w);
  if (fill_ok(*w.s, cap_rows, cap_runs)) ends_to_lengths(runs, w.s->total_trans / 2);
}

// ---- host ----------------------------------------------------------------------------------------------------------
bool is_flag(int32_t v) { return v == 0 || v == 1; }

// the sizes both calls and the workspace size agree on; false: refused
bool make_dims(const gapro_proposals_inputs* in, const gapro_proposals_params* p, PrDims* d) {
  if (!in || !p) return false;
  const int mode = p->mode;
  if (mode != GAPRO_PROPOSALS_FULL && mode != GAPRO_PROPOSALS_NMS && mode != GAPRO_PROPOSALS_RLE) return false;
  const long long Q = in->n_queries, V = in->n_voxels, N = in->n_points;
  if (Q < 1) return false;
  *d = PrDims{};
  d->mode = mode;
  d->Q = Q;
  if (mode == GAPRO_PROPOSALS_RLE) {
    if (N < 1 || N > kMaxIndex || Q > kMaxRows) return false;
    d->N = N;
    d->V = 1;
    d->W = 1;
    d->R = (int)Q;
  } else {
    if (V < 1 || V > kMaxIndex) return false;
    if (p->type_nms != GAPRO_PROPOSALS_NMS_MATRIX && p->type_nms != GAPRO_PROPOSALS_NMS_STANDARD) return false;
    if (p->topk < -1) return false;
    d->V = V;
    d->W = (V + 63) / 64;
    if (mode == GAPRO_PROPOSALS_NMS) {
      if (Q > kMaxTopk) return false;
      d->C = 1;
      d->P = (int)Q;
      d->R = (int)Q;
      d->N = 1;
    } else {
      const long long C = p->instance_classes;
      if (N < 1 || N > kMaxIndex || C < 1 || Q * C > kMaxScores || Q > kMaxScores) return false;
      if (p->pre_topk < 1 || p->pre_topk > kMaxTopk || p->npoint_thresh < 1) return false;
      if (p->n_sem2ins < 0 || p->n_sem2ins > kMaxSem || in->n_spps < 1 || in->n_mask_cols < 0) return false;
      d->N = N;
      d->C = (int)C;
      d->S = in->n_spps;
      d->Sv = in->n_mask_cols;
      d->n_sem = p->n_sem2ins;
      d->P = (int)(Q * C < p->pre_topk ? Q * C : p->pre_topk);
      const int kept = p->type_nms == GAPRO_PROPOSALS_NMS_MATRIX && p->topk >= 0 && p->topk < d->P ? p->topk : d->P;
      d->R = kept + d->n_sem > 0 ? kept + d->n_sem : 1;
      if ((long long)d->R * d->S > kMaxIndex) return false;
    }
  }
  chunking(d->N, &d->nchunks, &d->chunk_len);
  if (mode == GAPRO_PROPOSALS_NMS) d->nchunks = 1;  // no runs: N is 1 here
  return true;
}

PrPar make_par(const gapro_proposals_params* p) {
  PrPar par{};
  par.type_nms = p->type_nms;
  par.topk = p->topk;
  par.npoint_thresh = p->npoint_thresh;
  par.label_shift = p->label_shift;
  par.logit_thresh = p->logit_thresh;
  par.final_score_thresh = p->final_score_thresh;
  par.nms_threshold = p->nms_threshold;
  for (int i = 0; i < kMaxSem; ++i) par.sem[i] = p->sem2ins_classes[i];
  return par;
}

// what both calls refuse before anything is launched
int check_args(gapro_ctx* ctx, const char* who, const gapro_proposals_inputs* in, const gapro_proposals_params* p,
               PrDims* d, const void* d_ws, size_t ws_bytes) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  bool ok = make_dims(in, p, d) && d_ws;
  if (ok && d->mode == GAPRO_PROPOSALS_FULL) {
    ok = in->cls_logits && in->conf_logits && in->mask_logits && in->v2p_map && in->spps;
    ok = ok && in->mask_type == GAPRO_PROPOSALS_MASK_F32 && (in->n_mask_cols > 0) == (in->voxel_spps != nullptr);
    ok = ok && (d->n_sem == 0 || in->semantic_preds) && is_flag(in->voxel_spps_i64) && is_flag(in->v2p_i64) &&
         is_flag(in->spps_i64) && is_flag(in->semantic_i64);
    ok = ok && std::isfinite(p->logit_thresh) && std::isfinite(p->final_score_thresh) && std::isfinite(p->nms_threshold);
  } else if (ok && d->mode == GAPRO_PROPOSALS_NMS) {
    ok = in->mask_logits && in->cand_scores && in->cand_classes && in->n_mask_cols == 0 &&
         (in->mask_type == GAPRO_PROPOSALS_MASK_F32 || in->mask_type == GAPRO_PROPOSALS_MASK_U8);
    ok = ok && std::isfinite(p->logit_thresh) && std::isfinite(p->final_score_thresh) && std::isfinite(p->nms_threshold);
  } else if (ok) {
    ok = in->mask_logits && in->mask_type == GAPRO_PROPOSALS_MASK_U8;
  }
  if (!ok) return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: bad argument", who);
  PrWs w;
  if (ws_bytes < align_up(pr_ws(nullptr, *d, &w), 256))
    return gapro_fail(ctx, GAPRO_ERR_WORKSPACE, "%s: workspace too small", who);
  return GAPRO_OK;
}

}  // namespace

extern "C" {

size_t gapro_proposals_workspace_bytes(const gapro_proposals_inputs* in, const gapro_proposals_params* params) {
  PrDims d;
  if (!make_dims(in, params, &d)) return 0;
  PrWs w;
  return align_up(pr_ws(nullptr, d, &w), 256);
}

size_t gapro_proposals_header_bytes(const gapro_proposals_inputs* in, const gapro_proposals_params* params) {
  PrDims d;
  if (!make_dims(in, params, &d)) return 0;
  return GAPRO_PROPOSALS_HEADER_BYTES(d.R);
}

int gapro_proposals_count(gapro_ctx* ctx, void* stream_, const gapro_proposals_inputs* in,
                          const gapro_proposals_params* params, void* d_workspace, size_t workspace_bytes,
                          gapro_proposals_header* d_header, gapro_proposals_header* h_header_pinned) {
  PrDims d;
  const int rc = check_args(ctx, "gapro_proposals_count", in, params, &d, d_workspace, workspace_bytes);
  if (rc != GAPRO_OK) return rc;
  if (!d_header) return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_proposals_count: bad argument");
  hipStream_t stream = (hipStream_t)stream_;
  const PrPar par = make_par(params);
  PrWs w;
  pr_ws(d_workspace, d, &w);
  GAPRO_HIP_CHECK(ctx, hipMemsetAsync(d_workspace, 0, (size_t)(w.zero_end - (char*)d_workspace), stream));
  const dim3 block(kThreads);
  const PrPointIn pin{in->spps, in->spps_i64, (const unsigned char*)in->mask_logits};
  if (d.mode != GAPRO_PROPOSALS_RLE) {
    const PrMaskIn mask_in{in->mask_logits, in->mask_type,      in->voxel_spps,
                           in->voxel_spps_i64, in->semantic_preds, in->semantic_i64};
    if (d.mode == GAPRO_PROPOSALS_FULL)
      hipLaunchKernelGGL(k_pr_score, dim3(grid_for(d.Q, 1, kGridCap)), block, 0, stream, d_workspace, d, in->cls_logits,
                         in->conf_logits);
    hipLaunchKernelGGL(k_pr_select, dim3(1), block, 0, stream, d_workspace, d, in->cand_scores, in->cand_classes);
    hipLaunchKernelGGL(k_pr_pack, dim3(grid_for(d.bit_rows() * ((d.W + kPackWords - 1) / kPackWords) * 64, 1, kGridCap)),
                       block, 0, stream, d_workspace, d, mask_in, par);
    if (d.mode == GAPRO_PROPOSALS_FULL)
      hipLaunchKernelGGL(k_pr_points, dim3(grid_for(d.N, 1, kGridCap)), block, 0, stream, d_workspace, d, in->v2p_map,
                         in->v2p_i64, in->spps, in->spps_i64);
    hipLaunchKernelGGL(k_pr_filter, dim3(1), block, 0, stream, d_workspace, d, par);
    hipLaunchKernelGGL(k_pr_inter, dim3(grid_for((long long)d.P * d.P * 64, 1, kGridCap)), block, 0, stream,
                       d_workspace, d);
    if (par.type_nms == GAPRO_PROPOSALS_NMS_MATRIX)
      for (int second = 0; second < 2; ++second)
        hipLaunchKernelGGL(k_pr_decay, dim3(grid_for((long long)d.P * 64, 1, kGridCap)), block, 0, stream, d_workspace,
                           d, second);
    hipLaunchKernelGGL(k_pr_nms, dim3(1), block, 0, stream, d_workspace, d, par);
    if (d.mode == GAPRO_PROPOSALS_FULL)
      hipLaunchKernelGGL(k_pr_tally, dim3(grid_for(d.N, 1, kTallyGridX), d.R), block, 0, stream, d_workspace, d,
                         in->v2p_map, in->v2p_i64, in->spps, in->spps_i64);
  }
  if (d.mode != GAPRO_PROPOSALS_NMS)
    hipLaunchKernelGGL(k_pr_trans, dim3(d.nchunks, d.R), block, 0, stream, d_workspace, d, pin);
  hipLaunchKernelGGL(k_pr_chunks, dim3(grid_for((long long)d.R * 64, 1, kGridCap)), block, 0, stream, d_workspace, d);
  hipLaunchKernelGGL(k_pr_finish, dim3(1), block, 0, stream, d_workspace, d, par, d_header);
  GAPRO_LAUNCH_CHECK(ctx);
  if (h_header_pinned)
    GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(h_header_pinned, d_header, GAPRO_PROPOSALS_HEADER_BYTES(d.R),
                                        hipMemcpyDeviceToHost, stream));
  return GAPRO_OK;
}

int gapro_proposals_fill(gapro_ctx* ctx, void* stream_, const gapro_proposals_inputs* in,
                         const gapro_proposals_params* params, void* d_workspace, size_t workspace_bytes, float* d_conf,
                         int32_t* d_label_id, float* d_box, int32_t* d_query, int64_t cap_rows, int64_t* d_run_offsets,
                         int64_t* d_runs, int64_t cap_runs, uint8_t* d_masks, gapro_proposals_header* d_header) {
  PrDims d;
  const int rc = check_args(ctx, "gapro_proposals_fill", in, params, &d, d_workspace, workspace_bytes);
  if (rc != GAPRO_OK) return rc;
  const bool runs = d.mode != GAPRO_PROPOSALS_NMS;
  if (cap_rows < 1 || cap_runs < 0 || (runs && (!d_run_offsets || (cap_runs > 0 && !d_runs))) ||
      (!runs && (d_masks || d_runs)) || (d_masks && cap_rows > kMaxRows))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_proposals_fill: bad argument");
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 block(kThreads);
  const long long rows = (long long)cap_rows, cap = (long long)cap_runs;
  const PrPointIn pin{in->spps, in->spps_i64, (const unsigned char*)in->mask_logits};
  hipLaunchKernelGGL(k_pr_fill_rows, dim3(grid_for(d.R + 1, 1, kGridCap)), block, 0, stream, d_workspace, d,
                     (const unsigned*)in->box_preds, rows, cap, d_conf, (int*)d_label_id, (unsigned*)d_box,
                     (int*)d_query, (long long*)d_run_offsets, d_header);
  if (runs && (cap > 0 || d_masks)) {
    const int grid_rows = (int)(rows < d.R ? rows : d.R);
    hipLaunchKernelGGL(k_pr_fill_runs, dim3(d.nchunks, grid_rows), block, 0, stream, d_workspace, d, pin, rows, cap,
                       (long long*)d_runs, d_masks);
    if (cap > 0)
      hipLaunchKernelGGL(k_pr_fill_lengths, dim3(grid_for(cap, 1, kGridCap)), block, 0, stream, d_workspace, d, rows,
                         cap, (long long*)d_runs);
  }
  GAPRO_LAUNCH_CHECK(ctx);
  return GAPRO_OK;
}

}  // extern "C"
