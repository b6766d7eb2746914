// SPFormer's criterion over a matched batch, all prediction heads at once (include/gapro_hip.h, "SPFormer's criterion"):
// the loops of Criterion.forward and get_layer_loss (SPFormer/spformer/model/loss.py:415-499, 263-349) in two launches
// forward and one backward.  A task is one (head, sample); the kernels are match_loss.hip's in shape:
//   rows      a workgroup of four waves per (task, query).  Wave 0 forms the query's class term (skipped samples too:
//             the class loss runs over all B Q queries).  A matched query's workgroup walks its logit row against the
//             mask of its matched GT instance (loss_rows.h: the first walk, then for a box of at least min_points
//             members the second one around the mean the first gave) and refuses a mask value that is neither 0 nor
//             1.  Thread 0 writes one record of doubles.
//   finish    one workgroup: wave w takes the tasks w, w + 4, .., its lanes the task's rows and queries l, l + 64, ..;
//             a butterfly gives the task's values and normalisers (n_kept of the score filter among them).  Then thread
//             h takes head h: the samples in their order, the batch-wide class normaliser, the divisions by B.
//   backward  the grid of `rows` for the score and mask-logit gradients, and behind it a workgroup per four queries
//             for the class-logit gradients (a wave per query): every element of every head's gradients, zeros included.
// A head's arithmetic never meets another head's, so a call of seven heads gives the bytes of seven calls of one.
// This file's own: the records and the workspace, the heads, the class target, its weight and its refusal, the mask
// refusal, the score filter, the BCE switch and the normalisers of `finish` with the coefficients the backward forms
// from them, the host's checks and tables.  The walks over a row, its mask-logit gradient and the class term's
// arithmetic are loss_rows.h's.
// Arithmetic: every term in float64 from the float32 inputs, every sum in float64 in the order
// this layout fixes, one rounding to float32.  The level-set membership alone is a float32 comparison, as the
// reference's.  No floating-point atomics (the integer ones carry the refusal), no workgroup waits for another, no
// scratch; a lane outside the row forms no address.
#include "common.h"
#include "launch_util.h"
#include "loss_rows.h"
#include "match_math.h"
#include "wave_reduce.h"

#include <cmath>
#include <cstdint>
#include <vector>

namespace {

constexpr int kThreads = kLossThreads, kWaves = kLossWaves;
constexpr int kMaxF = kLossMaxF;
constexpr int kRowRec = 20, kQueryRec = 4, kTaskRec = 12, kHeadRec = 2;  // doubles
enum { kFlagClass = 1, kFlagMask = 2 };
// a row's record
enum { R_DICE, R_BCE, R_SQ, R_KEEP, R_LS, R_SSIG, R_ST, R_SST, R_IOU, R_A, R_NR, R_SW, R_MU, R_END = R_MU + kMaxF };
static_assert(R_END <= kRowRec, "a row's record");
// a task's record: its four per-sample values, its part of the class sums, the normalisers
enum { T_BCE, T_DICE, T_SCORE, T_LS, T_NUM, T_DEN, T_NKEPT, T_SW, T_N };
enum { L_CLS, L_BCE, L_DICE, L_SCORE, L_LS };  // the order of d_losses

struct DevTask {  // one per (head, sample); n_gt == 0: skipped
  const float* z;      // class logits f32[Q, C]
  const float* score;  // f32[Q]
  const float* x;
  long long ld;
  const float* t;
  const void* cls;
  const float* box;
  int n_gt, n_cols;
  long long col_off;   // the sample's first column in sp_prob, sp_feats and sp_coords
  long long row_off;   // matched rows of the tasks before this one
  long long grad_off;  // floats from the mask-logit gradient's base to this task's f32[Q, n_cols]
};

struct SpfDims {
  int L, B, Q, C, cls_type, F, min_points, flags;
  long long total_gt;
  double w_none;  // non_object_weight
};

struct SpfWs {
  RefusalHead* s;  // bad: a task
  DevTask* tasks;  // [L B]
  int* rows;       // [total_gt] the matched query of every row
  int* cols;       // [total_gt] the matched GT instance of every row
  int* inv;        // [L B Q] the row of every query, or -1
  double* qrec;    // [L B Q][kQueryRec] W (lse - z[tgt]), W, lse
  double* rrec;    // [total_gt][kRowRec]
  double* trec;    // [L B][kTaskRec]
  double* hrec;    // [L][kHeadRec] the class normaliser
};

__host__ __device__ inline size_t spf_ws(void* base, int T, int L, int Q, long long total_gt, SpfWs* w,
                                         size_t* upload) {
  char* p = (char*)base;
  w->s = (RefusalHead*)p; p += sizeof(RefusalHead);
  w->tasks = (DevTask*)p; p += (size_t)T * sizeof(DevTask);
  w->rows = (int*)p; p += (size_t)total_gt * 4;
  w->cols = (int*)p; p += (size_t)total_gt * 4;
  w->inv = (int*)p; p += (size_t)T * Q * 4;
  p = (char*)base + (((size_t)(p - (char*)base) + 7) & ~(size_t)7);
  if (upload) *upload = (size_t)(p - (char*)base);
  w->qrec = (double*)p; p += (size_t)T * Q * kQueryRec * 8;
  w->rrec = (double*)p; p += (size_t)total_gt * kRowRec * 8;
  w->trec = (double*)p; p += (size_t)T * kTaskRec * 8;
  w->hrec = (double*)p; p += (size_t)L * kHeadRec * 8;
  return (size_t)(p - (char*)base);
}

// query q of task t against its matched GT instance gi: the targets are the instance's
__device__ inline RowCols row_cols(const DevTask& t, int F, int q, int gi, const float* __restrict__ prob,
                                   const float* __restrict__ feats, const float* __restrict__ coords) {
  return RowCols{t.x + (size_t)q * (size_t)t.ld, t.t + (size_t)gi * (size_t)t.n_cols, prob + t.col_off,
                 coords + (size_t)t.col_off * 3, feats + (size_t)t.col_off * (size_t)F, t.n_cols, F,
                 box_test(t.box + (size_t)gi * 6)};
}

// ---- rows ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_spf_rows(void* base, SpfDims d, const float* __restrict__ prob,
                                                       const float* __restrict__ feats,
                                                       const float* __restrict__ coords) {
  SpfWs w;
  const int T = d.L * d.B;
  spf_ws(base, T, d.L, d.Q, d.total_gt, &w, nullptr);
  const int task = blockIdx.x / d.Q, q = blockIdx.x % d.Q;
  const DevTask& t = w.tasks[task];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t tq = (size_t)task * d.Q + q;
  const int r = t.n_gt != 0 ? w.inv[tq] : -1;
  const int gi = r >= 0 ? w.cols[t.row_off + r] : 0;  // the matched GT instance

  if (wave == 0) {  // the class term of loss.py:419-428 for this query
    const float* __restrict__ z = t.z + (size_t)q * (size_t)d.C;
    const double lse = wave_lse(z, d.C);
    if (lane == 0) {
      long long c = d.C - 1;
      if (r >= 0) {
        c = cls_at(t.cls, d.cls_type, gi);
        if (c < 0 || c >= d.C - 1) {  // refused: the flag, and an address inside the row
          atomicOr(&w.s->flags, kFlagClass);
          atomicMin(&w.s->bad, task);
          c = d.C - 1;
        }
      }
      const double wt = c == d.C - 1 ? d.w_none : 1.0;
      double* rec = w.qrec + tq * kQueryRec;
      rec[0] = wt * (lse - (double)z[c]);
      rec[1] = wt;
      rec[2] = lse;
      rec[3] = 0.0;
    }
  }
  if (r < 0) return;  // uniform over the workgroup

  const bool weighted = (d.flags & GAPRO_SPF_WEIGHTED_BCE) != 0;
  const RowCols rc = row_cols(t, d.F, q, gi, prob, feats, coords);
  const RowSums u = walk_row(rc, weighted);
  if (u.odd_target) {  // refused: a mask value that is neither 0 nor 1
    atomicOr(&w.s->flags, kFlagMask);
    atomicMin(&w.s->bad, task);
  }
  // uniform: a box of at least min_points members (loss.py:358: min_points_conds, and min_points >= 1)
  const double ls = u.nr >= d.min_points ? walk_members(rc, u.mu, u.nr) : 0.0;
  if (threadIdx.x != 0) return;

  // sums of 0 and 1: integers, exact in float64
  const double uni = (double)u.cnt + u.st - u.inter;
  const double iou = u.inter / (uni + 1e-6);
  const bool keep = 2.0 * u.inter > uni;  // iou > 0.5 of loss.py:458, for every pair of integers
  const double diff = (double)t.score[q] - iou;
  double* rec = w.rrec + (size_t)(t.row_off + r) * kRowRec;
  rec[R_DICE] = 1.0 - (2.0 * u.sst + 1.0) / (u.ssig + u.st + 1.0);
  rec[R_BCE] = u.swb;
  rec[R_SQ] = keep ? diff * diff : 0.0;
  rec[R_KEEP] = keep ? 1.0 : 0.0;
  rec[R_LS] = ls;
  rec[R_SSIG] = u.ssig;
  rec[R_ST] = u.st;
  rec[R_SST] = u.sst;
  rec[R_IOU] = iou;
  rec[R_A] = u.a;
  rec[R_NR] = (double)u.nr;
  rec[R_SW] = u.sw;
#pragma unroll
  for (int f = 0; f < kMaxF; ++f) rec[R_MU + f] = u.mu[f];
}

// the divisor of a sample's BCE sum: as released the plain mean, times sum w / sum w (1, or NaN for a weight sum that is
// 0, infinite or NaN); with GAPRO_SPF_WEIGHTED_BCE the weight sum
__device__ inline double bce_scale(int flags, double sw, double n, double S) {
  return (flags & GAPRO_SPF_WEIGHTED_BCE) ? 1.0 / sw / n : (sw / sw) / (n * S);
}

// ---- finish --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_spf_finish(void* base, SpfDims d, float* __restrict__ losses,
                                                         int* __restrict__ status) {
  SpfWs w;
  const int T = d.L * d.B;
  spf_ws(base, T, d.L, d.Q, d.total_gt, &w, nullptr);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int task = wave; task < T; task += kWaves) {  // uniform over the wave
    const DevTask& t = w.tasks[task];
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, num = 0.0, den = 0.0;
    for (int r = lane; r < t.n_gt; r += 64) {
      const double* rec = w.rrec + (size_t)(t.row_off + r) * kRowRec;
      v[0] += rec[R_BCE];
      v[1] += rec[R_DICE];
      v[2] += rec[R_SQ];
      v[3] += rec[R_LS];
      v[4] += rec[R_KEEP];
    }
    for (int q = lane; q < d.Q; q += 64) {
      const double* rec = w.qrec + ((size_t)task * d.Q + q) * kQueryRec;
      num += rec[0];
      den += rec[1];
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] = wave_sum(v[k]);
    num = wave_sum(num);
    den = wave_sum(den);
    if (lane == 0) {
      double* out = w.trec + (size_t)task * kTaskRec;
      const double n = (double)t.n_gt;
      const double sw = t.n_gt ? w.rrec[(size_t)t.row_off * kRowRec + R_SW] : 0.0;
      out[T_BCE] = t.n_gt ? v[0] * bce_scale(d.flags, sw, n, (double)t.n_cols) : 0.0;
      out[T_DICE] = t.n_gt ? v[1] / n : 0.0;
      out[T_SCORE] = v[4] > 0.0 ? v[2] / v[4] : 0.0;  // no kept row: nothing is added (loss.py:459)
      out[T_LS] = t.n_gt ? v[3] / (n + 1e-4) : 0.0;
      out[T_NUM] = num;
      out[T_DEN] = den;
      out[T_NKEPT] = v[4];
      out[T_SW] = sw;
      out[T_N] = n;
    }
  }
  __syncthreads();
  const int flags = w.s->flags;
  if (threadIdx.x == 0) write_status(status, *w.s);
  const double inv_b = 1.0 / (double)d.B;
  for (int h = threadIdx.x; h < d.L; h += kThreads) {
    double total[4] = {0.0, 0.0, 0.0, 0.0}, num = 0.0, den = 0.0;
    for (int b = 0; b < d.B; ++b) {  // sample order
      const double* rec = w.trec + (size_t)(h * d.B + b) * kTaskRec;
      num += rec[T_NUM];
      den += rec[T_DEN];
      if (w.tasks[h * d.B + b].n_gt == 0) continue;
#pragma unroll
      for (int k = 0; k < 4; ++k) total[k] += rec[T_BCE + k];
    }
    w.hrec[h * kHeadRec] = den;
    const bool main_as_released = h == d.L - 1 && !(d.flags & GAPRO_SPF_DICE_DIV_MAIN);  // loss.py:469-488: no division
    float* out = losses + (size_t)h * GAPRO_SPF_LOSS_N;
    out[L_CLS] = flags ? NAN : (float)(num / den);
    out[L_BCE] = flags ? NAN : (float)(total[0] * inv_b);
    out[L_DICE] = flags ? NAN : (float)(main_as_released ? total[1] : total[1] * inv_b);
    out[L_SCORE] = flags ? NAN : (float)(total[2] * inv_b);
    out[L_LS] = flags ? NAN : (float)(total[3] * inv_b);
  }
}

// the mask-logit gradient of one query of a kept sample (a skipped sample has no block in the gradient)
__device__ inline void spf_mask_grad(const SpfDims& d, const DevTask& t, int q, int h, int r, int gi,
                                     const float* __restrict__ up, const double* __restrict__ trec,
                                     const double* __restrict__ rec, const float* __restrict__ prob,
                                     const float* __restrict__ feats, const float* __restrict__ coords,
                                     float* __restrict__ g_mask) {
  const int S = t.n_cols;
  float* __restrict__ out = g_mask + t.grad_off + (size_t)q * (size_t)S;
  if (r < 0) {  // uniform over the workgroup
    for (int s = threadIdx.x; s < S; s += kThreads) out[s] = 0.0f;
    return;
  }
  const double inv_b = 1.0 / (double)d.B;
  const bool weighted = (d.flags & GAPRO_SPF_WEIGHTED_BCE) != 0;
  const double n = trec[T_N];
  const double den = rec[R_SSIG] + rec[R_ST] + 1.0, numr = 2.0 * rec[R_SST] + 1.0;
  const bool main_as_released = h == d.L - 1 && !(d.flags & GAPRO_SPF_DICE_DIV_MAIN);
  const double k_dice = (double)up[L_DICE] * (main_as_released ? 1.0 : inv_b) / n / (den * den);
  const double kd_num = k_dice * numr, kd_den = 2.0 * k_dice * den;
  const double k_bce = (double)up[L_BCE] * inv_b * bce_scale(d.flags, trec[T_SW], n, (double)S);
  const double nr = rec[R_NR], a = rec[R_A];
  const double k_ls = nr >= (double)d.min_points ? (double)up[L_LS] * inv_b / (n + 1e-4) / nr : 0.0;
  const double rfk = a < 1e-5 ? 2.0 * (1e-5 - a) / 1e-5 : 0.0;  // the clamped mean's own derivative (mask_grad_row)
  double mu[kMaxF];
#pragma unroll
  for (int f = 0; f < kMaxF; ++f) mu[f] = rec[R_MU + f];
  mask_grad_row(row_cols(t, d.F, q, gi, prob, feats, coords), kd_num, kd_den, k_bce, weighted, k_ls, rfk, mu, out);
}

// ---- backward ------------------------------------------------------------------------------------------------------
// the class-logit gradient of one query, by one wave
__device__ inline void spf_label_grad(const SpfDims& d, const SpfWs& w, size_t tq, const float* __restrict__ upstream,
                                      float* __restrict__ g_labels) {
  const int lane = threadIdx.x & 63;
  const int task = (int)(tq / (size_t)d.Q), q = (int)(tq % (size_t)d.Q), h = task / d.B;
  const DevTask& t = w.tasks[task];
  float* __restrict__ out = g_labels + tq * (size_t)d.C;
  if (w.s->flags != 0) {  // a refused call: zeros
    for (int c = lane; c < d.C; c += 64) out[c] = 0.0f;
    return;
  }
  const int r = t.n_gt != 0 ? w.inv[tq] : -1;
  const float* __restrict__ z = t.z + (size_t)q * (size_t)d.C;
  const long long tgt = r >= 0 ? cls_at(t.cls, d.cls_type, w.cols[t.row_off + r]) : d.C - 1;  // in [0, C - 1): no flag
  const double lse = w.qrec[tq * kQueryRec + 2];
  const double k = (double)upstream[(size_t)h * GAPRO_SPF_LOSS_N + L_CLS] * (tgt == d.C - 1 ? d.w_none : 1.0) /
                   w.hrec[h * kHeadRec];
  class_grad_row(z, d.C, lse, tgt, k, lane, 64, out);
}

// workgroups [0, L B Q): the score and mask-logit gradients of one (task, query) each; the workgroups behind them: the
// class-logit gradients, a query per wave
__global__ __launch_bounds__(kThreads) void k_spf_backward(const void* base, SpfDims d, const float* __restrict__ prob,
                                                           const float* __restrict__ feats,
                                                           const float* __restrict__ coords,
                                                           const float* __restrict__ upstream,
                                                           float* __restrict__ g_labels, float* __restrict__ g_scores,
                                                           float* __restrict__ g_mask) {
  SpfWs w;
  const int T = d.L * d.B;
  spf_ws((void*)base, T, d.L, d.Q, d.total_gt, &w, nullptr);
  const size_t n_tq = (size_t)T * d.Q;
  if (blockIdx.x >= n_tq) {  // uniform over the workgroup
    const size_t tq = ((size_t)blockIdx.x - n_tq) * kWaves + (threadIdx.x >> 6);
    if (tq < n_tq) spf_label_grad(d, w, tq, upstream, g_labels);
    return;
  }
  const int task = blockIdx.x / d.Q, q = blockIdx.x % d.Q, h = task / d.B;
  const DevTask& t = w.tasks[task];
  const size_t tq = (size_t)task * d.Q + q;
  const int r = w.s->flags == 0 && t.n_gt != 0 ? w.inv[tq] : -1;  // a refused call: zeros
  const int gi = r >= 0 ? w.cols[t.row_off + r] : 0;
  const float* __restrict__ up = upstream + (size_t)h * GAPRO_SPF_LOSS_N;
  const double* trec = w.trec + (size_t)task * kTaskRec;
  const double* rec = w.rrec + (size_t)(t.row_off + (r >= 0 ? r : 0)) * kRowRec;  // read for r >= 0 only

  if (threadIdx.x == 0 && g_scores) {
    double g = 0.0;
    if (r >= 0 && rec[R_KEEP] != 0.0)
      g = (double)up[L_SCORE] / (double)d.B * 2.0 * ((double)t.score[q] - rec[R_IOU]) / trec[T_NKEPT];
    g_scores[tq] = (float)g;
  }
  if (g_mask && t.n_gt != 0) spf_mask_grad(d, t, q, h, r, gi, up, trec, rec, prob, feats, coords, g_mask);
}

bool dims_ok(int32_t L, int32_t B, int32_t Q, int64_t total_gt) {
  return L >= 1 && B >= 1 && (int64_t)L * B <= GAPRO_SPP_GT_MAX_SAMPLES && Q >= 1 && total_gt >= 0 &&
         total_gt <= (int64_t)L * B * Q && (int64_t)L * B * Q <= 0x60000000LL;  // the backward grid: 5/4 of it
}

int check_common(gapro_ctx* ctx, const char* who, const gapro_spf_loss_dims* dm, const void* a, const void* b,
                 const void* c, const void* ws) {
  if (!dm || !a || !b || !c || !ws) return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: bad argument", who);
  if (dm->n_heads < 1 || dm->batch_size < 1 || (int64_t)dm->n_heads * dm->batch_size > GAPRO_SPP_GT_MAX_SAMPLES ||
      dm->n_queries < 1 || dm->n_classes < 2 || dm->min_points < 1 ||
      (dm->cls_type != GAPRO_LABEL_I32 && dm->cls_type != GAPRO_LABEL_I64) ||
      (dm->flags & ~(GAPRO_SPF_WEIGHTED_BCE | GAPRO_SPF_DICE_DIV_MAIN)))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: bad argument", who);
  if (dm->n_feats < 1 || dm->n_feats > kMaxF)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: n_feats outside [1, %d]", who, kMaxF);
  if (!std::isfinite(dm->non_object_weight))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: non_object_weight is not finite", who);
  return GAPRO_OK;
}

SpfDims dims_of(const gapro_spf_loss_dims& dm, long long total_gt) {
  return SpfDims{dm.n_heads, dm.batch_size, dm.n_queries, dm.n_classes, dm.cls_type, dm.n_feats, dm.min_points,
                 dm.flags, total_gt, dm.non_object_weight};
}

}  // namespace

extern "C" {

size_t gapro_spf_loss_workspace_bytes(int32_t n_heads, int32_t batch_size, int32_t n_queries, int64_t total_gt) {
  if (!dims_ok(n_heads, batch_size, n_queries, total_gt)) return 0;
  SpfWs w;
  return align_up(spf_ws(nullptr, n_heads * batch_size, n_heads, n_queries, total_gt, &w, nullptr), 256);
}

int gapro_spf_loss_forward(gapro_ctx* ctx, void* stream_, const gapro_spf_loss_dims* dims,
                           const gapro_spf_loss_task* h_tasks, const int32_t* h_rows, const int32_t* h_cols,
                           const float* d_sp_prob, const float* d_sp_feats, const float* d_sp_coords, int64_t n_points,
                           void* d_workspace, size_t workspace_bytes, float* d_losses, int32_t* d_status,
                           int32_t* h_status_pinned) {
  const char* who = "gapro_spf_loss_forward";
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  if (!h_tasks || !d_losses || !d_status || n_points < 1)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: bad argument", who);
  if (int rc = check_common(ctx, who, dims, d_sp_prob, d_sp_feats, d_sp_coords, d_workspace)) return rc;
  const int T = dims->n_heads * dims->batch_size, Q = dims->n_queries;

  long long total_gt = 0;
  for (int k = 0; k < T; ++k) {
    const gapro_spf_loss_task& t = h_tasks[k];
    if (!t.d_labels || !t.d_scores) return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: task %d: bad argument", who, k);
    if (t.n_gt < 0 || t.n_gt > Q)
      return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: task %d: n_gt outside [0, n_queries]", who, k);
    if (t.n_gt == 0) continue;
    if (!t.d_mask_logits || !t.d_gt_masks || !t.d_gt_labels || !t.d_gt_boxes || t.n_cols < 1 || t.n_inst < t.n_gt ||
        t.ld_logits < t.n_cols || t.col_offset < 0 || t.col_offset > n_points - t.n_cols || t.row_offset != total_gt)
      return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: task %d: bad argument", who, k);
    total_gt += t.n_gt;
  }
  if (total_gt > 0 && (!h_rows || !h_cols)) return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: bad argument", who);
  if (!dims_ok(dims->n_heads, dims->batch_size, Q, total_gt))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: sizes beyond the library's bounds", who);
  if (workspace_bytes < gapro_spf_loss_workspace_bytes(dims->n_heads, dims->batch_size, Q, total_gt))
    return gapro_fail(ctx, GAPRO_ERR_WORKSPACE, "%s: workspace too small", who);

  // the tables, as the kernels read them: one upload, which also zeroes the status
  SpfWs w;
  size_t upload = 0;
  spf_ws(nullptr, T, dims->n_heads, Q, total_gt, &w, &upload);
  std::vector<char> table(upload, 0);
  spf_ws(table.data(), T, dims->n_heads, Q, total_gt, &w, nullptr);
  w.s->bad = kNoBad;
  for (long long k = 0; k < (long long)T * Q; ++k) w.inv[k] = -1;
  long long grad_off = 0;
  for (int k = 0; k < T; ++k) {
    const gapro_spf_loss_task& t = h_tasks[k];
    if (t.n_gt == 0) {
      w.tasks[k] = DevTask{t.d_labels, t.d_scores, nullptr, 0, nullptr, nullptr, nullptr, 0, 0, 0, total_gt, 0};
      continue;
    }
    w.tasks[k] = DevTask{t.d_labels, t.d_scores, t.d_mask_logits, (long long)t.ld_logits, t.d_gt_masks, t.d_gt_labels,
                         t.d_gt_boxes, t.n_gt, t.n_cols, (long long)t.col_offset, (long long)t.row_offset, grad_off};
    grad_off += (long long)Q * t.n_cols;
    int* inv = w.inv + (size_t)k * Q;
    for (int r = 0; r < t.n_gt; ++r) {
      const int q = h_rows[t.row_offset + r], c = h_cols[t.row_offset + r];
      if (q < 0 || q >= Q)
        return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: task %d: row index %d outside [0, %d)", who, k, q, Q);
      if (c < 0 || c >= t.n_inst)
        return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: task %d: column index %d outside [0, %d)", who, k, c, t.n_inst);
      if (inv[q] >= 0) return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: task %d: row index %d twice", who, k, q);
      inv[q] = r;
      w.rows[t.row_offset + r] = q;
      w.cols[t.row_offset + r] = c;
    }
  }
  const SpfDims d = dims_of(*dims, total_gt);
  hipStream_t stream = (hipStream_t)stream_;
  GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(d_workspace, table.data(), upload, hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(k_spf_rows, dim3((unsigned)(T * Q)), dim3(kThreads), 0, stream, d_workspace, d, d_sp_prob,
                     d_sp_feats, d_sp_coords);
  hipLaunchKernelGGL(k_spf_finish, dim3(1), dim3(kThreads), 0, stream, d_workspace, d, d_losses, (int*)d_status);
  GAPRO_LAUNCH_CHECK(ctx);
  if (h_status_pinned)
    GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(h_status_pinned, d_status, GAPRO_MATCH_STATUS_WORDS * sizeof(int32_t),
                                        hipMemcpyDeviceToHost, stream));
  return GAPRO_OK;
}

int gapro_spf_loss_backward(gapro_ctx* ctx, void* stream_, const gapro_spf_loss_dims* dims, int64_t total_gt,
                            const float* d_sp_prob, const float* d_sp_feats, const float* d_sp_coords,
                            const void* d_workspace, size_t workspace_bytes, const float* d_grad_losses,
                            float* d_grad_labels, float* d_grad_scores, float* d_grad_masks) {
  const char* who = "gapro_spf_loss_backward";
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  if (!d_grad_losses) return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: bad argument", who);
  if (int rc = check_common(ctx, who, dims, d_sp_prob, d_sp_feats, d_sp_coords, d_workspace)) return rc;
  if (!dims_ok(dims->n_heads, dims->batch_size, dims->n_queries, total_gt))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: sizes beyond the library's bounds", who);
  if (workspace_bytes < gapro_spf_loss_workspace_bytes(dims->n_heads, dims->batch_size, dims->n_queries, total_gt))
    return gapro_fail(ctx, GAPRO_ERR_WORKSPACE, "%s: workspace too small", who);
  if (!d_grad_labels && !d_grad_scores && !d_grad_masks) return GAPRO_OK;
  const SpfDims d = dims_of(*dims, total_gt);
  const long long n_tq = (long long)dims->n_heads * dims->batch_size * dims->n_queries;
  const long long label_groups = d_grad_labels ? (n_tq + kWaves - 1) / kWaves : 0;
  hipLaunchKernelGGL(k_spf_backward, dim3((unsigned)(n_tq + label_groups)), dim3(kThreads), 0, (hipStream_t)stream_, d_workspace, d, d_sp_prob, d_sp_feats, d_sp_coords,
                     d_grad_losses, d_grad_labels, d_grad_scores, d_grad_masks);
  GAPRO_LAUNCH_CHECK(ctx);
  return GAPRO_OK;
}

}  // extern "C"
