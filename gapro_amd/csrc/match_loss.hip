// The criterion's seven main losses over a matched batch (include/gapro_hip.h, "Matched losses"): the loop of ISBNet's
// Criterion.single_layer_loss (isbnet/model/criterion.py:235-331) in two launches forward and one backward.
//   rows      a workgroup of four waves per (sample, query), skipped samples' workgroups leave at once.  Wave 0 forms
//             the query's class term.  A matched query's workgroup walks its logit row against the targets of its
//             matched row (loss_rows.h: the first walk, then for a box with a member the second one around the mean
//             the first gave).  Thread 0 forms the row's box, GIoU and confidence terms and writes one record of
//             doubles.
//   finish    one workgroup: wave w takes the samples w, w + 4, .., its lanes the sample's rows and queries l, l + 64,
//             ..; a butterfly gives the sample's seven values and normalisers; thread 0 adds the samples in their order,
//             divides by B and writes f32[7] and the status.
//   backward  the grid of `rows`: reads the records, the normalisers and the upstream f32[7]; per query the class
//             gradient row, the confidence and box gradients and the n_cols mask-logit gradients (zeros for an unmatched
//             query; for a skipped sample only the zeros of its class, confidence and box rows).
// This file's own: the records and the workspace, the class target, its weight and its refusal, the box, GIoU and
// confidence terms, the normalisers of `finish` and the coefficients the backward forms from them, the host's checks
// and tables.  The walks over a row, its mask-logit gradient and the class term's arithmetic are loss_rows.h's.
// Arithmetic: every term in float64 from the float32 inputs, every sum in float64 in the order this
// layout fixes, one rounding to float32.  The level-set membership alone is a float32 comparison, as the reference's.
// No floating-point atomics (the two integer ones carry the refusal), no workgroup waits for another, no scratch; a lane
// outside the row forms no address.  min / max / clamp hand a NaN on, as torch's.
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
constexpr int kRowRec = 24, kQueryRec = 4, kSampleRec = 12;  // doubles
enum { kFlagClass = 1 };
// a row's record
enum { R_DICE, R_BCE_NUM, R_SW, R_IOU_SQ, R_L1, R_GIOU, R_LS, R_SSIG, R_ST, R_SST, R_IOU, R_A, R_NR, R_MU, R_END = R_MU + kMaxF };
static_assert(R_END <= kRowRec, "a row's record");
// a sample's record: the seven losses of the sample, then the normalisers
enum { S_LOSS, S_SW = 7, S_WSUM, S_N };

struct DevTask {  // one per sample; n_gt == 0: skipped
  const float* x;
  long long ld;
  const float* t;
  const void* cls;
  const float* box;
  int n_gt, n_cols;
  long long col_off;   // the sample's first column in prob_labels, levelset_feats and levelset_coords
  long long row_off;   // matched rows of the samples before this one
  long long grad_off;  // floats from the mask-logit gradient's base to this sample's f32[Q, n_cols]
};

struct LossDims {
  int B, Q, C, cls_type, F, pad;
  long long total_gt;
  double l1_scale;  // voxel_scale / 50
};

struct LossWs {
  RefusalHead* s;  // bad: a sample
  DevTask* tasks;  // [B]
  int* rows;       // [total_gt] the matched query of every row
  int* inv;        // [B Q] the row of every query, or -1
  double* qrec;    // [B Q][kQueryRec] W (lse - z[tgt]), W, lse
  double* rrec;    // [total_gt][kRowRec]
  double* srec;    // [B][kSampleRec]
};

__host__ __device__ inline size_t loss_ws(void* base, int B, int Q, long long total_gt, LossWs* w, size_t* upload) {
  char* p = (char*)base;
  w->s = (RefusalHead*)p; p += sizeof(RefusalHead);
  w->tasks = (DevTask*)p; p += (size_t)B * sizeof(DevTask);
  w->rows = (int*)p; p += (size_t)total_gt * 4;
  w->inv = (int*)p; p += (size_t)B * Q * 4;
  p = (char*)base + (((size_t)(p - (char*)base) + 7) & ~(size_t)7);
  if (upload) *upload = (size_t)(p - (char*)base);
  w->qrec = (double*)p; p += (size_t)B * Q * kQueryRec * 8;
  w->rrec = (double*)p; p += (size_t)total_gt * kRowRec * 8;
  w->srec = (double*)p; p += (size_t)B * kSampleRec * 8;
  return (size_t)(p - (char*)base);
}

// query q of sample t against its matched row r: the targets are the row's
__device__ inline RowCols row_cols(const DevTask& t, int F, int q, int r, const float* __restrict__ prob,
                                   const float* __restrict__ feats, const float* __restrict__ coords) {
  return RowCols{t.x + (size_t)q * (size_t)t.ld, t.t + (size_t)r * (size_t)t.n_cols, prob + t.col_off,
                 coords + (size_t)t.col_off * 3, feats + (size_t)t.col_off * (size_t)F, t.n_cols, F,
                 box_test(t.box + (size_t)r * 6)};
}

// ---- rows ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_loss_rows(void* base, LossDims d, const float* __restrict__ cls_logits,
                                                        const float* __restrict__ conf_logits,
                                                        const float* __restrict__ box_preds,
                                                        const float* __restrict__ prob, const float* __restrict__ feats,
                                                        const float* __restrict__ coords,
                                                        const float* __restrict__ empty_weight) {
  LossWs w;
  loss_ws(base, d.B, d.Q, d.total_gt, &w, nullptr);
  const int b = blockIdx.x / d.Q, q = blockIdx.x % d.Q;
  const DevTask& t = w.tasks[b];
  if (t.n_gt == 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t bq = (size_t)b * d.Q + q;
  const int r = w.inv[bq];

  if (wave == 0) {  // the class term of criterion.py:299-310 for this query
    const float* __restrict__ z = cls_logits + bq * (size_t)d.C;
    const double lse = wave_lse(z, d.C);
    if (lane == 0) {
      long long c = d.C - 1;
      if (r >= 0) {
        c = cls_at(t.cls, d.cls_type, r);
        if (c < 0 || c >= d.C) {  // refused: the flag, and an address inside the row
          atomicOr(&w.s->flags, kFlagClass);
          atomicMin(&w.s->bad, b);
          c = d.C - 1;
        }
      }
      const double wt = (double)empty_weight[c];
      double* rec = w.qrec + bq * kQueryRec;
      rec[0] = wt * (lse - (double)z[c]);
      rec[1] = wt;
      rec[2] = lse;
      rec[3] = 0.0;
    }
  }
  if (r < 0) return;  // uniform over the workgroup

  const float* __restrict__ gbox = t.box + (size_t)r * 6;
  const RowCols rc = row_cols(t, d.F, q, r, prob, feats, coords);
  const RowSums u = walk_row(rc, true);  // any float32 target counts as the value it is: odd_target is not read
  const double ls = u.nr > 0 ? walk_members(rc, u.mu, u.nr) : 0.0;  // uniform
  if (threadIdx.x != 0) return;

  const double uni = (double)u.cnt + u.st - u.inter;
  const double iou = u.inter / (uni + 1e-6);
  const double conf = (double)conf_logits[bq];
  const float* __restrict__ pbox = box_preds + bq * 6;
  double l1 = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) l1 += fabs((double)pbox[k] - (double)gbox[k]);
  double* rec = w.rrec + (size_t)(t.row_off + r) * kRowRec;
  rec[R_DICE] = 1.0 - (2.0 * u.sst + 1.0) / (u.ssig + u.st + 1.0);
  rec[R_BCE_NUM] = u.swb;
  rec[R_SW] = u.sw;
  rec[R_IOU_SQ] = (conf - iou) * (conf - iou);
  rec[R_L1] = l1;
  rec[R_GIOU] = giou_loss_of(pbox, gbox, nullptr);
  rec[R_LS] = ls;
  rec[R_SSIG] = u.ssig;
  rec[R_ST] = u.st;
  rec[R_SST] = u.sst;
  rec[R_IOU] = iou;
  rec[R_A] = u.a;
  rec[R_NR] = (double)u.nr;
#pragma unroll
  for (int f = 0; f < kMaxF; ++f) rec[R_MU + f] = u.mu[f];
}

// ---- finish --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_loss_finish(void* base, LossDims d, float* __restrict__ losses,
                                                          int* __restrict__ status) {
  LossWs w;
  loss_ws(base, d.B, d.Q, d.total_gt, &w, nullptr);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int b = wave; b < d.B; b += kWaves) {  // uniform over the wave
    const DevTask& t = w.tasks[b];
    double* out = w.srec + (size_t)b * kSampleRec;
    if (t.n_gt == 0) continue;
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, num = 0.0, den = 0.0;
    for (int r = lane; r < t.n_gt; r += 64) {
      const double* rec = w.rrec + (size_t)(t.row_off + r) * kRowRec;
      v[0] += rec[R_DICE];
      v[1] += rec[R_BCE_NUM];
      v[2] += rec[R_IOU_SQ];
      v[3] += rec[R_L1];
      v[4] += rec[R_GIOU];
      v[5] += rec[R_LS];
    }
    for (int q = lane; q < d.Q; q += 64) {
      const double* rec = w.qrec + ((size_t)b * d.Q + q) * kQueryRec;
      num += rec[0];
      den += rec[1];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = wave_sum(v[k]);
    num = wave_sum(num);
    den = wave_sum(den);
    if (lane == 0) {
      const double n = (double)t.n_gt, sw = w.rrec[(size_t)t.row_off * kRowRec + R_SW];
      out[S_LOSS + 0] = v[0] / (n + 1e-6);
      out[S_LOSS + 1] = v[1] / sw / (n + 1e-6);  // a zero weight sum: NaN, as the reference
      out[S_LOSS + 2] = num / den;
      out[S_LOSS + 3] = v[2] / n;
      out[S_LOSS + 4] = d.l1_scale * v[3] / n;
      out[S_LOSS + 5] = v[4] / n;
      out[S_LOSS + 6] = v[5] / (n + 1e-4);
      out[S_SW] = sw;
      out[S_WSUM] = den;
      out[S_N] = n;
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const int flags = w.s->flags;
  write_status(status, *w.s);
  double total[GAPRO_MATCH_LOSS_N] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int b = 0; b < d.B; ++b) {  // sample order
    if (w.tasks[b].n_gt == 0) continue;
    const double* rec = w.srec + (size_t)b * kSampleRec;
#pragma unroll
    for (int k = 0; k < GAPRO_MATCH_LOSS_N; ++k) total[k] += rec[S_LOSS + k];
  }
#pragma unroll
  for (int k = 0; k < GAPRO_MATCH_LOSS_N; ++k) losses[k] = flags ? NAN : (float)(total[k] / (double)d.B);
}

// ---- backward ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_loss_backward(const void* base, LossDims d,
                                                            const float* __restrict__ cls_logits,
                                                            const float* __restrict__ conf_logits,
                                                            const float* __restrict__ box_preds,
                                                            const float* __restrict__ prob,
                                                            const float* __restrict__ feats,
                                                            const float* __restrict__ coords,
                                                            const float* __restrict__ empty_weight,
                                                            const float* __restrict__ upstream,
                                                            float* __restrict__ g_cls, float* __restrict__ g_mask,
                                                            float* __restrict__ g_conf, float* __restrict__ g_box) {
  LossWs w;
  loss_ws((void*)base, d.B, d.Q, d.total_gt, &w, nullptr);
  const int b = blockIdx.x / d.Q, q = blockIdx.x % d.Q;
  const DevTask& t = w.tasks[b];
  const size_t bq = (size_t)b * d.Q + q;
  const bool live = t.n_gt != 0 && w.s->flags == 0;  // a skipped sample, a refused call: zeros
  const int r = live ? w.inv[bq] : -1;
  const double inv_b = 1.0 / (double)d.B;
  // the upstream gradients, in the order of the losses: dice, bce, cls, iou, box, giou, levelset
  const double* srec = w.srec + (size_t)b * kSampleRec;

  if (g_cls) {
    float* __restrict__ out = g_cls + bq * (size_t)d.C;
    if (!live) {
      for (int c = threadIdx.x; c < d.C; c += kThreads) out[c] = 0.0f;
    } else {
      const float* __restrict__ z = cls_logits + bq * (size_t)d.C;
      const long long tgt = r >= 0 ? cls_at(t.cls, d.cls_type, r) : d.C - 1;  // inside [0, C): no flag
      const double lse = w.qrec[bq * kQueryRec + 2];
      const double k = (double)upstream[2] * inv_b * (double)empty_weight[tgt] / srec[S_WSUM];
      class_grad_row(z, d.C, lse, tgt, k, threadIdx.x, kThreads, out);
    }
  }
  if (r < 0) {  // uniform over the workgroup
    if (threadIdx.x == 0 && g_conf) g_conf[bq] = 0.0f;
    if (threadIdx.x < 6 && g_box) g_box[bq * 6 + threadIdx.x] = 0.0f;
    if (t.n_gt != 0 && g_mask) {
      float* __restrict__ out = g_mask + t.grad_off + (size_t)q * (size_t)t.n_cols;
      for (int s = threadIdx.x; s < t.n_cols; s += kThreads) out[s] = 0.0f;
    }
    return;
  }

  const double* rec = w.rrec + (size_t)(t.row_off + r) * kRowRec;
  const double n = srec[S_N];
  const float* __restrict__ gbox = t.box + (size_t)r * 6;
  if (threadIdx.x == 0) {
    if (g_conf) g_conf[bq] = (float)((double)upstream[3] * inv_b * 2.0 * ((double)conf_logits[bq] - rec[R_IOU]) / n);
    if (g_box) {
      const float* __restrict__ pbox = box_preds + bq * 6;
      double gg[6];
      giou_loss_of(pbox, gbox, gg);
      const double k_l1 = (double)upstream[4] * inv_b * d.l1_scale / n, k_gi = (double)upstream[5] * inv_b / n;
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const double diff = (double)pbox[k] - (double)gbox[k];
        const double sgn = diff > 0.0 ? 1.0 : (diff < 0.0 ? -1.0 : diff);  // sign(0) = 0; a NaN stays
        g_box[bq * 6 + k] = (float)(k_l1 * sgn + k_gi * gg[k]);
      }
    }
  }
  if (!g_mask) return;

  const double den = rec[R_SSIG] + rec[R_ST] + 1.0, numr = 2.0 * rec[R_SST] + 1.0;
  const double k_dice = (double)upstream[0] * inv_b / (n + 1e-6) / (den * den);
  const double k_bce = (double)upstream[1] * inv_b / (srec[S_SW] * (n + 1e-6));
  const double nr = rec[R_NR], a = rec[R_A];
  const double k_ls = nr > 0.0 ? (double)upstream[6] * inv_b / (n + 1e-4) / nr : 0.0;
  const double rfk = a < 1e-5 ? 2.0 * (1e-5 - a) / 1e-5 : 0.0;  // the clamped mean's own derivative (mask_grad_row)
  double mu[kMaxF];
#pragma unroll
  for (int f = 0; f < kMaxF; ++f) mu[f] = rec[R_MU + f];
  mask_grad_row(row_cols(t, d.F, q, r, prob, feats, coords), k_dice * numr, 2.0 * k_dice * den, k_bce, true, k_ls, rfk,
                mu, g_mask + t.grad_off + (size_t)q * (size_t)t.n_cols);
}

bool dims_ok(int32_t B, int32_t Q, int64_t total_gt) {
  return B >= 1 && B <= GAPRO_SPP_GT_MAX_SAMPLES && Q >= 1 && total_gt >= 1 && total_gt <= (int64_t)B * Q &&
         (int64_t)B * Q <= 0x7fffffffLL;
}

int check_common(gapro_ctx* ctx, const char* who, int32_t B, int32_t Q, int32_t C, int32_t cls_type, int32_t F,
                 const void* a, const void* b, const void* c, const void* d, const void* e, const void* f,
                 const void* g, const void* ws) {
  if (B < 1 || B > GAPRO_SPP_GT_MAX_SAMPLES || Q < 1 || C < 1 || (int64_t)B * Q > 0x7fffffffLL ||
      (cls_type != GAPRO_LABEL_I32 && cls_type != GAPRO_LABEL_I64) || !a || !b || !c || !d || !e || !f || !g || !ws)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: bad argument", who);
  if (F < 1 || F > kMaxF) return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: n_feats outside [1, %d]", who, kMaxF);
  return GAPRO_OK;
}

}  // namespace

extern "C" {

size_t gapro_match_loss_workspace_bytes(int32_t batch_size, int32_t n_queries, int64_t total_gt) {
  if (!dims_ok(batch_size, n_queries, total_gt)) return 0;
  LossWs w;
  return align_up(loss_ws(nullptr, batch_size, n_queries, total_gt, &w, nullptr), 256);
}

int gapro_match_loss_forward(gapro_ctx* ctx, void* stream_, const gapro_match_loss_task* h_tasks,
                             const int32_t* h_rows, int32_t batch_size, int32_t n_queries, int32_t n_classes,
                             int32_t cls_type, int32_t n_feats, const float* d_cls_logits, const float* d_conf_logits,
                             const float* d_box_preds, const float* d_prob_labels, const float* d_levelset_feats,
                             const float* d_levelset_coords, int64_t n_points, const float* d_empty_weight,
                             double voxel_scale, void* d_workspace, size_t workspace_bytes, float* d_losses,
                             int32_t* d_status, int32_t* h_status_pinned) {
  const char* who = "gapro_match_loss_forward";
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  if (!h_tasks || !h_rows || !d_losses || !d_status || n_points < 1)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: bad argument", who);
  if (int rc = check_common(ctx, who, batch_size, n_queries, n_classes, cls_type, n_feats, d_cls_logits, d_conf_logits,
                            d_box_preds, d_prob_labels, d_levelset_feats, d_levelset_coords, d_empty_weight,
                            d_workspace))
    return rc;
  if (!std::isfinite(voxel_scale)) return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: voxel_scale is not finite", who);

  long long total_gt = 0;
  for (int b = 0; b < batch_size; ++b) {
    const gapro_match_loss_task& t = h_tasks[b];
    if (t.n_gt < 0 || t.n_gt > n_queries)
      return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: sample %d: n_gt outside [0, n_queries]", who, b);
    if (t.n_gt == 0) continue;
    if (!t.d_mask_logits || !t.d_inst_labels || !t.d_cls_labels || !t.d_box_labels || t.n_cols < 1 ||
        t.ld_logits < t.n_cols || t.col_offset < 0 || t.col_offset > n_points - t.n_cols || t.row_offset != total_gt)
      return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: sample %d: bad argument", who, b);
    total_gt += t.n_gt;
  }
  if (total_gt == 0) return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: every sample is skipped", who);
  if (!dims_ok(batch_size, n_queries, total_gt))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: sizes beyond the library's bounds", who);
  if (workspace_bytes < gapro_match_loss_workspace_bytes(batch_size, n_queries, total_gt))
    return gapro_fail(ctx, GAPRO_ERR_WORKSPACE, "%s: workspace too small", who);

  // the tables, as the kernels read them: one upload, which also zeroes the status
  LossWs w;
  size_t upload = 0;
  loss_ws(nullptr, batch_size, n_queries, total_gt, &w, &upload);
  std::vector<char> table(upload, 0);
  loss_ws(table.data(), batch_size, n_queries, total_gt, &w, nullptr);
  w.s->bad = kNoBad;
  for (long long k = 0; k < (long long)batch_size * n_queries; ++k) w.inv[k] = -1;
  long long grad_off = 0;
  for (int b = 0; b < batch_size; ++b) {
    const gapro_match_loss_task& t = h_tasks[b];
    if (t.n_gt == 0) {
      w.tasks[b] = DevTask{nullptr, 0, nullptr, nullptr, nullptr, 0, 0, 0, 0, 0};
      continue;
    }
    w.tasks[b] = DevTask{t.d_mask_logits, (long long)t.ld_logits, t.d_inst_labels, t.d_cls_labels, t.d_box_labels,
                         t.n_gt, t.n_cols, (long long)t.col_offset, (long long)t.row_offset, grad_off};
    grad_off += (long long)n_queries * t.n_cols;
    int* inv = w.inv + (size_t)b * n_queries;
    for (int r = 0; r < t.n_gt; ++r) {
      const int q = h_rows[t.row_offset + r];
      if (q < 0 || q >= n_queries) return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: sample %d: row index %d outside [0, %d)", who, b, q, n_queries);
      if (inv[q] >= 0) return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: sample %d: row index %d twice", who, b, q);
      inv[q] = r;
      w.rows[t.row_offset + r] = q;
    }
  }
  const LossDims d{batch_size, n_queries, n_classes, cls_type, n_feats, 0, total_gt, voxel_scale / 50.0};
  hipStream_t stream = (hipStream_t)stream_;
  GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(d_workspace, table.data(), upload, hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(k_loss_rows, dim3((unsigned)(batch_size * n_queries)), dim3(kThreads), 0, stream, d_workspace, d,
                     d_cls_logits, d_conf_logits, d_box_preds, d_prob_labels, d_levelset_feats, d_levelset_coords,
                     d_empty_weight);
  hipLaunchKernelGGL(k_loss_finish, dim3(1), dim3(kThreads), 0, stream, d_workspace, d, d_losses, (int*)d_status);
  GAPRO_LAUNCH_CHECK(ctx);
  if (h_status_pinned)
    GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(h_status_pinned, d_status, GAPRO_MATCH_STATUS_WORDS * sizeof(int32_t),
                                        hipMemcpyDeviceToHost, stream));
  return GAPRO_OK;
}

int gapro_match_loss_backward(gapro_ctx* ctx, void* stream_, int32_t batch_size, int32_t n_queries, int32_t n_classes,
                              int32_t cls_type, int32_t n_feats, int64_t total_gt, const float* d_cls_logits,
                              const float* d_conf_logits, const float* d_box_preds, const float* d_prob_labels,
                              const float* d_levelset_feats, const float* d_levelset_coords,
                              const float* d_empty_weight, double voxel_scale, const void* d_workspace,
                              size_t workspace_bytes, const float* d_grad_losses, float* d_grad_cls_logits,
                              float* d_grad_mask_logits, float* d_grad_conf_logits, float* d_grad_box_preds) {
  const char* who = "gapro_match_loss_backward";
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  if (!d_grad_losses) return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: bad argument", who);
  if (int rc = check_common(ctx, who, batch_size, n_queries, n_classes, cls_type, n_feats, d_cls_logits, d_conf_logits,
                            d_box_preds, d_prob_labels, d_levelset_feats, d_levelset_coords, d_empty_weight,
                            d_workspace))
    return rc;
  if (!std::isfinite(voxel_scale)) return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: voxel_scale is not finite", who);
  if (!dims_ok(batch_size, n_queries, total_gt))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: sizes beyond the library's bounds", who);
  if (workspace_bytes < gapro_match_loss_workspace_bytes(batch_size, n_queries, total_gt))
    return gapro_fail(ctx, GAPRO_ERR_WORKSPACE, "%s: workspace too small", who);
  if (!d_grad_cls_logits && !d_grad_mask_logits && !d_grad_conf_logits && !d_grad_box_preds) return GAPRO_OK;
  const LossDims d{batch_size, n_queries, n_classes, cls_type, n_feats, 0, total_gt, voxel_scale / 50.0};
  hipLaunchKernelGGL(k_loss_backward, dim3((unsigned)(batch_size * n_queries)), dim3(kThreads), 0, (hipStream_t)stream_,
                     d_workspace, d, d_cls_logits, d_conf_logits, d_box_preds, d_prob_labels, d_levelset_feats,
                     d_levelset_coords, d_empty_weight, d_grad_losses, d_grad_cls_logits, d_grad_mask_logits,
                     d_grad_conf_logits, d_grad_box_preds);
  GAPRO_LAUNCH_CHECK(ctx);
  return GAPRO_OK;
}

}  // extern "C"
