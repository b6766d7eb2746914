// Cost matrices of the consumer's Hungarian matcher (include/gapro_hip.h, "Cost matrices"): the expression chain of ISBNet's
// HungarianMatcher.get_match (isbnet/model/matcher.py:144-199) for every sample of a batch in two launches.
//   check  a wave per instance row of the batch: every mask value is 0 or 1, the class label lies in [0, C); the row's
//          sum_s t (an integer, exact in any order) is kept for the cost kernel
//   cost   a workgroup of four waves per 16-query x 16-instance tile of one sample, the tiles of all samples in one grid
//          through a table built on the host.  The columns are walked in chunks of 16: chunk c belongs to wave c & 3.
//          Lane l holds row l & 15 and the four columns 4 (l >> 4) .. + 3 of the chunk, of the logits (row = query) and
//          of the mask (row = instance); step j of a chunk contracts column j of the four lanes' quadruples, which is one
//          mfma64.h::mma16 for sig . t^T and one for x . t^T.  sig and sp are formed as the logits arrive, and the row
//          sums sum_s sig, sum_s sp are kept by the same lanes.  The four waves' partial tiles and row sums meet in LDS and
//          are added in wave order, thread 16 row + column does the epilogue of its cell.
// The bce term: the reference's BCE(x,1) . t + BCE(x,0) . (1 - t) with BCE(x,0) = sp and BCE(x,1) = sp - x is
// sum_s sp - sum_s x t for t in {0, 1}, exactly.
// Arithmetic: every term in float64 from the float32 inputs, every sum over s in float64 in the order the
// layout above fixes (inside a wave ascending chunks, inside a chunk the MFMA's k order; then lanes 16 apart by a butterfly;
// then waves 0 .. 3), one rounding to float32, then NaN / +-inf -> 100000.  No floating-point atomics, no workgroup waits
// for another.  Tails in Q, I and S are zeros in the operands; a lane outside the matrix forms no address.
// A NaN propagates as in the reference, whose min / max / clamp hand a NaN on: nan_min / nan_max / clamp0 (match_math.h).
#include "common.h"
#include "launch_util.h"
#include "match_math.h"
#include "mfma64.h"
#include "wave_reduce.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace {

using gapro_mfma::d4;
using gapro_mfma::mma16;
using gapro_mfma::unrotate;

constexpr int kThreads = 256, kWaves = 4;
constexpr int kTile = 16;   // queries and instances of a tile
constexpr int kChunk = 16;  // columns a wave takes at a time: four per lane
enum { kFlagClass = 1, kFlagMask = 2 };

struct DevTask {  // one per sample
  const float* x;
  long long ld;
  const float* t;
  const void* cls;
  const float* box;
  int n_inst, n_cols;
  long long cost_off;
  long long row_off;  // instance rows of the samples before this one
};

struct Tile {
  int sample, q0, i0, pad;
};

struct MatchDims {
  int B, Q, C, cls_type;
  long long total_inst;
};

struct MatchWs {
  RefusalHead* s;   // bad: a sample
  DevTask* tasks;   // [B]
  Tile* tiles;      // [tile capacity]
  double* col_sum;  // [total_inst] sum_s t of every instance row
};

__host__ __device__ inline long long tile_capacity(int B, int Q, long long total_inst) {
  return (long long)((Q + kTile - 1) / kTile) * (total_inst / kTile + B);
}

// the table part [0, upload) is what the call uploads; the column sums follow it
__host__ __device__ inline size_t match_ws(void* base, int B, int Q, long long total_inst, MatchWs* w, size_t* upload) {
  char* p = (char*)base;
  w->s = (RefusalHead*)p; p += sizeof(RefusalHead);
  w->tasks = (DevTask*)p; p += (size_t)B * sizeof(DevTask);
  w->tiles = (Tile*)p; p += (size_t)tile_capacity(B, Q, total_inst) * sizeof(Tile);
  if (upload) *upload = (size_t)(p - (char*)base);
  w->col_sum = (double*)p; p += (size_t)total_inst * 8;
  return (size_t)(p - (char*)base);
}

// ---- check ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_match_check(void* base, MatchDims d) {
  MatchWs w;
  match_ws(base, d.B, d.Q, d.total_inst, &w, nullptr);
  const int lane = threadIdx.x & 63;
  const long long g = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);  // uniform over the wave
  if (g >= d.total_inst) return;
  int b = 0;  // the last sample whose rows start at or before g: the one that holds g (an empty one starts where the next does)
  for (int hi = d.B; hi - b > 1;) {
    const int mid = (b + hi) >> 1;
    if (w.tasks[mid].row_off <= g) b = mid;
    else hi = mid;
  }
  const DevTask& t = w.tasks[b];
  const int i = (int)(g - t.row_off), S = t.n_cols;
  const float* __restrict__ row = t.t + (size_t)i * S;
  double sum = 0.0;
  int flags = 0;
  for (int s = lane; s < S; s += 64) {
    const float v = row[s];
    if (!(v == 0.0f || v == 1.0f)) flags |= kFlagMask;
    sum += (double)v;
  }
  sum = wave_sum(sum);  // integers below 2^31: exact in any order
  if (lane == 0) {
    const long long c = cls_at(t.cls, d.cls_type, i);
    if (c < 0 || c >= d.C) flags |= kFlagClass;
    w.col_sum[g] = sum;
  }
  flags = wave_or(flags);
  if (flags != 0 && lane == 0) {
    atomicOr(&w.s->flags, flags);
    atomicMin(&w.s->bad, b);
  }
}

// ---- cost ----------------------------------------------------------------------------------------------------------
// model_utils.py:385-413 for one pair, in float64
__device__ inline double giou_of(const float* __restrict__ p, const float* __restrict__ g) {
  double inter = 1.0, v1 = 1.0, v2 = 1.0, bound = 1.0;
  for (int k = 0; k < 3; ++k) {
    const double a0 = p[k], a1 = p[k + 3], b0 = g[k], b1 = g[k + 3];
    inter *= clamp0(nan_min(a1, b1) - nan_max(a0, b0));
    v1 *= clamp0(a1 - a0);
    v2 *= clamp0(b1 - b0);
    bound *= clamp0(nan_max(a1, b1) - nan_min(a0, b0));
  }
  const double uni = v1 + v2 - inter;
  return inter / (uni + 1e-6) - (bound - uni) / (bound + 1e-6);
}

__global__ __launch_bounds__(kThreads) void k_match_cost(void* base, MatchDims d, const float* __restrict__ cls_logits,
                                                         const float* __restrict__ conf_logits,
                                                         const float* __restrict__ box_preds, gapro_match_weights wt,
                                                         float* __restrict__ cost, int* __restrict__ status) {
  MatchWs w;
  match_ws(base, d.B, d.Q, d.total_inst, &w, nullptr);
  const int flags = w.s->flags;  // written by k_match_check; uniform over the grid
  if (blockIdx.x == 0 && threadIdx.x == 0) write_status(status, *w.s);
  if (flags) return;

  __shared__ double s_acc[kWaves][2][4][64];  // the waves' partial tiles of sig . t^T and x . t^T, MFMA C layout
  __shared__ double s_row[kWaves][2][kTile];  // ... partial sum_s sig and sum_s sp of the tile's queries
  __shared__ double s_soft[2][kTile];         // max and sum exp(z - max) of the queries' class logits

  const Tile tile = w.tiles[blockIdx.x];
  const DevTask& t = w.tasks[tile.sample];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, kk = lane >> 4;
  const int S = t.n_cols, I = t.n_inst;
  const int q = tile.q0 + r, i = tile.i0 + r;
  const bool q_ok = q < d.Q, i_ok = i < I;
  // rows outside the matrix read nothing: the pointers below are only dereferenced under q_ok / i_ok and s < S
  const float* __restrict__ xrow = t.x + (size_t)(q_ok ? q : 0) * (size_t)t.ld;
  const float* __restrict__ trow = t.t + (size_t)(i_ok ? i : 0) * (size_t)S;

  d4 acc_sig = {0.0, 0.0, 0.0, 0.0}, acc_x = {0.0, 0.0, 0.0, 0.0};
  double row_sig = 0.0, row_sp = 0.0;
  const int n_chunks = (S + kChunk - 1) / kChunk;
  for (int c = wave; c < n_chunks; c += kWaves) {  // uniform over the wave
    const int s0 = c * kChunk + 4 * kk;
    float xv[4], tv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool in = s0 + j < S;
      xv[j] = (q_ok && in) ? xrow[s0 + j] : 0.0f;
      tv[j] = (i_ok && in) ? trow[s0 + j] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double x = (double)xv[j];
      double sig = 0.0, sp = 0.0;
      if (q_ok && s0 + j < S) {
        const Sig sg = sigmoid_of(x);
        sig = sg.sig;
        sp = softplus_of(x, sg);  // a NaN logit makes both NaN, and with them its whole row
      }
      row_sig += sig;
      row_sp += sp;
      const double tj = (double)tv[j];
      mma16(sig, tj, acc_sig);
      mma16(x, tj, acc_x);
    }
  }
  // lanes 16 apart hold the same row: every lane ends with the wave's sum of its row
  row_sig += __shfl_xor(row_sig, 16, 64);
  row_sig += __shfl_xor(row_sig, 32, 64);
  row_sp += __shfl_xor(row_sp, 16, 64);
  row_sp += __shfl_xor(row_sp, 32, 64);
  const d4 a = unrotate(acc_sig), bx = unrotate(acc_x);  // register k of lane l: row (l >> 4) + 4 k, column l & 15
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    s_acc[wave][0][k][lane] = a[k];
    s_acc[wave][1][k][lane] = bx[k];
  }
  if (lane < kTile) {
    s_row[wave][0][lane] = row_sig;
    s_row[wave][1][lane] = row_sp;
  }
  if (wave == kWaves - 1 && lane < kTile) {  // the softmax of the tile's queries: one lane per query
    double m = 0.0, den = 1.0;
    if (q_ok) {
      const float* __restrict__ z = cls_logits + ((size_t)tile.sample * d.Q + q) * (size_t)d.C;
      m = (double)z[0];
      for (int c = 1; c < d.C; ++c) m = nan_max(m, (double)z[c]);
      den = 0.0;
      for (int c = 0; c < d.C; ++c) den += exp((double)z[c] - m);
    }
    s_soft[0][lane] = m;
    s_soft[1][lane] = den;
  }
  __syncthreads();

  // thread 16 row + col: cell (row, col) of the tile
  const int row = threadIdx.x >> 4, col = threadIdx.x & 15;
  const int oq = tile.q0 + row, oi = tile.i0 + col;
  if (oq >= d.Q || oi >= I) return;
  const int src_lane = (row & 3) * 16 + col, src_reg = row >> 2;
  double dot_sig = 0.0, dot_x = 0.0, sum_sig = 0.0, sum_sp = 0.0;
#pragma unroll
  for (int v = 0; v < kWaves; ++v) {  // wave order
    dot_sig += s_acc[v][0][src_reg][src_lane];
    dot_x += s_acc[v][1][src_reg][src_lane];
    sum_sig += s_row[v][0][row];
    sum_sp += s_row[v][1][row];
  }
  const double sum_t = w.col_sum[t.row_off + oi];
  const double dice = 1.0 - (2.0 * dot_sig + 1.0) / (sum_sig + sum_t + 1.0);
  const double bce = (sum_sp - dot_x) / (double)S;
  const size_t bq = (size_t)tile.sample * d.Q + oq;
  const long long c = cls_at(t.cls, d.cls_type, oi);  // inside [0, C): k_match_check
  const double cls_cost = -exp((double)cls_logits[bq * (size_t)d.C + (size_t)c] - s_soft[0][row]) / s_soft[1][row];
  const double conf_cost = -(double)conf_logits[bq];
  const double giou_cost = -giou_of(box_preds + bq * 6, t.box + (size_t)oi * 6);
  const double total = wt.w_class * cls_cost + wt.w_dice * dice + wt.w_bce * bce + wt.w_conf * conf_cost +
                       wt.w_giou * giou_cost;
  float out = (float)total;
  if (out != out || fabsf(out) == INFINITY) out = 100000.0f;  // matcher.py:196-197
  cost[t.cost_off + (long long)oq * I + oi] = out;
}

bool dims_ok(int32_t B, int32_t Q, int64_t total_inst, int64_t total_cols) {
  return B >= 1 && B <= GAPRO_SPP_GT_MAX_SAMPLES && Q >= 1 && total_inst >= 1 && total_cols >= 1 &&
         total_inst <= 0x7fffffffLL && tile_capacity(B, Q, total_inst) <= 0x7fffffffLL;
}

}  // namespace

extern "C" {

size_t gapro_match_cost_workspace_bytes(int32_t batch_size, int32_t n_queries, int64_t total_inst, int64_t total_cols) {
  if (!dims_ok(batch_size, n_queries, total_inst, total_cols)) return 0;
  MatchWs w;
  return align_up(match_ws(nullptr, batch_size, n_queries, total_inst, &w, nullptr), 256);
}

int gapro_match_cost(gapro_ctx* ctx, void* stream_, const gapro_match_task* h_tasks, int32_t batch_size,
                     int32_t n_queries, int32_t n_classes, int32_t cls_type, const float* d_cls_logits,
                     const float* d_conf_logits, const float* d_box_preds, const gapro_match_weights* weights,
                     void* d_workspace, size_t workspace_bytes, float* d_cost, int64_t cost_floats, float* h_cost_pinned,
                     int32_t* d_status, int32_t* h_status_pinned) {
  const char* who = "gapro_match_cost";
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  if (!h_tasks || batch_size < 1 || batch_size > GAPRO_SPP_GT_MAX_SAMPLES || n_queries < 1 || n_classes < 1 ||
      (cls_type != GAPRO_LABEL_I32 && cls_type != GAPRO_LABEL_I64) || !d_cls_logits || !d_conf_logits || !d_box_preds ||
      !d_workspace || !d_cost || cost_floats < 1 || !d_status)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: bad argument", who);
  gapro_match_weights wt{0.5, 1.0, 1.0, 0.2, 0.2};  // matcher.py:192
  if (weights) wt = *weights;
  for (double v : {wt.w_class, wt.w_dice, wt.w_bce, wt.w_conf, wt.w_giou})
    if (!std::isfinite(v) || v < 0.0) return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: a weight is negative or not finite", who);

  long long total_inst = 0, total_cols = 0;
  std::vector<std::pair<long long, long long>> spans;  // [first, last) floats of every cost block
  for (int b = 0; b < batch_size; ++b) {
    const gapro_match_task& t = h_tasks[b];
    if (t.n_inst < 0) return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: sample %d: n_inst < 0", who, b);
    if (t.n_inst == 0) continue;
    if (!t.d_mask_logits || !t.d_mask || !t.d_cls || !t.d_box || t.n_cols < 1 || t.ld_logits < t.n_cols)
      return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: sample %d: bad argument", who, b);
    const long long cells = (long long)n_queries * t.n_inst;
    if (t.cost_offset < 0 || t.cost_offset > cost_floats - cells)
      return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: sample %d: its cost block leaves d_cost", who, b);
    spans.emplace_back(t.cost_offset, t.cost_offset + cells);
    total_inst += t.n_inst;
    total_cols += t.n_cols;
  }
  if (spans.empty()) return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: no sample has an instance", who);
  std::sort(spans.begin(), spans.end());
  for (size_t k = 1; k < spans.size(); ++k)
    if (spans[k].first < spans[k - 1].second)
      return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: cost blocks overlap", who);
  if (!dims_ok(batch_size, n_queries, total_inst, total_cols))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: sizes beyond the library's bounds", who);
  if (workspace_bytes < gapro_match_cost_workspace_bytes(batch_size, n_queries, total_inst, total_cols))
    return gapro_fail(ctx, GAPRO_ERR_WORKSPACE, "%s: workspace too small", who);

  // the tables, as the kernels read them
  MatchWs w;
  size_t upload = 0;
  match_ws(nullptr, batch_size, n_queries, total_inst, &w, &upload);
  std::vector<char> table(upload, 0);
  match_ws(table.data(), batch_size, n_queries, total_inst, &w, nullptr);
  w.s->bad = kNoBad;
  long long row_off = 0, n_tiles = 0;
  for (int b = 0; b < batch_size; ++b) {
    const gapro_match_task& t = h_tasks[b];
    w.tasks[b] = DevTask{t.d_mask_logits, (long long)t.ld_logits, t.d_mask, t.d_cls, t.d_box, t.n_inst, t.n_cols,
                         (long long)t.cost_offset, row_off};
    row_off += t.n_inst;
    for (int q0 = 0; q0 < n_queries && t.n_inst > 0; q0 += kTile)
      for (int i0 = 0; i0 < t.n_inst; i0 += kTile) w.tiles[n_tiles++] = Tile{b, q0, i0, 0};
  }
  const MatchDims d{batch_size, n_queries, n_classes, cls_type, total_inst};
  hipStream_t stream = (hipStream_t)stream_;
  GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(d_workspace, table.data(), upload, hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(k_match_check, dim3((unsigned)((total_inst + kWaves - 1) / kWaves)), dim3(kThreads), 0, stream,
                     d_workspace, d);
  hipLaunchKernelGGL(k_match_cost, dim3((unsigned)n_tiles), dim3(kThreads), 0, stream, d_workspace, d, d_cls_logits,
                     d_conf_logits, d_box_preds, wt, d_cost, (int*)d_status);
  GAPRO_LAUNCH_CHECK(ctx);
  if (h_status_pinned)
    GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(h_status_pinned, d_status, GAPRO_MATCH_STATUS_WORDS * sizeof(int32_t),
                                        hipMemcpyDeviceToHost, stream));
  if (h_cost_pinned)
    GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(h_cost_pinned, d_cost, (size_t)cost_floats * sizeof(float),
                                        hipMemcpyDeviceToHost, stream));
  return GAPRO_OK;
}

}  // extern "C"
