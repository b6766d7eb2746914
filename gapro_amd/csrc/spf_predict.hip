// SPFormer's inference post-processing (include/gapro_hip.h, "SPFormer's predicted instances"): SPFormer.predict_by_feat
// (SPFormer/spformer/model/spformer.py:180-242) with the rle_encode_gpu_batch it calls, without the [K, N] expansion of
// the superpoint masks and without a host round trip per instance.  Nothing of size K x N exists but the runs (and the
// masks, on request): points, boxes and runs of a row come from its superpoint bits and three tables per superpoint.
// gapro_spf_predict_count:
//   score    a thread per query: softmax and product in float64, rounded once
//   select   one workgroup: radix select of the K largest (score, lowest flat index first), sorted
//   points   one pass over the points: n(j), lo(j), hi(j) by integer atomics; the ranges of superpoints and coords_float
//   rows     a workgroup per candidate: the ballot of `logit > 0` over 64 superpoints is the word; cnt, the float64 sum
//            of the sigmoids in a fixed order, conf; npoints and the box from the tables
//   filter   one workgroup: the status, the rows with conf > score_thr and then npoints > npoint_thr, sorted by conf
//   trans    a workgroup per (row, chunk of points): transitions of m(k, .) in the chunk, no atomics
//   chunks   a wave per row: the transitions before each chunk, the row's transitions
//   finish   one workgroup: the run offsets by a prefix, the header
// gapro_spf_predict_fill:
//   rows     conf, label, box, query, run offsets
//   runs     the positions of the transitions in order (and the masks); then `lengths` turns every second into a length
// Integer atomics only, so every result is the same bits for every grid and every run.  The kernel boundaries on the
// stream are the only ordering.  A refusal is a status word written by `filter`: every later kernel returns at once.
// The softmax, the select / sort and the chunked run lengths are select_runs.h's, shared with proposals.hip; this file
// supplies its point bit (`mask_at`: the superpoint bit of the point) and its row indexing: the chunk cells of a row
// belong to output row r, and `row_cand[r]` only finds the row's bits.
#include "common.h"
#include "label_types.h"
#include "launch_util.h"
#include "select_runs.h"
#include "wave_reduce.h"

#include <cmath>
#include <cstdint>

namespace {

enum { kFlagScore = 1, kFlagMask = 2, kFlagCoords = 4, kFlagSpp = 8 };

struct SpScalars {  // the first 64 bytes of the workspace
  int flags;
  int status;   // set by k_sp_filter
  int n_cand;   // after `select`
  int n_score;  // rows with conf > score_thr
  int n_rows;   // rows out
  int reserved;
  long long total_trans;  // 2 * total_runs
  long long pad[4];
};
static_assert(sizeof(SpScalars) == 64, "SpScalars is the first 64 bytes of the workspace");

struct SpDims {
  long long Q, S, N;    // queries, superpoints (columns of the mask logits), points
  long long W;          // 64-bit words of a row of superpoint bits
  long long chunk_len;  // points of a chunk of `trans` / `runs`
  int C, K, nchunks;    // classes, candidates, chunks
};

struct SpWs {
  SpScalars* s;
  // cleared by the count's first memset, up to `zero_end`
  unsigned* ntab;  // [S] points of a superpoint
  unsigned* hi;    // [S][3] the largest coordinate of a superpoint, as order_bits
  char* zero_end;
  unsigned* lo;    // [S][3] the smallest; set to all ones by the second memset, up to `ones_end`
  char* ones_end;
  float* score;    // [Q * C]
  int* cand_q;     // [K] query, class, conf, points and box of the candidates, in stage-1 order
  int* cand_cls;
  float* cand_conf;
  int* cand_bad;   // a non-finite mask logit was read for the candidate
  long long* cand_np;
  unsigned* cand_box;        // [K][6] as order_bits
  int* row_cand;             // [K] the candidate k of output row r
  unsigned* chunk_cnt;       // [K][nchunks] transitions of a chunk; after `chunks` the transitions before it
  unsigned* row_trans;       // [K] transitions of a row
  long long* run_off;        // [K + 1] transitions before output row r
  unsigned long long* bits;  // [K][W]
};

__host__ __device__ inline size_t sp_ws(void* base, const SpDims& d, SpWs* w) {
  char* p = (char*)base;
  auto take = [&](size_t bytes) {
    char* q = p;
    p += (bytes + 15) & ~(size_t)15;
    return q;
  };
  const size_t K = (size_t)d.K, S = (size_t)d.S;
  w->s = (SpScalars*)take(sizeof(SpScalars));
  w->ntab = (unsigned*)take(S * 4);
  w->hi = (unsigned*)take(S * 12);
  w->zero_end = p;
  w->lo = (unsigned*)take(S * 12);
  w->ones_end = p;
  w->score = (float*)take((size_t)(d.Q * d.C) * 4);
  w->cand_q = (int*)take(K * 4);
  w->cand_cls = (int*)take(K * 4);
  w->cand_conf = (float*)take(K * 4);
  w->cand_bad = (int*)take(K * 4);
  w->cand_np = (long long*)take(K * 8);
  w->cand_box = (unsigned*)take(K * 24);
  w->row_cand = (int*)take(K * 4);
  w->chunk_cnt = (unsigned*)take(K * (size_t)d.nchunks * 4);
  w->row_trans = (unsigned*)take(K * 4);
  w->run_off = (long long*)take((K + 1) * 8);
  w->bits = (unsigned long long*)take(K * (size_t)d.W * 8);
  return (size_t)(p - (char*)base);
}

// ---- step 1 ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_sp_score(void* base, SpDims d, const float* __restrict__ labels,
                                                       const float* __restrict__ pred_scores) {
  SpWs w;
  sp_ws(base, d, &w);
  const int C = d.C;
  int bad = 0;
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long q = (long long)blockIdx.x * kThreads + threadIdx.x; q < d.Q; q += stride) {
    const float* row = labels + q * (C + 1);
    const RowSoftmax sm = row_softmax(row, C);
    if (!(sm.ok && isfinite(pred_scores[q]))) {
      bad = kFlagScore;
      for (int c = 0; c < C; ++c) w.score[q * C + c] = 0.f;
      continue;
    }
    const double ps = (double)pred_scores[q];
    for (int c = 0; c < C; ++c) w.score[q * C + c] = (float)sm.times(row[c], ps) + 0.f;  // + 0: never -0.0
  }
  if (bad) atomicOr(&w.s->flags, bad);
}

// One workgroup: the d.K largest (score, lowest index first), sorted, as candidates.
__global__ __launch_bounds__(kThreads) void k_sp_select(void* base, SpDims d) {
  SpWs w;
  sp_ws(base, d, &w);
  __shared__ unsigned long long s_key[kMaxTopk];
  const int t = threadIdx.x;
  select_topk(w.score, (unsigned)(d.Q * d.C), d.K, s_key);
  for (int j = t; j < d.K; j += kThreads) {
    const unsigned i = key_index(s_key[j]);
    w.cand_q[j] = (int)(i / (unsigned)d.C);
    w.cand_cls[j] = (int)(i % (unsigned)d.C);
  }
  if (t == 0) w.s->n_cand = d.K;
}

// ---- step 3 ------------------------------------------------------------------------------------------------------
// An extremum is an atomic only where the value read is not already beyond the point's: most points of a superpoint are
// inside its box, and a stale read costs an atomic too many, never one too few (the cells only move one way).
__global__ __launch_bounds__(kThreads) void k_sp_points(void* base, SpDims d, const void* __restrict__ spps,
                                                        int spps_i64, const float* __restrict__ coords) {
  SpWs w;
  sp_ws(base, d, &w);
  int flags = 0;
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < d.N; p += stride) {
    const long long s = idx_at(spps, spps_i64, p);
    const float x[3] = {coords[3 * p], coords[3 * p + 1], coords[3 * p + 2]};
    if (!(isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]))) flags |= kFlagCoords;
    if (s < 0 || s >= d.S) {
      flags |= kFlagSpp;
      continue;
    }
    atomicAdd(&w.ntab[s], 1u);
    for (int a = 0; a < 3; ++a) {
      const unsigned u = order_bits(x[a]);
      if (u < w.lo[3 * s + a]) atomicMin(&w.lo[3 * s + a], u);
      if (u > w.hi[3 * s + a]) atomicMax(&w.hi[3 * s + a], u);
    }
  }
  flags = wave_or(flags);
  if (flags && (threadIdx.x & 63) == 0) atomicOr(&w.s->flags, flags);
}

// ---- steps 2 and 4 -------------------------------------------------------------------------------------------------
// A workgroup per candidate; wave v packs the words v, v + 4, ...  The float64 sum of a row is fixed: a lane adds its
// words in ascending order, the lanes fold by the xor butterfly, thread 0 adds the waves in ascending order.  The loops
// are uniform over the wave: every lane reaches the ballots.
__global__ __launch_bounds__(kThreads) void k_sp_rows(void* base, SpDims d, const float* __restrict__ labels,
                                                      const float* __restrict__ pred_scores,
                                                      const float* __restrict__ masks) {
  SpWs w;
  sp_ws(base, d, &w);
  __shared__ double s_sum[kWaves];
  __shared__ unsigned long long s_cnt[kWaves], s_np[kWaves];
  __shared__ unsigned s_box[kWaves][6];
  __shared__ int s_nf[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k = blockIdx.x; k < d.K; k += gridDim.x) {  // uniform over the workgroup
    const int q = w.cand_q[k];
    const float* __restrict__ row = masks + (long long)q * d.S;
    double sum = 0.0;
    unsigned long long cnt = 0ull, np = 0ull;
    unsigned lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    bool nf = false;
    for (long long wd = wave; wd < d.W; wd += kWaves) {
      const long long j = wd * 64 + lane;
      const float x = j < d.S ? row[j] : 0.f;
      nf = nf || !isfinite(x);
      const bool bit = j < d.S && x > 0.f;
      const unsigned long long word = __ballot(bit);
      if (lane == 0) w.bits[(long long)k * d.W + wd] = word;
      if (bit) {
        ++cnt;
        sum += 1.0 / (1.0 + exp(-(double)x));
        const unsigned n = w.ntab[j];
        np += n;
        if (n > 0u)
          for (int a = 0; a < 3; ++a) {
            lo[a] = min(lo[a], w.lo[3 * j + a]);
            hi[a] = max(hi[a], w.hi[3 * j + a]);
          }
      }
    }
    sum = wave_sum(sum);
    cnt = wave_sum(cnt);
    np = wave_sum(np);
    for (int a = 0; a < 3; ++a) {
      lo[a] = wave_min(lo[a]);
      hi[a] = wave_max(hi[a]);
    }
    const unsigned long long any_nf = __ballot(nf);
    if (lane == 0) {
      s_sum[wave] = sum;
      s_cnt[wave] = cnt;
      s_np[wave] = np;
      s_nf[wave] = any_nf != 0ull;
      for (int a = 0; a < 3; ++a) {
        s_box[wave][a] = lo[a];
        s_box[wave][3 + a] = hi[a];
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int bad = 0;
      for (int v = 1; v < kWaves; ++v) {
        sum += s_sum[v];
        cnt += s_cnt[v];
        np += s_np[v];
        for (int a = 0; a < 3; ++a) {
          lo[a] = min(lo[a], s_box[v][a]);
          hi[a] = max(hi[a], s_box[v][3 + a]);
        }
      }
      for (int v = 0; v < kWaves; ++v) bad |= s_nf[v];
      float conf = 0.f;
      if (!bad && cnt > 0ull && !(w.s->flags & kFlagScore)) {
        const int c = w.cand_cls[k];
        const float* __restrict__ cls = labels + (long long)q * (d.C + 1);  // k_sp_score's term, before it is rounded
        const double cs = row_softmax(cls, d.C).times(cls[c], (double)pred_scores[q]);
        conf = (float)(cs * sum / ((double)cnt + 1e-6)) + 0.f;
      }
      w.cand_conf[k] = conf;
      w.cand_bad[k] = bad;
      w.cand_np[k] = (long long)np;
      for (int a = 0; a < 3; ++a) {
        w.cand_box[6 * k + a] = lo[a];
        w.cand_box[6 * k + 3 + a] = hi[a];
      }
    }
    __syncthreads();  // the LDS cells are written again
  }
}

// One workgroup: the status; the candidates with conf > score_thr and then npoints > npoint_thr, sorted by
// (conf descending, candidate ascending).
__global__ __launch_bounds__(kThreads) void k_sp_filter(void* base, SpDims d, float score_thr, int npoint_thr) {
  SpWs w;
  sp_ws(base, d, &w);
  __shared__ unsigned long long s_key[kMaxTopk];
  __shared__ int s_bad[kThreads];
  __shared__ int s_status, s_score, s_rows;
  const int t = threadIdx.x;
  int bad = 0;
  for (int k = t; k < d.K; k += kThreads)
    if (w.cand_bad[k]) bad = kFlagMask;
  s_bad[t] = bad;
  if (t == 0) s_score = s_rows = 0;
  __syncthreads();
  if (t == 0) {
    int flags = w.s->flags;
    for (int j = 0; j < kThreads; ++j) flags |= s_bad[j];
    const int status = (flags & (kFlagScore | kFlagMask | kFlagCoords)) ? GAPRO_ERR_NOT_FINITE
                       : (flags & kFlagSpp) ? GAPRO_ERR_SPP_RANGE : GAPRO_OK;
    w.s->flags = flags;
    w.s->status = status;
    s_status = status;
  }
  __syncthreads();
  if (s_status != GAPRO_OK) {  // uniform over the workgroup
    if (t == 0) w.s->n_score = w.s->n_rows = 0;
    return;
  }
  for (int k = t; k < kMaxTopk; k += kThreads) {
    unsigned long long key = 0ull;  // below every key of a row: order_bits sets a bit of every finite value
    if (k < d.K && w.cand_conf[k] > score_thr) {
      atomicAdd(&s_score, 1);
      if (w.cand_np[k] > (long long)npoint_thr) {
        atomicAdd(&s_rows, 1);
        key = sort_key(w.cand_conf[k], (unsigned)k);
      }
    }
    s_key[k] = key;
  }
  sort_desc(s_key);
  const int n_rows = s_rows;
  for (int r = t; r < n_rows; r += kThreads) w.row_cand[r] = (int)key_index(s_key[r]);
  if (t == 0) {
    w.s->n_score = s_score;
    w.s->n_rows = n_rows;
  }
}

// ---- step 6 ------------------------------------------------------------------------------------------------------
// m(k, .) of candidate k as select_runs.h's `bit`: m(k, p) for p in [0, N); 0 outside.  `filter` found every superpoint
// id in range, or there are no rows.
__device__ inline auto mask_at(const SpWs& w, const SpDims& d, const void* spps, int spps_i64, int k) {
  return [=](long long p) -> int {
    if (p < 0 || p >= d.N) return 0;
    const long long s = idx_at(spps, spps_i64, p);
    return (int)((w.bits[(long long)k * d.W + (s >> 6)] >> (s & 63)) & 1ull);
  };
}

// blockIdx = (chunk, output row): the transitions at the positions [chunk * chunk_len, ...) of [0, N].
__global__ __launch_bounds__(kThreads) void k_sp_trans(void* base, SpDims d, const void* __restrict__ spps,
                                                       int spps_i64) {
  SpWs w;
  sp_ws(base, d, &w);
  const int r = blockIdx.y;
  if (r >= w.s->n_rows) return;
  const ChunkTally c = chunk_tally(d.chunk_len, d.N, mask_at(w, d, spps, spps_i64, w.row_cand[r]));
  if (threadIdx.x == 0) w.chunk_cnt[(size_t)r * d.nchunks + blockIdx.x] = c.trans;  // the cell is this workgroup's alone
}

// A wave per row: the chunk counts become the counts before the chunk; the row's transitions.
__global__ __launch_bounds__(kThreads) void k_sp_chunks(void* base, SpDims d) {
  SpWs w;
  sp_ws(base, d, &w);
  const int n_rows = w.s->n_rows, n_waves = gridDim.x * kWaves;
  for (int r = blockIdx.x * kWaves + (threadIdx.x >> 6); r < n_rows; r += n_waves) {
    const unsigned trans = scan_chunks(w.chunk_cnt + (size_t)r * d.nchunks, d.nchunks);
    if ((threadIdx.x & 63) == 0) w.row_trans[r] = trans;
  }
}

// One workgroup.  Thread t owns kRowsPer consecutive rows: by a prefix over the threads the transitions before them; the
// header.
__global__ __launch_bounds__(kThreads) void k_sp_finish(void* base, SpDims d,
                                                        gapro_spf_predict_header* __restrict__ header) {
  SpWs w;
  sp_ws(base, d, &w);
  constexpr int kRowsPer = kMaxTopk / kThreads;
  __shared__ unsigned long long s_sum[kThreads];
  const int n_rows = w.s->n_rows, t = threadIdx.x, r0 = t * kRowsPer;
  unsigned trans[kRowsPer];
  unsigned long long sum = 0ull;
  for (int i = 0; i < kRowsPer; ++i) {
    trans[i] = r0 + i < n_rows ? w.row_trans[r0 + i] : 0u;
    sum += trans[i];
  }
  unsigned long long total, off = block_sum_before(s_sum, sum, &total);
  int* counts = (int*)(header + 1);
  for (int i = 0; i < kRowsPer; ++i)
    if (r0 + i < n_rows) {
      w.run_off[r0 + i] = (long long)off;
      counts[r0 + i] = (int)(trans[i] / 2u);
      off += trans[i];
    }
  if (t != 0) return;
  w.run_off[n_rows] = (long long)total;
  w.s->total_trans = (long long)total;
  const bool ok = w.s->status == GAPRO_OK;
  header->status = w.s->status;
  header->flags = w.s->flags;
  header->n_candidates = ok ? w.s->n_cand : 0;
  header->n_after_score = ok ? w.s->n_score : 0;
  header->n_rows = n_rows;
  header->reserved = 0;
  header->total_runs = (long long)(total / 2);
}

// ---- fill --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_sp_fill_rows(void* base, SpDims d, long long cap_rows, long long cap_runs,
                                                           float* __restrict__ conf, int* __restrict__ label,
                                                           unsigned* __restrict__ box, int* __restrict__ query,
                                                           long long* __restrict__ run_offsets,
                                                           gapro_spf_predict_header* __restrict__ header) {
  SpWs w;
  sp_ws(base, d, &w);
  if (!fill_ok(*w.s, cap_rows, cap_runs)) {
    if (header && blockIdx.x == 0 && threadIdx.x == 0 && w.s->status == GAPRO_OK) header->status = GAPRO_ERR_WORKSPACE;
    return;
  }
  const int n = w.s->n_rows;
  for (int r = blockIdx.x * kThreads + threadIdx.x; r <= n; r += gridDim.x * kThreads) {
    if (run_offsets) run_offsets[r] = w.run_off[r] / 2;
    if (r == n) continue;
    const int k = w.row_cand[r];
    if (conf) conf[r] = w.cand_conf[k];
    if (label) label[r] = w.cand_cls[k] + 1;
    if (query) query[r] = w.cand_q[k];
    if (box)
      for (int j = 0; j < 6; ++j) box[6 * (size_t)r + j] = order_bits_inv(w.cand_box[6 * k + j]);
  }
}

// blockIdx = (chunk, output row): the positions of the chunk's transitions, 1-based, in order; the mask bytes.
__global__ __launch_bounds__(kThreads) void k_sp_fill_runs(void* base, SpDims d, const void* __restrict__ spps,
                                                           int spps_i64, long long cap_rows, long long cap_runs,
                                                           long long* __restrict__ runs,
                                                           unsigned char* __restrict__ masks) {
  SpWs w;
  sp_ws(base, d, &w);
  if (!fill_ok(*w.s, cap_rows, cap_runs)) return;
  const int r = blockIdx.y;
  if (r >= w.s->n_rows) return;
  emit_runs(d.chunk_len, d.N, mask_at(w, d, spps, spps_i64, w.row_cand[r]),
            w.run_off[r] + w.chunk_cnt[(size_t)r * d.nchunks + blockIdx.x], runs,
            masks ? masks + (long long)r * d.N : nullptr);
}

__global__ __launch_bounds__(kThreads) void k_sp_fill_lengths(void* base, SpDims d, long long cap_rows,
                                                              long long cap_runs, long long* __restrict__ runs) {
  SpWs w;
  sp_ws(base, d, &w);
  if (fill_ok(*w.s, cap_rows, cap_runs)) ends_to_lengths(runs, w.s->total_trans / 2);
}

// ---- host ----------------------------------------------------------------------------------------------------------
// the sizes both calls and the workspace size agree on; false: refused
bool make_dims(const gapro_spf_predict_inputs* in, const gapro_spf_predict_params* p, SpDims* d) {
  if (!in || !p) return false;
  const long long Q = in->n_queries, S = in->n_spps, N = in->n_points, C = p->num_class;
  if (Q < 1 || C < 1 || Q > kMaxScores || Q * C > kMaxScores) return false;
  if (S < 1 || S > kMaxIndex || N < 1 || N > kMaxIndex) return false;
  if (p->topk_insts < 1 || p->topk_insts > kMaxTopk || p->npoint_thr < 0 || !std::isfinite(p->score_thr)) return false;
  *d = SpDims{};
  d->Q = Q;
  d->S = S;
  d->N = N;
  d->W = (S + 63) / 64;
  d->C = (int)C;
  d->K = (int)(Q * C < p->topk_insts ? Q * C : p->topk_insts);
  chunking(N, &d->nchunks, &d->chunk_len);
  return true;
}

// what both calls refuse before anything is launched
int check_args(gapro_ctx* ctx, const char* who, const gapro_spf_predict_inputs* in, const gapro_spf_predict_params* p,
               SpDims* d, const void* d_ws, size_t ws_bytes) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  bool ok = make_dims(in, p, d) && d_ws;
  ok = ok && in->labels && in->pred_scores && in->masks && in->superpoints && in->coords_float &&
       (in->superpoints_i64 == 0 || in->superpoints_i64 == 1);
  if (!ok) return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: bad argument", who);
  SpWs w;
  if (ws_bytes < align_up(sp_ws(nullptr, *d, &w), 256))
    return gapro_fail(ctx, GAPRO_ERR_WORKSPACE, "%s: workspace too small", who);
  return GAPRO_OK;
}

}  // namespace

extern "C" {

size_t gapro_spf_predict_workspace_bytes(const gapro_spf_predict_inputs* in, const gapro_spf_predict_params* params) {
  SpDims d;
  if (!make_dims(in, params, &d)) return 0;
  SpWs w;
  return align_up(sp_ws(nullptr, d, &w), 256);
}

size_t gapro_spf_predict_header_bytes(const gapro_spf_predict_inputs* in, const gapro_spf_predict_params* params) {
  SpDims d;
  if (!make_dims(in, params, &d)) return 0;
  return GAPRO_SPF_PREDICT_HEADER_BYTES(d.K);
}

int gapro_spf_predict_count(gapro_ctx* ctx, void* stream_, const gapro_spf_predict_inputs* in,
                            const gapro_spf_predict_params* params, void* d_workspace, size_t workspace_bytes,
                            gapro_spf_predict_header* d_header, gapro_spf_predict_header* h_header_pinned) {
  SpDims d;
  const int rc = check_args(ctx, "gapro_spf_predict_count", in, params, &d, d_workspace, workspace_bytes);
  if (rc != GAPRO_OK) return rc;
  if (!d_header) return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_spf_predict_count: bad argument");
  hipStream_t stream = (hipStream_t)stream_;
  SpWs w;
  sp_ws(d_workspace, d, &w);
  GAPRO_HIP_CHECK(ctx, hipMemsetAsync(d_workspace, 0, (size_t)(w.zero_end - (char*)d_workspace), stream));
  GAPRO_HIP_CHECK(ctx, hipMemsetAsync(w.lo, 0xff, (size_t)(w.ones_end - (char*)w.lo), stream));
  const dim3 block(kThreads);
  hipLaunchKernelGGL(k_sp_score, dim3(grid_for(d.Q, 1, kGridCap)), block, 0, stream, d_workspace, d, in->labels,
                     in->pred_scores);
  hipLaunchKernelGGL(k_sp_select, dim3(1), block, 0, stream, d_workspace, d);
  hipLaunchKernelGGL(k_sp_points, dim3(grid_for(d.N, 1, kGridCap)), block, 0, stream, d_workspace, d, in->superpoints,
                     in->superpoints_i64, in->coords_float);
  hipLaunchKernelGGL(k_sp_rows, dim3(d.K), block, 0, stream, d_workspace, d, in->labels, in->pred_scores, in->masks);
  hipLaunchKernelGGL(k_sp_filter, dim3(1), block, 0, stream, d_workspace, d, params->score_thr, params->npoint_thr);
  hipLaunchKernelGGL(k_sp_trans, dim3(d.nchunks, d.K), block, 0, stream, d_workspace, d, in->superpoints,
                     in->superpoints_i64);
  hipLaunchKernelGGL(k_sp_chunks, dim3(grid_for((long long)d.K * 64, 1, kGridCap)), block, 0, stream, d_workspace, d);
  hipLaunchKernelGGL(k_sp_finish, dim3(1), block, 0, stream, d_workspace, d, d_header);
  GAPRO_LAUNCH_CHECK(ctx);
  if (h_header_pinned)
    GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(h_header_pinned, d_header, GAPRO_SPF_PREDICT_HEADER_BYTES(d.K),
                                        hipMemcpyDeviceToHost, stream));
  return GAPRO_OK;
}

int gapro_spf_predict_fill(gapro_ctx* ctx, void* stream_, const gapro_spf_predict_inputs* in,
                           const gapro_spf_predict_params* params, void* d_workspace, size_t workspace_bytes,
                           float* d_conf, int32_t* d_label_id, float* d_box, int32_t* d_query, int64_t cap_rows,
                           int64_t* d_run_offsets, int64_t* d_runs, int64_t cap_runs, uint8_t* d_masks,
                           gapro_spf_predict_header* d_header) {
  SpDims d;
  const int rc = check_args(ctx, "gapro_spf_predict_fill", in, params, &d, d_workspace, workspace_bytes);
  if (rc != GAPRO_OK) return rc;
  if (cap_rows < 1 || cap_runs < 0 || !d_run_offsets || (cap_runs > 0 && !d_runs) || (d_masks && cap_rows > kMaxTopk))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_spf_predict_fill: bad argument");
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 block(kThreads);
  const long long rows = (long long)cap_rows, cap = (long long)cap_runs;
  hipLaunchKernelGGL(k_sp_fill_rows, dim3(grid_for(d.K + 1, 1, kGridCap)), block, 0, stream, d_workspace, d, rows, cap,
                     d_conf, (int*)d_label_id, (unsigned*)d_box, (int*)d_query, (long long*)d_run_offsets, d_header);
  if (cap > 0 || d_masks) {
    const int grid_rows = (int)(rows < d.K ? rows : d.K);
    hipLaunchKernelGGL(k_sp_fill_runs, dim3(d.nchunks, grid_rows), block, 0, stream, d_workspace, d, in->superpoints,
                       in->superpoints_i64, rows, cap, (long long*)d_runs, d_masks);
    if (cap > 0)
      hipLaunchKernelGGL(k_sp_fill_lengths, dim3(grid_for(cap, 1, kGridCap)), block, 0, stream, d_workspace, d, rows,
                         cap, (long long*)d_runs);
  }
  GAPRO_LAUNCH_CHECK(ctx);
  return GAPRO_OK;
}

}  // extern "C"
