// ScanNet instance AP of pseudo-labels: the integer tables behind the reference's gapro/eval_ap_ps_labels.py with
// ISBNet's ScanNetEval.assign_instances_for_scan (instance_eval.py:244-336), for a batch of scenes laid out back to
// back in the label arrays (blockIdx.y = scene).  The matching and the AP (evaluate_matches) run on the host.
//
// A GT point's key is the reference's code g = (sem + 1) * 1000 + (inst + 1) after the script's remap (:59-60):
// class c = sem + 1 in 1..18 and inst + 1 in [0, 1000) make a GT instance; any other class, or inst + 1 < 0, is void.
// An inst >= 999 (inst + 1 >= 1000) would carry into the class digit: it sets the scene's status.
//   gapro_eval_ap_keys   : pass 1 marks the present keys in a per-scene bitmap (LDS-privatised), and a per-scene
//                          exclusive scan of the word popcounts turns it into dense ranks in ascending code order.
//   gapro_eval_ap_tables : pass 2 tallies per point the (key rank + 1, pseudo id + 1) pair count (row 0 = void,
//                          column 0 = pseudo id -100), per pseudo id its first point (packed with the label of that
//                          point) and the sum of rint(prob * 2^32); the finalize derives the key codes and counts
//                          and the per-id counts from the pair table.
//   gapro_eval_ap_tables_rows : the same pass with T probability thresholds.  A point tallies into the tables of its
//                          bin b = #{j : prob >= thresholds[j]} (one pair cell, one first point, one probability sum,
//                          as without thresholds); row t keeps the points of the bins t..T, so a suffix sum (pair
//                          cells, probability sums) / suffix min (first points) over the bins turns the bin tables
//                          into the row tables, and the finalize derives every row's counts and labels from them.
//                          Key ranks are over the whole scene: a key without a kept point has count 0 in that row.
// Integer atomics only: every table is bit-identical to a plain tally of the scene, whatever the batch.
#include "common.h"
#include "eval_labels.h"
#include "exact_sum.h"
#include "launch_util.h"

#include <algorithm>
#include <type_traits>

namespace {

constexpr int kThreads = 256;
constexpr int kApClasses = 18;                        // ScanNet's valid class ids 1..18
constexpr int kApInst = 1000;                         // inst + 1 in [0, 1000): the instance digits of a code
constexpr int kApCodes = kApClasses * kApInst;        // (class, inst + 1) keys, ranked in ascending code order
constexpr int kApWords = (kApCodes + 31) / 32;        // presence bitmap words per scene
constexpr int kPairLds = 8192;                        // pair cells kept in LDS ((keys + 1) x (ids + 1))
constexpr int kIdLds = 512;                           // per-id first points / probability sums kept in LDS
constexpr unsigned long long kFirstNone = ~0ull;
constexpr int kProbShift = 32;                        // a probability term is rint(prob * 2^32)


// one scene in the workspace: bitmap u32[kApWords] | exclusive rank of each word i32[kApWords] | first u64[max_ps]
// (bin / row 0); the first points of the bins / rows 1..T follow the last scene's block as u64[T][ids of the batch]
__host__ __device__ inline size_t scene_bytes(int max_ps) {
  return align_up((size_t)kApWords * 8 + (size_t)max_ps * sizeof(unsigned long long), 256);
}
struct SceneWs {
  unsigned* bits;
  int* rank;
  unsigned long long* first;  // (scene-local point << 8) | label id (1..18, 0 = not a class) of the id's first point
};
__device__ inline SceneWs scene_ws(void* ws, const gapro_eval_ap_scene& s) {
  SceneWs w;
  w.bits = (unsigned*)((char*)ws + s.ws_offset);
  w.rank = (int*)(w.bits + kApWords);
  w.first = (unsigned long long*)(w.rank + kApWords);
  return w;
}

// the row dimension of a launch: B = K + 1 bins / rows, each output's row stride, the first points of the rows 1..K
struct Rows {
  Thresholds thr;
  int K;
  long long n_keys, n_ids, n_cells;  // entries of the whole batch per key / per id / pair output: the row strides
  unsigned long long* first;         // [K][n_ids]
};
__device__ inline unsigned long long* first_of(const SceneWs& w, const Rows& r, const gapro_eval_ap_scene& s, int b) {
  return b == 0 ? w.first : r.first + (long long)(b - 1) * r.n_ids + s.id_offset;
}

// the key index of a GT point ((class - 1) * 1000 + inst + 1 = code - 1000, ascending in the code), -1 = void,
// -2 = inst >= 999
template <class TGS, class TGI>
__device__ inline int gt_key(const TGS* sem_gt, const TGI* inst_gt, long long i, int remap) {
  const long long sg = remap_gt(label_at(sem_gt, i), remap), g = label_at(inst_gt, i);
  if (g >= kApInst - 1) return -2;  // inst + 1 = 1000 is the next class's inst + 1 = 0
  if (g < -1 || sg < 0 || sg >= kApClasses) return -1;  // code 0, class 0 (wall / floor after the remap) or > 18
  return (int)sg * kApInst + (int)g + 1;
}

__global__ __launch_bounds__(kThreads) void k_ap_init(const gapro_eval_ap_scene* __restrict__ scenes, void* ws) {
  const gapro_eval_ap_scene s = scenes[blockIdx.y];
  SceneWs w = scene_ws(ws, s);
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < kApWords + (long long)s.max_ps; i += stride) {
    if (i < kApWords) w.bits[i] = 0u;
    else w.first[i - kApWords] = kFirstNone;
  }
}

// pass 1: the keys present in each scene
template <class TGS, class TGI>
__global__ __launch_bounds__(kThreads) void k_ap_mark(const gapro_eval_ap_scene* __restrict__ scenes,
                                                      const TGS* __restrict__ sem_gt, const TGI* __restrict__ inst_gt,
                                                      int remap, void* ws, int* __restrict__ status) {
  const int scene = blockIdx.y;
  const gapro_eval_ap_scene s = scenes[scene];
  const long long n = s.n_points, off = s.point_offset;
  if ((long long)blockIdx.x * kThreads >= n) return;
  __shared__ unsigned s_bits[kApWords];
  for (int j = threadIdx.x; j < kApWords; j += kThreads) s_bits[j] = 0u;
  __syncthreads();
  bool bad = false;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    const int k = gt_key(sem_gt, inst_gt, off + i, remap);
    if (k >= 0) atomicOr(&s_bits[k >> 5], 1u << (k & 31));
    bad |= k == -2;
  }
  if (bad) atomicExch(&status[scene], GAPRO_ERR_BAD_ARG);
  __syncthreads();
  unsigned* bits = scene_ws(ws, s).bits;
  for (int j = threadIdx.x; j < kApWords; j += kThreads)
    if (s_bits[j]) atomicOr(&bits[j], s_bits[j]);
}

// per scene (one workgroup): exclusive prefix of the word popcounts -> ranks; the key count
__global__ __launch_bounds__(kThreads) void k_ap_rank(const gapro_eval_ap_scene* __restrict__ scenes, void* ws,
                                                      int* __restrict__ n_keys) {
  constexpr int kPer = (kApWords + kThreads - 1) / kThreads;
  SceneWs w = scene_ws(ws, scenes[blockIdx.y]);
  __shared__ int s_sum[kThreads];
  const int w0 = threadIdx.x * kPer;
  int own = 0;
  for (int j = w0; j < w0 + kPer && j < kApWords; ++j) own += __popc(w.bits[j]);
  s_sum[threadIdx.x] = own;
  __syncthreads();
  for (int d = 1; d < kThreads; d <<= 1) {  // inclusive Hillis-Steele scan over the threads' sums
    const int v = threadIdx.x >= d ? s_sum[threadIdx.x - d] : 0;
    __syncthreads();
    s_sum[threadIdx.x] += v;
    __syncthreads();
  }
  int r = s_sum[threadIdx.x] - own;
  for (int j = w0; j < w0 + kPer && j < kApWords; ++j) {
    w.rank[j] = r;
    r += __popc(w.bits[j]);
  }
  if (threadIdx.x == kThreads - 1) n_keys[blockIdx.y] = s_sum[kThreads - 1];
}

// pass 2: pair counts, first points and probability sums per bin; tables in LDS while all bins of them fit
template <class TGS, class TGI, class TPS, class TPI>
__global__ __launch_bounds__(kThreads) void k_ap_tally(const gapro_eval_ap_scene* __restrict__ scenes,
                                                       const TGS* __restrict__ sem_gt, const TGI* __restrict__ inst_gt,
                                                       const TPS* __restrict__ sem_ps, const TPI* __restrict__ inst_ps,
                                                       const float* __restrict__ prob, Rows rows, int remap,
                                                       void* ws, int* __restrict__ pair,
                                                       long long* __restrict__ ps_sum, int* __restrict__ status) {
  const int scene = blockIdx.y;
  const gapro_eval_ap_scene s = scenes[scene];
  const long long n = s.n_points, off = s.point_offset;
  if ((long long)blockIdx.x * kThreads >= n) return;
  SceneWs w = scene_ws(ws, s);
  const int P = s.max_ps, W = P + 1, K = rows.K, B = K + 1;
  const long long cells = (long long)(s.n_keys + 1) * W;
  const bool lds_pair = cells * B <= kPairLds, lds_id = (long long)P * B <= kIdLds;
  __shared__ unsigned s_bits[kApWords];
  __shared__ int s_rank[kApWords];
  __shared__ int s_pair[kPairLds];
  __shared__ unsigned long long s_first[kIdLds], s_sum[kIdLds];
  for (int j = threadIdx.x; j < kApWords; j += kThreads) {
    s_bits[j] = w.bits[j];
    s_rank[j] = w.rank[j];
  }
  if (lds_pair)
    for (int j = threadIdx.x; j < (int)cells * B; j += kThreads) s_pair[j] = 0;
  if (lds_id)
    for (int j = threadIdx.x; j < P * B; j += kThreads) {
      s_first[j] = kFirstNone;
      s_sum[j] = 0ull;
    }
  __syncthreads();
  int* g_pair = pair + s.pair_offset;
  unsigned long long* g_sum = (unsigned long long*)ps_sum + s.id_offset;
  bool bad = false;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    const long long gi_ = off + i;
    const int k = gt_key(sem_gt, inst_gt, gi_, remap);
    int row = 0;
    if (k >= 0) {
      row = 1 + s_rank[k >> 5] + __popc(s_bits[k >> 5] & ((1u << (k & 31)) - 1u));
      if (row > s.n_keys) {  // n_keys below what gapro_eval_ap_keys counted
        bad = true;
        continue;
      }
    }
    bad |= k == -2;
    float pr = 0.0f;
    if (prob) {
      pr = prob[gi_];
      if (!(pr >= 0.0f && pr <= 1.0f)) {
        bad = true;
        pr = 0.0f;
      }
    }
    const long long p = label_at(inst_ps, gi_);
    if (p != -100 && (p < 0 || p >= P)) {
      bad = true;
      continue;
    }
    const int col = p == -100 ? 0 : (int)p + 1;
    const int b = K ? prob_bin(rows.thr, K, pr) : 0;
    const long long cell = (long long)row * W + col;
    if (lds_pair) atomicAdd(&s_pair[b * (int)cells + (int)cell], 1);
    else atomicAdd(&g_pair[b * rows.n_cells + cell], 1);
    if (col) {
      const long long sp = label_at(sem_ps, gi_);
      const unsigned long long first =
          ((unsigned long long)i << 8) | (unsigned long long)(sp >= 0 && sp < kApClasses ? sp + 1 : 0);
      if (lds_id) atomicMin(&s_first[b * P + p], first);
      else atomicMin(&first_of(w, rows, s, b)[p], first);
      if (prob) {
        const unsigned long long q = (unsigned long long)to_fixed((double)pr, kProbShift);
        if (lds_id) atomicAdd(&s_sum[b * P + p], q);
        else atomicAdd(&g_sum[b * rows.n_ids + p], q);
      }
    }
  }
  if (bad) atomicExch(&status[scene], GAPRO_ERR_BAD_ARG);
  __syncthreads();
  if (lds_pair)
    for (int j = threadIdx.x; j < (int)cells * B; j += kThreads)
      if (s_pair[j]) atomicAdd(&g_pair[j / (int)cells * rows.n_cells + j % (int)cells], s_pair[j]);
  if (lds_id)
    for (int j = threadIdx.x; j < P * B; j += kThreads) {
      const int b = j / P, p = j % P;
      if (s_first[j] != kFirstNone) atomicMin(&first_of(w, rows, s, b)[p], s_first[j]);
      if (s_sum[j]) atomicAdd(&g_sum[b * rows.n_ids + p], s_sum[j]);
    }
}

// bins -> rows: row t = bins t..K (suffix sum of the pair cells and the probability sums, suffix min of the first points)
__global__ __launch_bounds__(kThreads) void k_ap_suffix(const gapro_eval_ap_scene* __restrict__ scenes, void* ws, Rows rows,
                                                        int* __restrict__ pair, long long* __restrict__ ps_sum) {
  const gapro_eval_ap_scene s = scenes[blockIdx.y];
  SceneWs w = scene_ws(ws, s);
  const long long P = s.max_ps, cells = (long long)(s.n_keys + 1) * (P + 1), items = cells + 2 * P;
  for (long long it = (long long)blockIdx.x * kThreads + threadIdx.x; it < items; it += (long long)gridDim.x * kThreads) {
    if (it < cells) {
      int* a = pair + s.pair_offset + it;
      for (int b = rows.K - 1; b >= 0; --b) a[b * rows.n_cells] += a[(b + 1) * rows.n_cells];
    } else if (it < cells + P) {
      long long* a = ps_sum + s.id_offset + (it - cells);
      for (int b = rows.K - 1; b >= 0; --b) a[b * rows.n_ids] += a[(b + 1) * rows.n_ids];
    } else {
      const long long p = it - cells - P;
      unsigned long long f = first_of(w, rows, s, rows.K)[p];
      for (int b = rows.K - 1; b >= 0; --b) {
        unsigned long long* a = first_of(w, rows, s, b) + p;
        f = *a < f ? *a : f;
        *a = f;
      }
    }
  }
}

// per scene and row (blockIdx.z): the key codes (class * 1000 + inst + 1) and point counts, and per pseudo id the
// point count, the void points (pair row 0) and the label id of the first point, from the row's pair table
__global__ __launch_bounds__(kThreads) void k_ap_finalize(const gapro_eval_ap_scene* __restrict__ scenes, void* ws,
                                                          Rows rows, const int* __restrict__ pair,
                                                          int* __restrict__ key_code, int* __restrict__ key_n,
                                                          int* __restrict__ ps_n, int* __restrict__ ps_label,
                                                          int* __restrict__ ps_void) {
  const gapro_eval_ap_scene s = scenes[blockIdx.y];
  SceneWs w = scene_ws(ws, s);
  const int P = s.max_ps, W = P + 1, K = s.n_keys, z = blockIdx.z;
  const int* t = pair + z * rows.n_cells + s.pair_offset;
  const unsigned long long* first = first_of(w, rows, s, z);
  key_code += z * rows.n_keys;
  key_n += z * rows.n_keys;
  ps_n += z * rows.n_ids;
  ps_label += z * rows.n_ids;
  ps_void += z * rows.n_ids;
  const long long items = (long long)kApWords + K + P;
  for (long long it = (long long)blockIdx.x * kThreads + threadIdx.x; it < items; it += (long long)gridDim.x * kThreads) {
    if (it < kApWords) {
      const int j = (int)it;
      unsigned b = w.bits[j];
      int r = w.rank[j];
      while (b) {
        const int bit = __ffs(b) - 1, k = j * 32 + bit;
        b &= b - 1u;
        if (r < K) key_code[s.key_offset + r] = (k / kApInst + 1) * 1000 + k % kApInst;
        ++r;
      }
    } else if (it < (long long)kApWords + K) {
      const int k = (int)(it - kApWords);
      const int* row = t + (long long)(k + 1) * W;
      int c = 0;
      for (int p = 0; p < W; ++p) c += row[p];
      key_n[s.key_offset + k] = c;
    } else {
      const int p = (int)(it - kApWords - K);
      int c = 0;
      for (int k = 0; k <= K; ++k) c += t[(long long)k * W + p + 1];
      ps_n[s.id_offset + p] = c;
      ps_void[s.id_offset + p] = t[p + 1];
      const unsigned long long f = first[p];
      ps_label[s.id_offset + p] = f == kFirstNone ? 0 : (int)(f & 0xffull);
    }
  }
}

bool valid_scene(const gapro_eval_ap_scene& s) {
  return s.n_points >= 0 && s.point_offset >= 0 && s.max_ps >= 1 && s.max_ps < (1 << 30);
}

}  // namespace

extern "C" {

size_t gapro_eval_ap_workspace_bytes(gapro_eval_ap_scene* h_scenes, int32_t n_scenes) {
  if (!h_scenes || n_scenes < 1 || n_scenes > 65535) return 0;
  size_t bytes = 0;
  long long ids = 0;
  for (int i = 0; i < n_scenes; ++i) {
    gapro_eval_ap_scene& s = h_scenes[i];
    if (!valid_scene(s)) return 0;
    s.ws_offset = (int64_t)bytes;
    s.id_offset = ids;
    bytes += scene_bytes(s.max_ps);
    ids += s.max_ps;
  }
  return bytes;
}

size_t gapro_eval_ap_workspace_bytes_rows(gapro_eval_ap_scene* h_scenes, int32_t n_scenes, int32_t n_thresholds) {
  if (n_thresholds < 0 || n_thresholds > GAPRO_EVAL_MAX_THRESHOLDS) return 0;
  const size_t bytes = gapro_eval_ap_workspace_bytes(h_scenes, n_scenes);
  if (!bytes) return 0;
  const gapro_eval_ap_scene& last = h_scenes[n_scenes - 1];
  return bytes + (size_t)n_thresholds * (size_t)(last.id_offset + last.max_ps) * sizeof(unsigned long long);
}

int64_t gapro_eval_ap_pair_cells(gapro_eval_ap_scene* h_scenes, int32_t n_scenes) {
  if (!h_scenes || n_scenes < 1 || n_scenes > 65535) return 0;
  long long keys = 0, cells = 0;
  for (int i = 0; i < n_scenes; ++i) {
    gapro_eval_ap_scene& s = h_scenes[i];
    if (!valid_scene(s) || s.n_keys < 0 || s.n_keys > kApCodes) return 0;
    s.key_offset = keys;
    s.pair_offset = cells;
    keys += s.n_keys;
    cells += (long long)(s.n_keys + 1) * (s.max_ps + 1);
  }
  return cells;
}

// the descriptors as the two sizing functions laid them out, inside the arrays and the workspace (the scenes' blocks and
// more_rows first-point rows behind them, at *rows_at): GAPRO_OK or the error
static int check_layout(gapro_ctx* ctx, const char* fn, int32_t n_scenes, const gapro_eval_ap_scene* h_scenes,
                         int64_t n_total_points, size_t workspace_bytes, bool with_keys, int more_rows, long long* n_max,
                         long long* ps_max, long long* fin_max, size_t* rows_at) {
  size_t bytes = 0;
  long long ids = 0, keys = 0, cells = 0;
  *n_max = *ps_max = *fin_max = 0;
  for (int i = 0; i < n_scenes; ++i) {
    const gapro_eval_ap_scene& s = h_scenes[i];
    if (!valid_scene(s) || s.point_offset > n_total_points || s.n_points > n_total_points - s.point_offset ||
        s.ws_offset != (int64_t)bytes || s.id_offset != ids ||
        (with_keys && (s.n_keys < 0 || s.n_keys > kApCodes || s.key_offset != keys || s.pair_offset != cells))) {
      return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: scene %d: bad descriptor", fn, i);
    }
    bytes += scene_bytes(s.max_ps);
    ids += s.max_ps;
    if (with_keys) {
      keys += s.n_keys;
      cells += (long long)(s.n_keys + 1) * (s.max_ps + 1);
    }
    *n_max = std::max<long long>(*n_max, s.n_points);
    *ps_max = std::max<long long>(*ps_max, s.max_ps);
    *fin_max = std::max<long long>(*fin_max, (long long)kApWords + (with_keys ? s.n_keys : 0) + s.max_ps);
  }
  *rows_at = bytes;
  if (workspace_bytes < bytes + (size_t)more_rows * (size_t)ids * sizeof(unsigned long long))
    return gapro_fail(ctx, GAPRO_ERR_WORKSPACE, "%s: workspace too small", fn);
  return GAPRO_OK;
}

int gapro_eval_ap_keys(gapro_ctx* ctx, void* stream_, int32_t n_scenes, const gapro_eval_ap_scene* h_scenes,
                       gapro_eval_ap_scene* d_scenes, int64_t n_total_points, int32_t sem_gt_dtype, const void* d_sem_gt,
                       int32_t inst_gt_dtype, const void* d_inst_gt, int32_t scannet_remap, void* d_workspace,
                       size_t workspace_bytes, int32_t* d_n_keys, int32_t* d_status) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  if (n_scenes < 1 || n_scenes > 65535 || !h_scenes || !d_scenes || n_total_points < 0 || !d_workspace || !d_n_keys ||
      !d_status || (n_total_points > 0 && (!d_sem_gt || !d_inst_gt)))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_eval_ap_keys: bad argument");
  if (!with_label_type(sem_gt_dtype, [](auto) {}) || !with_label_type(inst_gt_dtype, [](auto) {}))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_eval_ap_keys: unsupported label dtype code");
  long long n_max, ps_max, fin_max;
  size_t rows_at;
  const int rc = check_layout(ctx, "gapro_eval_ap_keys", n_scenes, h_scenes, n_total_points, workspace_bytes, false, 0,
                              &n_max, &ps_max, &fin_max, &rows_at);
  if (rc != GAPRO_OK) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(d_scenes, h_scenes, (size_t)n_scenes * sizeof(gapro_eval_ap_scene),
                                      hipMemcpyHostToDevice, stream));
  GAPRO_HIP_CHECK(ctx, hipMemsetAsync(d_status, 0, (size_t)n_scenes * sizeof(int32_t), stream));
  hipLaunchKernelGGL(k_ap_init, dim3(grid_for(kApWords + ps_max, 1, 64), n_scenes), dim3(kThreads), 0, stream,
                     d_scenes, d_workspace);
  if (n_max > 0)
    with_label_type(sem_gt_dtype, [&](auto sgt) {
      with_label_type(inst_gt_dtype, [&](auto igt) {
        using TGS = std::remove_const_t<std::remove_pointer_t<decltype(sgt)>>;
        using TGI = std::remove_const_t<std::remove_pointer_t<decltype(igt)>>;
        hipLaunchKernelGGL((k_ap_mark<TGS, TGI>), dim3(grid_for(n_max, 8, 128), n_scenes), dim3(kThreads), 0,
                           stream, d_scenes, (const TGS*)d_sem_gt, (const TGI*)d_inst_gt, (int)(scannet_remap != 0),
                           d_workspace, (int*)d_status);
      });
    });
  hipLaunchKernelGGL(k_ap_rank, dim3(1, n_scenes), dim3(kThreads), 0, stream, d_scenes, d_workspace, (int*)d_n_keys);
  GAPRO_LAUNCH_CHECK(ctx);
  return GAPRO_OK;
}

// gapro_eval_ap_tables_rows, named fn in the errors
static int ap_tables_rows(const char* fn, gapro_ctx* ctx, void* stream_, int32_t n_scenes,
                          const gapro_eval_ap_scene* h_scenes, gapro_eval_ap_scene* d_scenes, int64_t n_total_points,
                          int32_t sem_gt_dtype, const void* d_sem_gt, int32_t inst_gt_dtype, const void* d_inst_gt,
                          int32_t sem_ps_dtype, const void* d_sem_ps, int32_t inst_ps_dtype, const void* d_inst_ps,
                          const float* d_prob, int32_t n_thresholds, const float* h_thresholds, int32_t scannet_remap,
                          void* d_workspace, size_t workspace_bytes, int32_t* d_key_code, int32_t* d_key_n,
                          int32_t* d_ps_n, int32_t* d_ps_label, int32_t* d_ps_void, int64_t* d_ps_sum, int32_t* d_pair,
                          int32_t* d_status) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  const int K = n_thresholds, B = K + 1;
  if (n_scenes < 1 || n_scenes > 65535 || !h_scenes || !d_scenes || n_total_points < 0 || K < 0 ||
      K > GAPRO_EVAL_MAX_THRESHOLDS || (K > 0 && (!h_thresholds || (n_total_points > 0 && !d_prob))) || !d_workspace ||
      !d_key_code || !d_key_n || !d_ps_n || !d_ps_label || !d_ps_void || !d_ps_sum || !d_pair || !d_status ||
      (n_total_points > 0 && (!d_sem_gt || !d_inst_gt || !d_sem_ps || !d_inst_ps)))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: bad argument", fn);
  if (!with_label_type(sem_gt_dtype, [](auto) {}) || !with_label_type(inst_gt_dtype, [](auto) {}) ||
      !with_ps_type(sem_ps_dtype, [](auto) {}) || !with_ps_type(inst_ps_dtype, [](auto) {}))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: unsupported label dtype code", fn);
  Rows rows = {};
  rows.K = K;
  for (int j = 0; j < K; ++j) {
    rows.thr.t[j] = h_thresholds[j];
    if (!(rows.thr.t[j] == rows.thr.t[j]) || (j > 0 && !(rows.thr.t[j] >= rows.thr.t[j - 1])))
      return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: thresholds must be ascending and not NaN", fn);
  }
  long long n_max, ps_max, fin_max, suffix_max = 0;
  size_t rows_at;
  const int rc = check_layout(ctx, fn, n_scenes, h_scenes, n_total_points, workspace_bytes, true, K, &n_max, &ps_max,
                              &fin_max, &rows_at);
  if (rc != GAPRO_OK) return rc;
  for (int i = 0; i < n_scenes; ++i)
    suffix_max = std::max<long long>(
        suffix_max, (long long)(h_scenes[i].n_keys + 1) * (h_scenes[i].max_ps + 1) + 2ll * h_scenes[i].max_ps);
  const gapro_eval_ap_scene& last = h_scenes[n_scenes - 1];
  rows.n_keys = last.key_offset + last.n_keys;
  rows.n_ids = last.id_offset + last.max_ps;
  rows.n_cells = last.pair_offset + (long long)(last.n_keys + 1) * (last.max_ps + 1);
  rows.first = (unsigned long long*)((char*)d_workspace + rows_at);
  hipStream_t stream = (hipStream_t)stream_;
  GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(d_scenes, h_scenes, (size_t)n_scenes * sizeof(gapro_eval_ap_scene),
                                      hipMemcpyHostToDevice, stream));
  GAPRO_HIP_CHECK(ctx, hipMemsetAsync(d_status, 0, (size_t)n_scenes * sizeof(int32_t), stream));
  GAPRO_HIP_CHECK(ctx, hipMemsetAsync(d_pair, 0, (size_t)B * rows.n_cells * sizeof(int32_t), stream));
  GAPRO_HIP_CHECK(ctx, hipMemsetAsync(d_ps_sum, 0, (size_t)B * rows.n_ids * sizeof(int64_t), stream));
  if (K > 0)  // kFirstNone in every byte; row 0's first points are gapro_eval_ap_keys'
    GAPRO_HIP_CHECK(ctx, hipMemsetAsync(rows.first, 0xff, (size_t)K * rows.n_ids * sizeof(unsigned long long), stream));
  if (n_max > 0)
    with_label_type(sem_gt_dtype, [&](auto sgt) {
      with_label_type(inst_gt_dtype, [&](auto igt) {
        with_ps_type(sem_ps_dtype, [&](auto sps) {
          with_ps_type(inst_ps_dtype, [&](auto ips) {
            using TGS = std::remove_const_t<std::remove_pointer_t<decltype(sgt)>>;
            using TGI = std::remove_const_t<std::remove_pointer_t<decltype(igt)>>;
            using TPS = std::remove_const_t<std::remove_pointer_t<decltype(sps)>>;
            using TPI = std::remove_const_t<std::remove_pointer_t<decltype(ips)>>;
            hipLaunchKernelGGL((k_ap_tally<TGS, TGI, TPS, TPI>), dim3(grid_for(n_max, 8, 128), n_scenes),
                               dim3(kThreads), 0, stream, d_scenes, (const TGS*)d_sem_gt, (const TGI*)d_inst_gt,
                               (const TPS*)d_sem_ps, (const TPI*)d_inst_ps, d_prob, rows, (int)(scannet_remap != 0),
                               d_workspace, (int*)d_pair, (long long*)d_ps_sum, (int*)d_status);
          });
        });
      });
    });
  if (K > 0 && n_max > 0)
    hipLaunchKernelGGL(k_ap_suffix, dim3(grid_for(suffix_max, 4, 256), n_scenes), dim3(kThreads), 0, stream, d_scenes,
                       d_workspace, rows, (int*)d_pair, (long long*)d_ps_sum);
  hipLaunchKernelGGL(k_ap_finalize, dim3(grid_for(fin_max, 1, 64), n_scenes, B), dim3(kThreads), 0, stream, d_scenes,
                     d_workspace, rows, (const int*)d_pair, (int*)d_key_code, (int*)d_key_n, (int*)d_ps_n,
                     (int*)d_ps_label, (int*)d_ps_void);
  GAPRO_LAUNCH_CHECK(ctx);
  return GAPRO_OK;
}

int gapro_eval_ap_tables_rows(gapro_ctx* ctx, void* stream, int32_t n_scenes, const gapro_eval_ap_scene* h_scenes,
                              gapro_eval_ap_scene* d_scenes, int64_t n_total_points, int32_t sem_gt_dtype,
                              const void* d_sem_gt, int32_t inst_gt_dtype, const void* d_inst_gt, int32_t sem_ps_dtype,
                              const void* d_sem_ps, int32_t inst_ps_dtype, const void* d_inst_ps, const float* d_prob,
                              int32_t n_thresholds, const float* h_thresholds, int32_t scannet_remap, void* d_workspace,
                              size_t workspace_bytes, int32_t* d_key_code, int32_t* d_key_n, int32_t* d_ps_n,
                              int32_t* d_ps_label, int32_t* d_ps_void, int64_t* d_ps_sum, int32_t* d_pair,
                              int32_t* d_status) {
  return ap_tables_rows("gapro_eval_ap_tables_rows", ctx, stream, n_scenes, h_scenes, d_scenes, n_total_points,
                        sem_gt_dtype, d_sem_gt, inst_gt_dtype, d_inst_gt, sem_ps_dtype, d_sem_ps, inst_ps_dtype, d_inst_ps,
                        d_prob, n_thresholds, h_thresholds, scannet_remap, d_workspace, workspace_bytes, d_key_code,
                        d_key_n, d_ps_n, d_ps_label, d_ps_void, d_ps_sum, d_pair, d_status);
}

int gapro_eval_ap_tables(gapro_ctx* ctx, void* stream, int32_t n_scenes, const gapro_eval_ap_scene* h_scenes,
                         gapro_eval_ap_scene* d_scenes, int64_t n_total_points, int32_t sem_gt_dtype,
                         const void* d_sem_gt, int32_t inst_gt_dtype, const void* d_inst_gt, int32_t sem_ps_dtype,
                         const void* d_sem_ps, int32_t inst_ps_dtype, const void* d_inst_ps, const float* d_prob,
                         int32_t scannet_remap, void* d_workspace, size_t workspace_bytes, int32_t* d_key_code,
                         int32_t* d_key_n, int32_t* d_ps_n, int32_t* d_ps_label, int32_t* d_ps_void,
                         int64_t* d_ps_sum, int32_t* d_pair, int32_t* d_status) {
  return ap_tables_rows("gapro_eval_ap_tables", ctx, stream, n_scenes, h_scenes, d_scenes, n_total_points, sem_gt_dtype,
                        d_sem_gt, inst_gt_dtype, d_inst_gt, sem_ps_dtype, d_sem_ps, inst_ps_dtype, d_inst_ps, d_prob, 0,
                        nullptr, scannet_remap, d_workspace, workspace_bytes, d_key_code, d_key_n, d_ps_n, d_ps_label,
                        d_ps_void, d_ps_sum, d_pair, d_status);
}

}  // extern "C"
