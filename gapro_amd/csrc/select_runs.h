// What the two predicted-instance chains share (proposals.hip: ISBNet's; spf_predict.hip: SPFormer's; DESIGN.md 4.8 and
// 4.12): the float64 softmax of a row of class logits, the order of (score, lowest index first) as one integer key, the
// radix select and sort of the largest keys in LDS, and the chunked run lengths of a row of point bits.  Device and host
// inline code only.  A chain supplies its point bit m(k, .) as a callable and the cells of its row: the kernels, the
// workspaces and the row indexing stay in the two files.  Every function that is said to be called by the whole
// workgroup (or wave) holds barriers (or shuffles): the returns in front of such a call must be uniform over it.
#pragma once
#include "common.h"
#include "scan.h"
#include "wave_reduce.h"

#include <cmath>

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kGridCap = GAPRO_PROPOSALS_GRID_CAP;
constexpr int kMaxTopk = GAPRO_PROPOSALS_MAX_PRE_TOPK;  // also the length of the sorts in LDS: a power of two
constexpr int kMaxChunks = 1024;  // chunks of points of a row (`trans`, `runs`)
constexpr int kMinChunk = 1024;   // points of a chunk, at least
constexpr long long kMaxIndex = 0x7fffffffLL;
constexpr long long kMaxScores = 1LL << 20;
static_assert((kMaxTopk & (kMaxTopk - 1)) == 0 && kMaxTopk % kThreads == 0, "the LDS sorts need a power of two");

// ---- the class scores ----------------------------------------------------------------------------------------------
// softmax of row[0, C] in float64: the maximum, the sum of exp(x - max) in ascending column, and whether all are finite
struct RowSoftmax {
  double mx, den;
  bool ok;
  // softmax(row)[c] * factor for x = row[c]
  __device__ double times(float x, double factor) const { return exp((double)x - mx) / den * factor; }
};
__device__ inline RowSoftmax row_softmax(const float* __restrict__ row, int C) {
  RowSoftmax s{-INFINITY, 0.0, true};
  for (int c = 0; c <= C; ++c) {
    s.ok = s.ok && isfinite(row[c]);
    s.mx = fmax(s.mx, (double)row[c]);
  }
  for (int c = 0; c <= C; ++c) s.den += exp((double)row[c] - s.mx);
  return s;
}

// ---- keys, select and sort -------------------------------------------------------------------------------------------
// float32 as an unsigned integer of the same order (-0.0 below +0.0; the scores are never -0.0), and back
__device__ inline unsigned order_bits(float f) {
  const unsigned b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ inline unsigned order_bits_inv(unsigned u) { return (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u; }
// larger value first, then the lower index: the larger key
__device__ inline unsigned long long sort_key(float value, unsigned index) {
  return ((unsigned long long)order_bits(value) << 32) | (unsigned long long)(0xffffffffu - index);
}
__device__ inline unsigned key_index(unsigned long long key) { return 0xffffffffu - (unsigned)(key & 0xffffffffull); }

// Bitonic sort of s[0, kMaxTopk) in LDS, descending; the whole workgroup calls.
__device__ inline void sort_desc(unsigned long long* s) {
  for (int k = 2; k <= kMaxTopk; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int i = threadIdx.x; i < kMaxTopk; i += kThreads) {
        const int l = i ^ j;
        if (l > i) {
          const unsigned long long a = s[i], b = s[l];
          const bool desc = (i & k) == 0;
          if (desc ? a < b : a > b) {
            s[i] = b;
            s[l] = a;
          }
        }
      }
    }
  __syncthreads();
}

// The whole workgroup (the only one of its grid) calls: the keys of the K <= kMaxTopk largest of score[0, n), sorted, in
// s_key[0, K) (LDS, kMaxTopk long; zeros behind them).  The key of entry i is (score, lowest index first); the keys are
// distinct, so the K-th largest is found by eight passes of an 8-bit radix select, the K keys at or above it are gathered
// and sorted.
__device__ inline void select_topk(const float* __restrict__ score, unsigned n, int K, unsigned long long* s_key) {
  __shared__ unsigned s_hist[256], s_group[16];
  __shared__ unsigned long long s_prefix;
  __shared__ unsigned s_need, s_n;
  const int t = threadIdx.x;
  if (t == 0) {
    s_prefix = 0ull;
    s_need = (unsigned)K;
    s_n = 0u;
  }
  for (int shift = 56; shift >= 0; shift -= 8) {
    s_hist[t] = 0u;
    __syncthreads();
    const unsigned long long prefix = s_prefix, high = shift == 56 ? 0ull : ~0ull << (shift + 8);
    for (unsigned i = t; i < n; i += kThreads) {
      const unsigned long long key = sort_key(score[i], i);
      if (((key ^ prefix) & high) == 0ull) atomicAdd(&s_hist[(unsigned)(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (t < 16) {  // the buckets in sixteen groups, so that the walk below reads 32 counters, not 256
      unsigned g = 0u;
      for (int b = 0; b < 16; ++b) g += s_hist[16 * t + b];
      s_group[t] = g;
    }
    __syncthreads();
    if (t == 0) {
      unsigned need = s_need, above = 0u;
      int g = 15;
      for (; g > 0 && above + s_group[g] < need; --g) above += s_group[g];
      int b = 16 * g + 15;
      for (; b > 16 * g && above + s_hist[b] < need; --b) above += s_hist[b];
      s_need = need - above;
      s_prefix = prefix | ((unsigned long long)b << shift);
    }
    __syncthreads();
  }
  const unsigned long long kth = s_prefix;
  for (int i = t; i < kMaxTopk; i += kThreads) s_key[i] = 0ull;
  __syncthreads();
  for (unsigned i = t; i < n; i += kThreads) {
    const unsigned long long key = sort_key(score[i], i);
    if (key >= kth) {
      const unsigned at = atomicAdd(&s_n, 1u);
      if (at < (unsigned)kMaxTopk) s_key[at] = key;
    }
  }
  sort_desc(s_key);
}

// The whole workgroup calls, s[kThreads] in LDS: the sum of `v` over the threads below this one; *total: over all.
template <typename T>
__device__ inline T block_sum_before(T* s, T v, T* total) {
  s[threadIdx.x] = v;
  __syncthreads();
  T before = 0, all = 0;
  for (int j = 0; j < kThreads; ++j) {
    before += j < (int)threadIdx.x ? s[j] : 0;
    all += s[j];
  }
  *total = all;
  return before;
}

// ---- the run lengths of a row --------------------------------------------------------------------------------------
// The positions [0, N] of a row are cut into `nchunks` chunks of `chunk_len`; workgroup blockIdx.x of a row has chunk
// blockIdx.x.  `bit(p)` is the row's m(k, p): 0 outside [0, N).  A transition at p is bit(p) != bit(p - 1).
inline void chunking(long long N, int* nchunks, long long* chunk_len) {
  long long nc = (N + 1 + kMinChunk - 1) / kMinChunk;
  *nchunks = (int)(nc > kMaxChunks ? kMaxChunks : nc);
  *chunk_len = (N + 1 + *nchunks - 1) / *nchunks;
}

struct ChunkTally {
  unsigned trans, ones;
};

// The whole workgroup calls; no atomics.  In thread 0: the transitions and the set bits of this workgroup's chunk.
template <typename Bit>
__device__ inline ChunkTally chunk_tally(long long chunk_len, long long N, Bit bit) {
  __shared__ unsigned s_trans[kWaves], s_ones[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long p0 = (long long)blockIdx.x * chunk_len, p1 = min(p0 + chunk_len, N + 1);
  ChunkTally c{0u, 0u};
  for (long long b0 = p0; b0 < p1; b0 += kThreads) {  // uniform over the workgroup
    const long long p = b0 + threadIdx.x;
    const int cur = p < p1 ? bit(p) : 0;
    int prev = __shfl_up(cur, 1, 64);
    if (lane == 0) prev = bit(p - 1);
    if (p < p1) {
      c.trans += cur != prev;
      c.ones += cur;
    }
  }
  c.trans = wave_sum(c.trans);
  c.ones = wave_sum(c.ones);
  if (lane == 0) {
    s_trans[wave] = c.trans;
    s_ones[wave] = c.ones;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int j = 1; j < kWaves; ++j) {
      c.trans += s_trans[j];
      c.ones += s_ones[j];
    }
  return c;
}

// A wave calls with the chunk counts c[0, nchunks) of a row: they become the counts before the chunk (a shuffle scan over
// 64 chunks at a time).  Returns the row's count.
__device__ inline unsigned scan_chunks(unsigned* c, int nchunks) {
  const int lane = threadIdx.x & 63;
  unsigned before = 0u;
  for (int j0 = 0; j0 < nchunks; j0 += 64) {  // uniform over the wave
    const int j = j0 + lane;
    const unsigned x = j < nchunks ? c[j] : 0u;
    const unsigned inc = wave_inclusive(x);
    if (j < nchunks) c[j] = before + inc - x;
    before += __shfl(inc, 63, 64);
  }
  return before;
}

// status, n_rows and total_trans of a chain's scalars against what the caller of `fill` has room for
template <typename Scalars>
__device__ inline bool fill_ok(const Scalars& s, long long cap_rows, long long cap_runs) {
  return s.status == GAPRO_OK && s.n_rows <= cap_rows && s.total_trans <= 2 * cap_runs;
}

// The whole workgroup calls: the positions of the transitions of its chunk, 1-based and in order, go to runs[at, ...),
// where `at` counts the row's transitions before the chunk and those of the rows before it; the chunk's bits go to
// mask_row[0, N), if there is one.
template <typename Bit>
__device__ inline void emit_runs(long long chunk_len, long long N, Bit bit, long long at, long long* __restrict__ runs,
                                 unsigned char* __restrict__ mask_row) {
  __shared__ unsigned s_wave[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long p0 = (long long)blockIdx.x * chunk_len, p1 = min(p0 + chunk_len, N + 1);
  for (long long b0 = p0; b0 < p1; b0 += kThreads) {  // uniform over the workgroup
    const long long p = b0 + threadIdx.x;
    const int cur = p < p1 ? bit(p) : 0;
    int prev = __shfl_up(cur, 1, 64);
    if (lane == 0) prev = bit(p - 1);
    const bool tr = p < p1 && cur != prev;
    const unsigned long long b = __ballot(tr);
    if (lane == 0) s_wave[wave] = (unsigned)__popcll(b);
    __syncthreads();
    unsigned before = 0u, total = 0u;
    for (int j = 0; j < kWaves; ++j) {
      before += j < wave ? s_wave[j] : 0u;
      total += s_wave[j];
    }
    if (tr && runs) runs[at + before + __popcll(b & ((1ull << lane) - 1ull))] = p + 1;
    if (mask_row && p < p1 && p < N) mask_row[p] = (unsigned char)cur;
    at += total;
    __syncthreads();  // s_wave is written again
  }
}

// every second value of a row is the end of a run: it becomes the length.  The rows hold whole pairs.
__device__ inline void ends_to_lengths(long long* __restrict__ runs, long long n_runs) {
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n_runs; i += stride)
    runs[2 * i + 1] -= runs[2 * i];
}
