// Ground-truth instance masks per batch sample (include/gapro_hip.h, "Ground-truth instance masks"): ISBNet's get_spp_gt
// (isbnet/model/model_utils.py:692-738) and get_subsample_gt (:647-689) without their loops over the samples and the ids.
// gapro_spp_gt_count:
//   init       clears the per-sample presence bit-words (instance ids, superpoint ids), checks the offsets
//   mark       one pass over the points: sample by bisection of the offsets, the two bits, the refusals; the instance
//              words are few and hit by every point, so the workgroups spread over copies of them (GtDims::reps)
//   rank       a workgroup per sample and table: ORs the copies, drops the ignored classes, prefix popcounts over the
//              words, the count
//   pack       one workgroup: packed offsets of the samples, the totals, the status, the header
// gapro_spp_gt_fill:
//   clear      the mask buffer (read as uint32: it is the table of the counts c) and the table of n
//   tally      one pass over the points: n(s) and c(i, s), the lanes of a wave that share a cell combined first
//   threshold  one pass over the cells: the count becomes 1.0f or 0.0f by the integer rule, in place
//   gather     cls, box and ids by rank
// Without superpoints (every point its own column) clear / scatter replace clear / tally / threshold.
// Integer atomics only, so every result is the same bits for every grid and every run.  No workgroup waits for another:
// the kernel boundaries on the stream are the only ordering.  A refusal is a status word written by `pack`: every kernel
// of the fill returns at once and no output is touched.
#include "common.h"
#include "label_types.h"
#include "launch_util.h"
#include "wave_reduce.h"

#include <cstdint>
#include <type_traits>

namespace {

constexpr int kThreads = 256;
constexpr int kGridCap = GAPRO_SPP_GT_GRID_CAP;  // workgroups of the passes over the points
constexpr int kLeaderRounds = 4;                 // distinct cells of a wave combined by a leader before the rest add alone
constexpr int kReplicaWords = 16384, kMaxReplicas = 64;  // copies of a bit-word table `mark` spreads over (GtDims)
constexpr long long kMaxPoints = 0x7fffffffLL;
constexpr int kNoSample = 0x7fffffff;

enum { kFlagOffsets = 1, kFlagGather = 2, kFlagLabel = 4, kFlagSpp = 8, kNumFlags = 4 };

struct GtScalars {  // the first 64 bytes of the workspace
  int flags;
  int status;  // set by k_gt_pack
  int bad_sample[kNumFlags];
  long long total_rows, total_cols, total_cells;
  int reserved[4];
};
static_assert(sizeof(GtScalars) == 64, "GtScalars is the first 64 bytes of the workspace");

struct GtDims {
  long long n;  // points of the pass
  int B, I, S;
  __host__ __device__ int wi() const { return (I + 31) >> 5; }  // bit-words of a sample's instance ids
  __host__ __device__ int ws() const { return (S + 31) >> 5; }  // ... of its superpoint ids
  // The bit-words of a batch are few (40 instance ids a sample: two words; 1500 superpoint ids: two cache lines) and
  // every point of the batch hits them, from every workgroup at once: same-line atomics from all over the chip, which
  // run one after the other.  `mark` spreads its workgroups over copies of each table, every copy on cache lines of its
  // own, and `rank` ORs the copies into the first.  A table too large for that to matter has one copy.
  __host__ __device__ static int copy_stride(int words) { return (words + 31) & ~31; }  // whole 128-byte lines
  __host__ __device__ static int copies(int words) {
    const int r = words > 0 ? kReplicaWords / words : 1;
    return r < 1 ? 1 : (r > kMaxReplicas ? kMaxReplicas : r);
  }
  __host__ __device__ int inst_stride() const { return copy_stride(B * wi()); }
  __host__ __device__ int inst_copies() const { return copies(B * wi()); }
  __host__ __device__ int spp_stride() const { return copy_stride(B * ws()); }
  __host__ __device__ int spp_copies() const { return copies(B * ws()); }
};

struct GtWs {
  GtScalars* s;
  long long* row_off;   // [B + 1] first row of a sample in cls / box / ids
  long long* col_off;   // [B + 1] first column of a sample in the table of n
  long long* mask_off;  // [B + 1] first cell of a sample in the mask
  int* n_inst;          // [B]
  int* n_spp;           // [B]
  unsigned* inst_bits;  // [inst_copies][inst_stride]; the first copy is [B][wi]: id present and, after `rank`, kept
  unsigned* spp_bits;   // [spp_copies][spp_stride]; the first copy is [B][ws]
  int* inst_pre;        // [B][wi] set bits of the sample's words before this one
  int* spp_pre;         // [B][ws]
  unsigned* ntab;       // [n] points per column (superpoint mode)
};

__host__ __device__ inline size_t gt_ws(void* base, const GtDims& d, GtWs* w) {
  char* p = (char*)base;
  const size_t B = (size_t)d.B, nwi = B * (size_t)d.wi(), nws = B * (size_t)d.ws();
  w->s = (GtScalars*)p; p += sizeof(GtScalars);
  w->row_off = (long long*)p; p += (B + 1) * 8;
  w->col_off = (long long*)p; p += (B + 1) * 8;
  w->mask_off = (long long*)p; p += (B + 1) * 8;
  w->n_inst = (int*)p; p += B * 4;
  w->n_spp = (int*)p; p += B * 4;
  w->inst_bits = (unsigned*)p; p += (size_t)d.inst_copies() * d.inst_stride() * 4;
  w->spp_bits = (unsigned*)p; p += (size_t)d.spp_copies() * d.spp_stride() * 4;
  w->inst_pre = (int*)p; p += nwi * 4;
  w->spp_pre = (int*)p; p += nws * 4;
  w->ntab = (unsigned*)p; p += (d.S > 0 ? (size_t)d.n : 0) * 4;
  return (size_t)(p - (char*)base);
}

struct GtIn {  // the inputs both calls take
  const void* labels;
  const long long* gather;
  const void* spps;
  int spp_is_i64;
  const void* cls;
  int cls_type;
  const long long* offsets;
  long long n_labels, ignore;
};

// The instance id of a label: [0, I); -1 for ignore_label; -2 for a label the reference would index instance_cls from the
// end with or fail on (negative, >= I, a float64 that is no integer).
template <class T>
__device__ inline int inst_id(T v, long long ignore, int I) {
  if ((long long)v == ignore) return -1;
  if (v < 0 || v >= (T)I) return -2;
  return (int)v;
}
template <>
__device__ inline int inst_id<double>(double v, long long ignore, int I) {
  if (v == (double)ignore) return -1;
  if (!(v >= 0.0) || v >= (double)I) return -2;
  const int id = (int)v;
  return (double)id == v ? id : -2;
}

__device__ inline bool cls_kept(const void* cls, int type, int id) {  // instance_cls[id] >= 0
  if (type == GAPRO_LABEL_I32) return ((const int*)cls)[id] >= 0;
  if (type == GAPRO_LABEL_I64) return ((const long long*)cls)[id] >= 0;
  return ((const double*)cls)[id] >= 0.0;
}

// The sample of point p: the last b with offsets[b] <= p.  Inside [0, B) for any offsets; -1 for a point outside
// [offsets[0], offsets[B]).
__device__ inline int sample_of(const long long* __restrict__ off, int B, long long p) {
  if (p < off[0] || p >= off[B]) return -1;
  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= p) lo = mid;
    else hi = mid;
  }
  return lo;
}

__device__ inline unsigned peek(const unsigned* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Sets `bit` of bits[w] for every lane with w >= 0 (bits only ever gain bits, so a word that already holds the bit needs
// no atomic).  The lanes of a wave that all hit one word send one atomic.  Otherwise -- the ids of a sample share a few
// words, and every wave of the grid finds them empty at once -- the first lane of each of the first kLeaderRounds
// distinct (word, bit) pairs sends its pair once, what is left goes alone.  Every lane of the wave calls.
__device__ inline void or_bits(unsigned* bits, long long w, unsigned bit, int lane) {
  const bool on = w >= 0;
  const unsigned long long act = __ballot(on);
  if (act == 0ull) return;  // uniform over the wave
  const int first = __ffsll((long long)act) - 1;
  const long long lead = __shfl(w, first, 64);
  if (__ballot(on && w != lead) == 0ull) {
    const unsigned v = (unsigned)wave_or((int)(on ? bit : 0u));
    if (lane == first && (peek(&bits[lead]) & v) != v) atomicOr(&bits[lead], v);
    return;
  }
  const long long key = on ? w * 32 + (__ffs((int)bit) - 1) : -1;
  unsigned long long rest = act;
  bool mine = false;  // this lane sends its pair
  for (int round = 0; rest != 0ull && round < kLeaderRounds; ++round) {  // uniform over the wave
    const int l = __ffsll((long long)rest) - 1;
    const unsigned long long same = __ballot(key == __shfl(key, l, 64));
    mine = mine || lane == l;
    rest &= ~same;
  }
  mine = mine || ((rest >> lane) & 1ull);
  if (mine && !(peek(&bits[w]) & bit)) atomicOr(&bits[w], bit);
}

// tab[key] += 1 for every lane with key >= 0.  Superpoints are runs of like-labelled neighbours, so most waves hold one or
// two distinct keys: the first lane of each of the first kLeaderRounds distinct keys adds the count of its lanes, what is
// left adds alone.  Every lane of the wave calls.
__device__ inline void add_by_key(unsigned* tab, long long key, int lane) {
  unsigned long long rest = __ballot(key >= 0);
  for (int round = 0; rest != 0ull && round < kLeaderRounds; ++round) {  // uniform over the wave
    const int lead = __ffsll((long long)rest) - 1;
    const long long k = __shfl(key, lead, 64);
    const unsigned long long same = __ballot(key == k);
    if (lane == lead) atomicAdd(&tab[k], (unsigned)__popcll(same));
    rest &= ~same;
  }
  if ((rest >> lane) & 1ull) atomicAdd(&tab[key], 1u);
}

__device__ inline int rank_of(const unsigned* bits, const int* pre, size_t word, int id) {
  return pre[word] + __popc(bits[word] & ((1u << (id & 31)) - 1u));
}

__global__ __launch_bounds__(kThreads) void k_gt_init(void* base, GtDims d, const long long* __restrict__ off) {
  GtWs w;
  gt_ws(base, d, &w);
  const size_t nwi = (size_t)d.inst_copies() * d.inst_stride(), nws = (size_t)d.spp_copies() * d.spp_stride();
  const size_t stride = (size_t)gridDim.x * kThreads;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < nwi + nws; i += stride) {
    if (i < nwi) w.inst_bits[i] = 0u;
    else w.spp_bits[i - nwi] = 0u;
  }
  if (blockIdx.x != 0) return;
  // the offsets: B <= GAPRO_SPP_GT_MAX_SAMPLES, one workgroup
  __shared__ int s_bad[kThreads];
  int bad = kNoSample;
  for (int b = threadIdx.x; b <= d.B; b += kThreads) {
    const long long o = off[b];
    if (o < 0 || o > d.n || (b < d.B && off[b + 1] < o)) bad = min(bad, min(b, d.B - 1));
  }
  s_bad[threadIdx.x] = bad;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int j = 1; j < kThreads; ++j) bad = min(bad, s_bad[j]);
    w.s->flags = bad != kNoSample ? kFlagOffsets : 0;
    for (int k = 0; k < kNumFlags; ++k) w.s->bad_sample[k] = kNoSample;
    if (bad != kNoSample) w.s->bad_sample[0] = bad;
  }
}

// The loop is uniform over the workgroup: every lane of a wave reaches the ballots.
template <class LabelT>
__global__ __launch_bounds__(kThreads) void k_gt_mark(void* base, GtDims d, GtIn in) {
  GtWs w;
  gt_ws(base, d, &w);
  if (w.s->flags & kFlagOffsets) return;  // written by k_gt_init: the samples are not defined
  const LabelT* __restrict__ labels = (const LabelT*)in.labels;
  const int lane = threadIdx.x & 63, wi = d.wi(), ws = d.ws();
  unsigned* inst_copy = w.inst_bits + (size_t)(blockIdx.x % d.inst_copies()) * d.inst_stride();
  unsigned* spp_copy = w.spp_bits + (size_t)(blockIdx.x % d.spp_copies()) * d.spp_stride();
  const long long stride = (long long)gridDim.x * kThreads;
  int flags = 0, bad[kNumFlags];
  for (int k = 0; k < kNumFlags; ++k) bad[k] = kNoSample;
  for (long long b0 = (long long)blockIdx.x * kThreads; b0 < d.n; b0 += stride) {
    const long long p = b0 + threadIdx.x;
    long long iw = -1, sw = -1;
    unsigned ibit = 0u, sbit = 0u;
    const int b = p < d.n ? sample_of(in.offsets, d.B, p) : -1;
    if (b >= 0) {
      const long long src = in.gather ? in.gather[p] : p;
      if (src < 0 || src >= in.n_labels) {
        flags |= kFlagGather;
        bad[1] = min(bad[1], b);
      } else {
        const int id = inst_id(labels[src], in.ignore, d.I);
        if (id == -2) {
          flags |= kFlagLabel;
          bad[2] = min(bad[2], b);
        } else if (id >= 0) {
          iw = (long long)b * wi + (id >> 5);
          ibit = 1u << (id & 31);
        }
        if (in.spps) {
          const long long s = idx_at(in.spps, in.spp_is_i64, src);
          if (s < 0 || s >= d.S) {
            flags |= kFlagSpp;
            bad[3] = min(bad[3], b);
          } else {
            sw = (long long)b * ws + (s >> 5);
            sbit = 1u << (s & 31);
          }
        }
      }
    }
    or_bits(inst_copy, iw, ibit, lane);
    or_bits(spp_copy, sw, sbit, lane);
  }
  flags = wave_or(flags);
  if (flags == 0) return;  // uniform over the wave
  for (int k = 1; k < kNumFlags; ++k) {
    if (!(flags & (1 << k))) continue;
    const int m = wave_min(bad[k]);
    if (lane == 0) atomicMin(&w.s->bad_sample[k], m);
  }
  if (lane == 0) atomicOr(&w.s->flags, flags);
}

// Two workgroups per sample, one for its instance words (blockIdx.y == 0) and one for its superpoint words: they share
// nothing.  First the copies of the sample's words are ORed into the first copy, one thread per word.  Then thread t owns
// a run of words: it drops the instance bits whose class is negative, counts, and writes the prefix popcounts of its run
// behind the counts of the threads before it.
__global__ __launch_bounds__(kThreads) void k_gt_rank(void* base, GtDims d, GtIn in) {
  GtWs w;
  gt_ws(base, d, &w);
  __shared__ int s_cnt[kThreads];
  const int b = blockIdx.x, t = threadIdx.x;
  const bool inst = blockIdx.y == 0;
  const int words = inst ? d.wi() : d.ws();
  const int copies = inst ? d.inst_copies() : d.spp_copies();
  const size_t copy_stride = inst ? d.inst_stride() : d.spp_stride();
  unsigned* bits = (inst ? w.inst_bits : w.spp_bits) + (size_t)b * words;
  int* pre = (inst ? w.inst_pre : w.spp_pre) + (size_t)b * words;
  if (copies > 1) {  // uniform over the workgroup
    for (int j = t; j < words; j += kThreads) {
      unsigned word = 0u;
#pragma unroll
      for (int r = 0; r < kMaxReplicas; ++r)  // no branch: every load in flight at once (beyond `copies`: the first again)
        word |= bits[(r < copies ? r : 0) * copy_stride + j];
      bits[j] = word;
    }
    __syncthreads();  // the runs below read words other threads merged
  }
  const int per = (words + kThreads - 1) / kThreads;
  const int w0 = min(words, t * per), w1 = min(words, w0 + per);
  int c = 0;
  for (int j = w0; j < w1; ++j) {
    unsigned word = bits[j];
    if (inst) {
      for (unsigned m = word; m != 0u; m &= m - 1u) {
        const int bit = __ffs((int)m) - 1;
        if (!cls_kept(in.cls, in.cls_type, j * 32 + bit)) word &= ~(1u << bit);
      }
      bits[j] = word;
    }
    c += __popc(word);
  }
  s_cnt[t] = c;
  __syncthreads();
  int before = 0, total = 0;
  for (int j = 0; j < kThreads; ++j) {
    before += j < t ? s_cnt[j] : 0;
    total += s_cnt[j];
  }
  for (int j = w0; j < w1; ++j) {
    pre[j] = before;
    before += __popc(bits[j]);
  }
  if (t == 0) {
    if (inst) w.n_inst[b] = total;
    else w.n_spp[b] = d.S > 0 ? total : (int)(in.offsets[b + 1] - in.offsets[b]);  // n <= 2^31 - 1
  }
}

// One workgroup; B <= GAPRO_SPP_GT_MAX_SAMPLES, so one thread walks the samples.
__global__ __launch_bounds__(kThreads) void k_gt_pack(void* base, GtDims d, gapro_spp_gt_header* __restrict__ header) {
  GtWs w;
  gt_ws(base, d, &w);
  if (threadIdx.x != 0) return;
  const int flags = w.s->flags;
  int status = GAPRO_OK, bad = -1;
  for (int k = 0; k < kNumFlags; ++k)
    if (flags & (1 << k)) {
      status = k == 3 ? GAPRO_ERR_SPP_RANGE : GAPRO_ERR_BAD_ARG;
      bad = w.s->bad_sample[k];
      break;
    }
  int* counts = (int*)(header + 1);
  long long rows = 0, cols = 0, cells = 0;
  for (int b = 0; b < d.B; ++b) {
    const int ni = status == GAPRO_OK ? w.n_inst[b] : 0, ns = status == GAPRO_OK ? w.n_spp[b] : 0;
    w.row_off[b] = rows;
    w.col_off[b] = cols;
    w.mask_off[b] = cells;
    counts[2 * b] = ni;
    counts[2 * b + 1] = ns;
    rows += ni;
    cols += ns;
    cells += (long long)ni * ns;
  }
  w.row_off[d.B] = rows;
  w.col_off[d.B] = cols;
  w.mask_off[d.B] = cells;
  w.s->status = status;
  w.s->total_rows = rows;
  w.s->total_cols = cols;
  w.s->total_cells = cells;
  header->status = status;
  header->bad_sample = bad;
  header->flags = flags;
  header->batch_size = d.B;
  header->total_rows = rows;
  header->total_cols = cols;
  header->total_cells = cells;
}

// ---- fill --------------------------------------------------------------------------------------------------------
__device__ inline bool fill_ok(const GtWs& w, long long mask_cells, long long n_rows) {
  return w.s->status == GAPRO_OK && w.s->total_cells <= mask_cells && w.s->total_rows <= n_rows;
}

__global__ __launch_bounds__(kThreads) void k_gt_clear(void* base, GtDims d, unsigned* __restrict__ mask,
                                                       long long mask_cells, long long n_rows,
                                                       gapro_spp_gt_header* __restrict__ header) {
  GtWs w;
  gt_ws(base, d, &w);
  if (!fill_ok(w, mask_cells, n_rows)) {
    if (header && blockIdx.x == 0 && threadIdx.x == 0 && w.s->status == GAPRO_OK) header->status = GAPRO_ERR_WORKSPACE;
    return;
  }
  const long long cells = w.s->total_cells, cols = d.S > 0 ? w.s->total_cols : 0;
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < cells + cols; i += stride) {
    if (i < cells) mask[i] = 0u;
    else w.ntab[i - cells] = 0u;
  }
}

// The cell of point p's label in its sample's mask (-1: no row), and with kCol the column's entry of the table of n.
template <class LabelT>
__device__ inline long long cell_of(const GtWs& w, const GtDims& d, const GtIn& in, long long p, long long* col_key) {
  *col_key = -1;
  const int b = p < d.n ? sample_of(in.offsets, d.B, p) : -1;
  if (b < 0) return -1;
  const long long src = in.gather ? in.gather[p] : p;
  long long col;
  if (in.spps) {
    const long long s = idx_at(in.spps, in.spp_is_i64, src);
    col = rank_of(w.spp_bits, w.spp_pre, (size_t)b * d.ws() + (size_t)(s >> 5), (int)s);
    *col_key = w.col_off[b] + col;
  } else {
    col = p - in.offsets[b];
  }
  const int id = inst_id(((const LabelT*)in.labels)[src], in.ignore, d.I);
  if (id < 0) return -1;
  const size_t word = (size_t)b * d.wi() + (size_t)(id >> 5);
  if (!((w.inst_bits[word] >> (id & 31)) & 1u)) return -1;  // a class < 0
  return w.mask_off[b] + (long long)rank_of(w.inst_bits, w.inst_pre, word, id) * w.n_spp[b] + col;
}

// The loop is uniform over the workgroup: every lane of a wave reaches the ballots.
template <class LabelT>
__global__ __launch_bounds__(kThreads) void k_gt_tally(void* base, GtDims d, GtIn in, unsigned* __restrict__ mask,
                                                       long long mask_cells, long long n_rows) {
  GtWs w;
  gt_ws(base, d, &w);
  if (!fill_ok(w, mask_cells, n_rows)) return;
  const int lane = threadIdx.x & 63;
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long b0 = (long long)blockIdx.x * kThreads; b0 < d.n; b0 += stride) {
    long long col_key;
    const long long cell = cell_of<LabelT>(w, d, in, b0 + threadIdx.x, &col_key);
    add_by_key(w.ntab, col_key, lane);
    add_by_key(mask, cell, lane);
  }
}

// 2 c >= n (2 c > n with `strict`), in place: the count becomes the float.
__global__ __launch_bounds__(kThreads) void k_gt_threshold(void* base, GtDims d, unsigned* __restrict__ mask,
                                                           long long mask_cells, long long n_rows, int strict) {
  GtWs w;
  gt_ws(base, d, &w);
  if (!fill_ok(w, mask_cells, n_rows)) return;
  const long long cells = w.s->total_cells;
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < cells; e += stride) {
    const int b = sample_of(w.mask_off, d.B, e);  // e < mask_off[B]: never -1
    const long long col = (e - w.mask_off[b]) % w.n_spp[b];
    const unsigned long long c2 = 2ull * mask[e], n = w.ntab[w.col_off[b] + col];
    mask[e] = __float_as_uint((strict ? c2 > n : c2 >= n) ? 1.0f : 0.0f);
  }
}

// Every point its own column: a one where the point's label has a row.
template <class LabelT>
__global__ __launch_bounds__(kThreads) void k_gt_scatter(void* base, GtDims d, GtIn in, float* __restrict__ mask,
                                                         long long mask_cells, long long n_rows) {
  GtWs w;
  gt_ws(base, d, &w);
  if (!fill_ok(w, mask_cells, n_rows)) return;
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < d.n; p += stride) {
    long long col_key;
    const long long cell = cell_of<LabelT>(w, d, in, p, &col_key);
    if (cell >= 0) mask[cell] = 1.0f;
  }
}

// One lane per bit of the instance bit-words: the row of a set bit.
__global__ __launch_bounds__(kThreads) void k_gt_gather(void* base, GtDims d, GtIn in, const unsigned* __restrict__ box_in,
                                                        long long mask_cells, long long n_rows, void* __restrict__ cls_out,
                                                        unsigned* __restrict__ box_out, long long* __restrict__ ids_out) {
  GtWs w;
  gt_ws(base, d, &w);
  if (!fill_ok(w, mask_cells, n_rows)) return;
  const int wi = d.wi();
  const size_t bits = (size_t)d.B * wi * 32, stride = (size_t)gridDim.x * kThreads;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < bits; i += stride) {
    const size_t word = i >> 5;
    const int bit = (int)(i & 31);
    const unsigned m = w.inst_bits[word];
    if (!((m >> bit) & 1u)) continue;
    const int b = (int)(word / wi), id = (int)(word % wi) * 32 + bit;
    const long long row = w.row_off[b] + w.inst_pre[word] + __popc(m & ((1u << bit) - 1u));
    if (ids_out) ids_out[row] = id;
    if (cls_out) {
      if (in.cls_type == GAPRO_LABEL_I32) ((unsigned*)cls_out)[row] = ((const unsigned*)in.cls)[id];
      else ((unsigned long long*)cls_out)[row] = ((const unsigned long long*)in.cls)[id];
    }
    if (box_out)
      for (int k = 0; k < 6; ++k) box_out[6 * row + k] = box_in[6 * (size_t)id + k];
  }
}

bool dims_ok(int64_t n, int32_t B, int32_t I, int32_t S) {
  return n >= 1 && n <= kMaxPoints && B >= 1 && B <= GAPRO_SPP_GT_MAX_SAMPLES && I >= 1 && I <= GAPRO_INST_PREP_MAX_IDS &&
         S >= 0 && (long long)B * S <= (long long)GAPRO_SPP_GT_MAX_BATCH_SPPS;
}

// what both calls refuse before anything is launched
int check_args(gapro_ctx* ctx, const char* who, int64_t n, int32_t label_type, const GtIn& in, const GtDims& d,
               const void* d_ws, size_t ws_bytes) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  bool ok = dims_ok(n, d.B, d.I, d.S) && in.labels && in.cls && in.offsets && d_ws;
  ok = ok && in.n_labels >= 1 && in.n_labels <= kMaxPoints && (in.gather || in.n_labels == n);
  ok = ok && (in.spps != nullptr) == (d.S > 0) && (in.spp_is_i64 == 0 || in.spp_is_i64 == 1);
  ok = ok && with_label_type(label_type, [](auto*) {}) && with_label_type(in.cls_type, [](auto*) {});
  if (!ok) return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: bad argument", who);
  if (ws_bytes < gapro_spp_gt_workspace_bytes(n, d.B, d.I, d.S))
    return gapro_fail(ctx, GAPRO_ERR_WORKSPACE, "%s: workspace too small", who);
  return GAPRO_OK;
}

}  // namespace

extern "C" {

size_t gapro_spp_gt_workspace_bytes(int64_t n_points, int32_t batch_size, int32_t n_cls, int32_t n_spps) {
  if (!dims_ok(n_points, batch_size, n_cls, n_spps)) return 0;
  GtWs w;
  return align_up(gt_ws(nullptr, GtDims{(long long)n_points, batch_size, n_cls, n_spps}, &w), 256);
}

int gapro_spp_gt_count(gapro_ctx* ctx, void* stream_, int64_t n_points, int64_t n_labels, const void* d_labels,
                       int32_t label_type, const int64_t* d_gather, const void* d_spps, int32_t spp_is_i64,
                       int32_t n_spps, const void* d_instance_cls, int32_t cls_type, int32_t n_cls,
                       const int64_t* d_offsets, int32_t batch_size, int64_t ignore_label, void* d_workspace,
                       size_t workspace_bytes, gapro_spp_gt_header* d_header, gapro_spp_gt_header* h_header_pinned) {
  const GtDims d{(long long)n_points, batch_size, n_cls, n_spps};
  const GtIn in{d_labels, (const long long*)d_gather, d_spps, spp_is_i64, d_instance_cls, cls_type,
                (const long long*)d_offsets, (long long)n_labels, (long long)ignore_label};
  const int rc = check_args(ctx, "gapro_spp_gt_count", n_points, label_type, in, d, d_workspace, workspace_bytes);
  if (rc != GAPRO_OK) return rc;
  if (!d_header) return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_spp_gt_count: bad argument");
  hipStream_t stream = (hipStream_t)stream_;
  const long long words = (long long)d.inst_copies() * d.inst_stride() + (long long)d.spp_copies() * d.spp_stride();
  hipLaunchKernelGGL(k_gt_init, dim3(grid_for(words, 1, kGridCap)), dim3(kThreads), 0, stream, d_workspace, d,
                     in.offsets);
  with_label_type(label_type, [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    hipLaunchKernelGGL(k_gt_mark<T>, dim3(grid_for(d.n, 1, kGridCap)), dim3(kThreads), 0, stream, d_workspace, d, in);
  });
  hipLaunchKernelGGL(k_gt_rank, dim3(d.B, 2), dim3(kThreads), 0, stream, d_workspace, d, in);
  hipLaunchKernelGGL(k_gt_pack, dim3(1), dim3(kThreads), 0, stream, d_workspace, d, d_header);
  GAPRO_LAUNCH_CHECK(ctx);
  if (h_header_pinned)
    GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(h_header_pinned, d_header, GAPRO_SPP_GT_HEADER_BYTES(batch_size),
                                        hipMemcpyDeviceToHost, stream));
  return GAPRO_OK;
}

int gapro_spp_gt_fill(gapro_ctx* ctx, void* stream_, int64_t n_points, int64_t n_labels, const void* d_labels,
                      int32_t label_type, const int64_t* d_gather, const void* d_spps, int32_t spp_is_i64,
                      int32_t n_spps, const void* d_instance_cls, int32_t cls_type, int32_t n_cls,
                      const float* d_instance_box, const int64_t* d_offsets, int32_t batch_size, int64_t ignore_label,
                      int32_t rule, void* d_workspace, size_t workspace_bytes, float* d_mask, int64_t mask_cells,
                      void* d_cls, float* d_box, int64_t* d_ids, int64_t n_rows, gapro_spp_gt_header* d_header) {
  const GtDims d{(long long)n_points, batch_size, n_cls, n_spps};
  const GtIn in{d_labels, (const long long*)d_gather, d_spps, spp_is_i64, d_instance_cls, cls_type,
                (const long long*)d_offsets, (long long)n_labels, (long long)ignore_label};
  const int rc = check_args(ctx, "gapro_spp_gt_fill", n_points, label_type, in, d, d_workspace, workspace_bytes);
  if (rc != GAPRO_OK) return rc;
  if (!d_mask || mask_cells < 1 || n_rows < 1 || (rule != GAPRO_SPP_GT_HALF && rule != GAPRO_SPP_GT_STRICT) ||
      (d_box != nullptr) != (d_instance_box != nullptr))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_spp_gt_fill: bad argument");
  hipStream_t stream = (hipStream_t)stream_;
  const long long cells = (long long)mask_cells, rows = (long long)n_rows;
  const int point_grid = grid_for(d.n, 1, kGridCap), cell_grid = grid_for(cells, 1, kGridCap);
  hipLaunchKernelGGL(k_gt_clear, dim3(grid_for(cells + (d.S > 0 ? d.n : 0), 1, kGridCap)), dim3(kThreads), 0, stream,
                     d_workspace, d, (unsigned*)d_mask, cells, rows, d_header);
  with_label_type(label_type, [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    if (d.S > 0)
      hipLaunchKernelGGL(k_gt_tally<T>, dim3(point_grid), dim3(kThreads), 0, stream, d_workspace, d, in,
                         (unsigned*)d_mask, cells, rows);
    else
      hipLaunchKernelGGL(k_gt_scatter<T>, dim3(point_grid), dim3(kThreads), 0, stream, d_workspace, d, in, d_mask,
                         cells, rows);
  });
  if (d.S > 0)
    hipLaunchKernelGGL(k_gt_threshold, dim3(cell_grid), dim3(kThreads), 0, stream, d_workspace, d, (unsigned*)d_mask,
                       cells, rows, (int)(rule == GAPRO_SPP_GT_STRICT));
  if (d_cls || d_box || d_ids)
    hipLaunchKernelGGL(k_gt_gather, dim3(grid_for((long long)d.B * d.wi() * 32, 1, kGridCap)), dim3(kThreads), 0, stream,
                       d_workspace, d, in, (const unsigned*)d_instance_box, cells, rows, d_cls, (unsigned*)d_box,
                       (long long*)d_ids);
  GAPRO_LAUNCH_CHECK(ctx);
  return GAPRO_OK;
}

}  // extern "C"
