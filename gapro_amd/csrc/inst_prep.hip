// The consumer's per-step instance-label preparation (include/gapro_hip.h, "Instance-label preparation"): ISBNet's
// get_cropped_instance_label (isbnet/model/model_utils.py:589-597) and get_instance_info (:519-555) as one chain of
// kernels, without a host read between them.
//   init     tables of the call's id capacity
//   scan     presence flag per id, largest id, largest |coordinate| of the labelled points, the refusals
//   map      one workgroup: K = distinct ids, the status, and the id map (holes ascending <- ids >= K descending)
//   tally    applies the map to the labels and tallies per new id: count, first point, min / max keys, fixed-point sums
//   final    one lane per instance: box, class, point count, centroid
//   offsets  centroid - p, min - p, max - p per point
// Integer atomics only, so every result is the same bits for every grid and every run.  No workgroup waits for another:
// the kernel boundaries on the stream are the only ordering.  A refusal is a status word written by `map`: every later
// kernel returns at once and neither the labels nor the outputs are touched.
#include "common.h"
#include "exact_sum.h"
#include "label_types.h"
#include "launch_util.h"
#include "wave_reduce.h"

#include <cstdint>
#include <type_traits>

namespace {

constexpr int kThreads = 256;
constexpr int kLdsIds = GAPRO_INST_PREP_LDS_IDS;    // new ids whose tallies a workgroup keeps in LDS
constexpr int kGridCap = GAPRO_INST_PREP_GRID_CAP;  // workgroups of the passes over the points
constexpr int kIdBound = GAPRO_INST_PREP_MAX_IDS;
constexpr unsigned long long kNoPoint = ~0ull;
constexpr unsigned kKeyMax = ~0u;

enum { kFlagNotFinite = 1, kFlagBadId = 2, kFlagBeyondTable = 4 };

struct PrepScalars {  // the first 64 bytes of the workspace
  int max_id;            // largest id met, clamped to kIdBound; -1 without one
  unsigned absmax_bits;  // bits of the largest |coordinate| of the labelled points (non-negative floats order like bits)
  int flags;
  int status;            // set by k_prep_map
  int K;                 // distinct ids >= 0
  int shift;             // fixed_point_shift(absmax, V)
  int reserved[10];
};
static_assert(sizeof(PrepScalars) == 64, "PrepScalars is the first 64 bytes of the workspace");

struct PrepWs {
  PrepScalars* s;
  unsigned long long* first;  // [cap] smallest point index of the new id
  unsigned long long* sum;    // [cap][3] fixed-point coordinate sums
  int* present;               // [cap] old id met
  int* map;                   // [cap] old id -> new id, -1 for an id that is not present
  int* holes;                 // [cap] the empty ids below K, ascending
  int* cnt;                   // [cap] points of the new id
  unsigned* lo;               // [cap][3] keys of the coordinate minima
  unsigned* hi;               // [cap][3] keys of the coordinate maxima
  float* centroid;            // [cap][3]
};

__host__ __device__ inline PrepWs prep_ws(void* base, int cap) {
  PrepWs w;
  char* p = (char*)base;
  const size_t c = (size_t)cap;
  w.s = (PrepScalars*)p; p += sizeof(PrepScalars);
  w.first = (unsigned long long*)p; p += c * 8;
  w.sum = (unsigned long long*)p; p += c * 24;
  w.present = (int*)p; p += c * 4;
  w.map = (int*)p; p += c * 4;
  w.holes = (int*)p; p += c * 4;
  w.cnt = (int*)p; p += c * 4;
  w.lo = (unsigned*)p; p += c * 12;
  w.hi = (unsigned*)p; p += c * 12;
  w.centroid = (float*)p;
  return w;
}
constexpr size_t kBytesPerId = 8 + 24 + 4 * 4 + 12 + 12 + 12;

// order-preserving map float -> uint32 and back (-0.0 sorts below +0.0): integer min / max atomics order floats exactly
__device__ inline unsigned key_of(float x) {
  const unsigned b = __float_as_uint(x);
  return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ inline float float_of(unsigned k) { return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k); }

// The instance id of a label: >= 0, clamped to kIdBound; -1 for a label that names no instance (negative, NaN).  A
// float64 label that is no integer matches no `instance_label == j` of the reference and is refused (*bad).
template <class T>
__device__ inline int id_of(T v, int* bad) {
  if (v < 0) return -1;
  return v >= (T)kIdBound ? kIdBound : (int)v;
}
template <>
__device__ inline int id_of<double>(double v, int* bad) {
  if (!(v >= 0.0)) return -1;
  if (v >= (double)kIdBound) return kIdBound;
  const int id = (int)v;
  if ((double)id != v) *bad = 1;
  return id;
}

__global__ __launch_bounds__(kThreads) void k_prep_init(void* base, int cap) {
  PrepWs w = prep_ws(base, cap);
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < 3 * cap) {
    w.sum[i] = 0ull;
    w.lo[i] = kKeyMax;
    w.hi[i] = 0u;
  }
  if (i < cap) {
    w.first[i] = kNoPoint;
    w.present[i] = 0;
    w.cnt[i] = 0;
  }
  if (i == 0) {
    w.s->max_id = -1;
    w.s->absmax_bits = 0u;
    w.s->flags = 0;
  }
}

template <class LabelT>
__global__ __launch_bounds__(kThreads) void k_prep_scan(long long n, const LabelT* __restrict__ labels,
                                                        const float* __restrict__ coords, void* base, int cap) {
  PrepWs w = prep_ws(base, cap);
  const long long stride = (long long)gridDim.x * kThreads;
  int my_max = -1, flags = 0;
  float amax = 0.f;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
    int bad = 0;
    const int id = id_of(labels[i], &bad);
    if (id < 0) continue;
    my_max = id > my_max ? id : my_max;
    if (bad || id >= kIdBound) {
      flags |= kFlagBadId;
      continue;
    }
    if (id >= cap) flags |= kFlagBeyondTable;
    else w.present[id] = 1;
    if (coords) {
      const float x = coords[3 * i], y = coords[3 * i + 1], z = coords[3 * i + 2];
      if (isfinite(x) && isfinite(y) && isfinite(z)) amax = fmaxf(amax, fmaxf(fabsf(x), fmaxf(fabsf(y), fabsf(z))));
      else flags |= kFlagNotFinite;
    }
  }
  my_max = wave_max(my_max);
  flags = wave_or(flags);
  amax = wave_max(amax);
  if ((threadIdx.x & 63) == 0) {
    if (my_max >= 0) atomicMax(&w.s->max_id, my_max);
    if (flags) atomicOr(&w.s->flags, flags);
    if (amax > 0.f) atomicMax(&w.s->absmax_bits, __float_as_uint(amax));
  }
}

// One workgroup.  K = the number of present ids; the holes h_0 < h_1 < .. of [0, K) take the present ids >= K in
// descending order (there are as many of the one as of the other), every other present id keeps its value.  Without
// `crop` the map is the identity and a hole below the largest id is a refusal.
__global__ __launch_bounds__(kThreads) void k_prep_map(void* base, int cap, long long n, int crop, int info,
                                                       gapro_inst_prep_header* __restrict__ header) {
  PrepWs w = prep_ws(base, cap);
  __shared__ int s_a[kThreads], s_b[kThreads];
  const int t = threadIdx.x;
  const int per = (cap + kThreads - 1) / kThreads;
  const int b0 = min(cap, t * per), b1 = min(cap, b0 + per);
  int c = 0;
  for (int id = b0; id < b1; ++id) c += w.present[id];
  s_a[t] = c;
  __syncthreads();
  int K = 0;
  for (int j = 0; j < kThreads; ++j) K += s_a[j];
  const int flags = w.s->flags, max_id = w.s->max_id;
  int status = GAPRO_OK;
  if (flags & kFlagBadId) status = GAPRO_ERR_BAD_ARG;
  else if (flags & kFlagBeyondTable) status = GAPRO_ERR_WORKSPACE;
  else if (info && (flags & kFlagNotFinite)) status = GAPRO_ERR_NOT_FINITE;
  else if (info && K == 0) status = GAPRO_ERR_BAD_ARG;
  else if (info && !crop && K != max_id + 1) status = GAPRO_ERR_BAD_ARG;
  __syncthreads();  // s_a is reused below
  if (status == GAPRO_OK && crop) {
    int nh = 0, nb = 0;
    for (int id = b0; id < b1; ++id) {
      nh += id < K && !w.present[id];
      nb += id >= K && w.present[id];
    }
    s_a[t] = nh;
    s_b[t] = nb;
    __syncthreads();
    int hp = 0, above = 0;
    for (int j = 0; j < t; ++j) hp += s_a[j];
    for (int j = t + 1; j < kThreads; ++j) above += s_b[j];
    for (int id = b0; id < b1; ++id)
      if (id < K && !w.present[id]) w.holes[hp++] = id;
    __threadfence_block();
    __syncthreads();
    for (int id = b1 - 1; id >= b0; --id) {
      if (!w.present[id]) w.map[id] = -1;
      else w.map[id] = id < K ? id : w.holes[above++];
    }
  } else if (status == GAPRO_OK) {
    for (int id = b0; id < b1; ++id) w.map[id] = w.present[id] ? id : -1;
  }
  if (t == 0) {
    const int shift = fixed_point_shift((double)__uint_as_float(w.s->absmax_bits), n);
    w.s->status = status;
    w.s->K = K;
    w.s->shift = shift;
    header->instance_num = crop ? K : max_id + 1;
    header->n_ids = K;
    header->max_id = max_id;
    header->status = status;
    header->fixed_shift = shift;
    header->flags = flags;
  }
}

struct Tally {  // what one point, or the lanes of a wave that share an id, add to an instance
  int count;
  unsigned long long first;
  unsigned lo[3], hi[3];
  long long q[3];
};

__device__ inline void tally_add(int* cnt, unsigned long long* first, unsigned* lo, unsigned* hi,
                                 unsigned long long* sum, int id, const Tally& v) {
  atomicAdd(&cnt[id], v.count);
  atomicMin(&first[id], v.first);
  for (int k = 0; k < 3; ++k) {
    atomicMin(&lo[3 * id + k], v.lo[k]);
    atomicMax(&hi[3 * id + k], v.hi[k]);
    atomicAdd(&sum[3 * id + k], (unsigned long long)v.q[k]);
  }
}

// Applies the map to the labels (crop) and, with kInfo, tallies per new id.  New ids below kLdsIds are tallied in LDS
// first (one flush per workgroup); the lanes of a wave that all carry one id are combined by shuffles before the atomic.
// The loop is uniform over the workgroup: every lane of a wave reaches the shuffles.
template <class LabelT, bool kInfo>
__global__ __launch_bounds__(kThreads) void k_prep_tally(long long n, LabelT* __restrict__ labels,
                                                         const float* __restrict__ coords, void* base, int cap,
                                                         int crop) {
  PrepWs w = prep_ws(base, cap);
  if (w.s->status != GAPRO_OK) return;
  __shared__ int s_cnt[kInfo ? kLdsIds : 1];
  __shared__ unsigned long long s_first[kInfo ? kLdsIds : 1], s_sum[kInfo ? kLdsIds * 3 : 1];
  __shared__ unsigned s_lo[kInfo ? kLdsIds * 3 : 1], s_hi[kInfo ? kLdsIds * 3 : 1];
  const int nl = kInfo ? min(w.s->K, kLdsIds) : 0;
  const int shift = w.s->shift;
  if (kInfo) {
    for (int j = threadIdx.x; j < nl; j += kThreads) {
      s_cnt[j] = 0;
      s_first[j] = kNoPoint;
    }
    for (int j = threadIdx.x; j < nl * 3; j += kThreads) {
      s_lo[j] = kKeyMax;
      s_hi[j] = 0u;
      s_sum[j] = 0ull;
    }
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long b = (long long)blockIdx.x * kThreads; b < n; b += stride) {
    const long long i = b + threadIdx.x;
    int nid = -1;
    if (i < n) {
      int bad = 0;
      const int id = id_of(labels[i], &bad);
      if (id >= 0) {
        nid = w.map[id];
        if (crop && nid != id) labels[i] = (LabelT)nid;
      }
    }
    if (!kInfo) continue;
    const bool on = nid >= 0;
    const unsigned long long act = __ballot(on);
    if (act == 0ull) continue;  // uniform over the wave
    Tally v;
    v.count = on ? 1 : 0;
    v.first = on ? (unsigned long long)i : kNoPoint;
    for (int k = 0; k < 3; ++k) {
      const float x = on ? coords[3 * i + k] : 0.f;
      v.lo[k] = on ? key_of(x) : kKeyMax;
      v.hi[k] = on ? key_of(x) : 0u;
      v.q[k] = on ? to_fixed((double)x, shift) : 0ll;
    }
    const int lead = __shfl(nid, __ffsll((long long)act) - 1, 64);
    const bool shared_id = __ballot(on && nid != lead) == 0ull;
    int dst = nid;
    bool add = on;
    if (shared_id && __popcll(act) > 1) {
      v.count = __popcll(act);
      v.first = wave_min(v.first);
      for (int k = 0; k < 3; ++k) {
        v.lo[k] = wave_min(v.lo[k]);
        v.hi[k] = wave_max(v.hi[k]);
        v.q[k] = wave_sum(v.q[k]);
      }
      dst = lead;
      add = lane == 0;
    }
    if (add) {
      if (dst < nl) tally_add(s_cnt, s_first, s_lo, s_hi, s_sum, dst, v);
      else tally_add(w.cnt, w.first, w.lo, w.hi, w.sum, dst, v);
    }
  }
  if (kInfo) {
    __syncthreads();
    for (int j = threadIdx.x; j < nl; j += kThreads) {
      if (s_cnt[j] == 0) continue;
      Tally v;
      v.count = s_cnt[j];
      v.first = s_first[j];
      for (int k = 0; k < 3; ++k) {
        v.lo[k] = s_lo[3 * j + k];
        v.hi[k] = s_hi[3 * j + k];
        v.q[k] = (long long)s_sum[3 * j + k];
      }
      tally_add(w.cnt, w.first, w.lo, w.hi, w.sum, j, v);
    }
  }
}

// One lane per instance: box = [min | max], class = the first point's semantic label minus label_shift unless -100
// (model_utils.py:548-553), centroid = the exact mean rounded once to float32.
template <class SemT>
__global__ __launch_bounds__(kThreads) void k_prep_final(void* base, int cap, const SemT* __restrict__ sem,
                                                         long long label_shift, long long* __restrict__ cls,
                                                         float* __restrict__ box, int* __restrict__ pointnum) {
  PrepWs w = prep_ws(base, cap);
  if (w.s->status != GAPRO_OK) return;
  const int r = blockIdx.x * kThreads + threadIdx.x;
  if (r >= w.s->K) return;
  const int c = w.cnt[r], shift = w.s->shift;
  long long s = (long long)sem[w.first[r]];
  if (s != -100) s -= label_shift;
  cls[r] = s;
  pointnum[r] = c;
  for (int k = 0; k < 3; ++k) {
    box[6 * r + k] = float_of(w.lo[3 * r + k]);
    box[6 * r + 3 + k] = float_of(w.hi[3 * r + k]);
    w.centroid[3 * r + k] = (float)fixed_mean((long long)w.sum[3 * r + k], shift, (double)c);
  }
}

// One float32 subtraction per component (:541-543); rows of points without an instance are -100 (:525-530).
template <class LabelT>
__global__ __launch_bounds__(kThreads) void k_prep_offsets(long long n, const float* __restrict__ coords,
                                                           const LabelT* __restrict__ labels, const void* base, int cap,
                                                           const float* __restrict__ box,
                                                           float* __restrict__ centroid_off,
                                                           float* __restrict__ corner_off) {
#pragma clang fp contract(off)
  PrepWs w = prep_ws((void*)base, cap);
  if (w.s->status != GAPRO_OK) return;
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
    int bad = 0;
    const int id = id_of(labels[i], &bad);  // the labels are the new ids by now
    for (int k = 0; k < 3; ++k) {
      const float x = coords[3 * i + k];
      centroid_off[3 * i + k] = id >= 0 ? w.centroid[3 * id + k] - x : -100.0f;
      corner_off[6 * i + k] = id >= 0 ? box[6 * id + k] - x : -100.0f;
      corner_off[6 * i + 3 + k] = id >= 0 ? box[6 * id + 3 + k] - x : -100.0f;
    }
  }
}

struct PrepOut {
  int64_t* cls;
  float* box;
  int32_t* pointnum;
  float* centroid_off;
  float* corner_off;
};

int prep_run(gapro_ctx* ctx, const char* who, void* stream_, int64_t n, const float* d_coords, void* d_labels,
             int32_t label_type, const void* d_sem, int32_t sem_type, int64_t label_shift, int32_t max_ids, void* d_ws,
             size_t ws_bytes, const PrepOut& out, gapro_inst_prep_header* d_header,
             gapro_inst_prep_header* h_header_pinned, bool crop, bool info) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  bool ok = n > 0 && d_labels && max_ids >= 1 && max_ids <= kIdBound && d_ws && d_header;
  if (info) ok = ok && d_coords && d_sem && out.cls && out.box && out.pointnum && out.centroid_off && out.corner_off;
  ok = ok && with_label_type(label_type, [](auto*) {}) && (!info || with_label_type(sem_type, [](auto*) {}));
  if (!ok) return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "%s: bad argument", who);
  if (ws_bytes < gapro_inst_prep_workspace_bytes(max_ids))
    return gapro_fail(ctx, GAPRO_ERR_WORKSPACE, "%s: workspace too small", who);
  hipStream_t stream = (hipStream_t)stream_;
  const int cap = max_ids;
  const long long nn = (long long)n;
  const int grid = grid_for(nn, 1, kGridCap);
  hipLaunchKernelGGL(k_prep_init, dim3((3 * cap + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, d_ws, cap);
  with_label_type(label_type, [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    hipLaunchKernelGGL(k_prep_scan<T>, dim3(grid), dim3(kThreads), 0, stream, nn, (const T*)d_labels,
                       info ? d_coords : (const float*)nullptr, d_ws, cap);
    hipLaunchKernelGGL(k_prep_map, dim3(1), dim3(kThreads), 0, stream, d_ws, cap, nn, (int)crop, (int)info, d_header);
    if (info)
      hipLaunchKernelGGL((k_prep_tally<T, true>), dim3(grid), dim3(kThreads), 0, stream, nn, (T*)d_labels, d_coords,
                         d_ws, cap, (int)crop);
    else
      hipLaunchKernelGGL((k_prep_tally<T, false>), dim3(grid), dim3(kThreads), 0, stream, nn, (T*)d_labels,
                         (const float*)nullptr, d_ws, cap, (int)crop);
  });
  if (info) {
    with_label_type(sem_type, [&](auto* tag) {
      using T = std::remove_pointer_t<decltype(tag)>;
      hipLaunchKernelGGL(k_prep_final<T>, dim3((cap + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, d_ws, cap,
                         (const T*)d_sem, (long long)label_shift, (long long*)out.cls, out.box, out.pointnum);
    });
    with_label_type(label_type, [&](auto* tag) {
      using T = std::remove_pointer_t<decltype(tag)>;
      hipLaunchKernelGGL(k_prep_offsets<T>, dim3(grid), dim3(kThreads), 0, stream, nn, d_coords, (const T*)d_labels,
                         (const void*)d_ws, cap, (const float*)out.box, out.centroid_off, out.corner_off);
    });
  }
  GAPRO_LAUNCH_CHECK(ctx);
  if (h_header_pinned)
    GAPRO_HIP_CHECK(ctx, hipMemcpyAsync(h_header_pinned, d_header, sizeof(gapro_inst_prep_header), hipMemcpyDeviceToHost,
                                        stream));
  return GAPRO_OK;
}

}  // namespace

extern "C" {

size_t gapro_inst_prep_workspace_bytes(int32_t max_ids) {
  if (max_ids < 1 || max_ids > kIdBound) return 0;
  return align_up(sizeof(PrepScalars) + (size_t)max_ids * kBytesPerId, 256);
}

int gapro_inst_crop(gapro_ctx* ctx, void* stream, int64_t n_points, void* d_instance_label, int32_t label_type,
                    int32_t max_ids, void* d_workspace, size_t workspace_bytes, gapro_inst_prep_header* d_header,
                    gapro_inst_prep_header* h_header_pinned) {
  return prep_run(ctx, "gapro_inst_crop", stream, n_points, nullptr, d_instance_label, label_type, nullptr, 0, 0,
                  max_ids, d_workspace, workspace_bytes, PrepOut{}, d_header, h_header_pinned, true, false);
}

int gapro_inst_info(gapro_ctx* ctx, void* stream, int64_t n_points, const float* d_coords,
                    const void* d_instance_label, int32_t label_type, const void* d_semantic_label, int32_t semantic_type,
                    int64_t label_shift, int32_t max_ids, void* d_workspace, size_t workspace_bytes,
                    int64_t* d_instance_cls, float* d_instance_box, int32_t* d_instance_pointnum,
                    float* d_centroid_offset, float* d_corners_offset, gapro_inst_prep_header* d_header,
                    gapro_inst_prep_header* h_header_pinned) {
  const PrepOut out{d_instance_cls, d_instance_box, d_instance_pointnum, d_centroid_offset, d_corners_offset};
  return prep_run(ctx, "gapro_inst_info", stream, n_points, d_coords, (void*)d_instance_label, label_type,
                  d_semantic_label, semantic_type, label_shift, max_ids, d_workspace, workspace_bytes, out, d_header,
                  h_header_pinned, false, true);
}

int gapro_inst_prepare(gapro_ctx* ctx, void* stream, int64_t n_points, const float* d_coords, void* d_instance_label,
                       int32_t label_type, const void* d_semantic_label, int32_t semantic_type, int64_t label_shift,
                       int32_t max_ids, void* d_workspace, size_t workspace_bytes, int64_t* d_instance_cls,
                       float* d_instance_box, int32_t* d_instance_pointnum, float* d_centroid_offset,
                       float* d_corners_offset, gapro_inst_prep_header* d_header,
                       gapro_inst_prep_header* h_header_pinned) {
  const PrepOut out{d_instance_cls, d_instance_box, d_instance_pointnum, d_centroid_offset, d_corners_offset};
  return prep_run(ctx, "gapro_inst_prepare", stream, n_points, d_coords, d_instance_label, label_type, d_semantic_label,
                  semantic_type, label_shift, max_ids, d_workspace, workspace_bytes, out, d_header, h_header_pinned, true,
                  true);
}

}  // extern "C"
