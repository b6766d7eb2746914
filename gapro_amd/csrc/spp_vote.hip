// Superpoint vote of per-point labels (include/gapro_hip.h, "Superpoint vote"): the reference's spp_align_label
// (gen_ps_utils.py:99-129) and spp_major_voting (:132-166) behind one entry point.
//   tally   cnt[s, c] += 1 per point (int32 atomics); checks ids, labels and probabilities; max |prob|
//   occ     spp_major_voting only: occn[s, b] += 1 per point inside box b (int32 atomics)
//   sums    P[s, c] += rint(prob * 2^k) per point (int64 atomics: exact, so the order does not matter)
//   final   one lane per superpoint: masked counts, first maximum, the probability in float64
//   back    label_spp / prob_spp gathered to the points
// A refusal raised by tally is a status word in the workspace: every later kernel returns at once and the outputs stay
// untouched.  The heuristic labelers keep their own welded vote (labels.hip k_lab_tally / k_lab_argmax, LabWs).
#include "common.h"
#include "exact_sum.h"
#include "launch_util.h"

namespace {

constexpr int kThreads = 256;

struct VoteHeader {
  int status;             // gapro_status raised by k_vote_tally (the most negative code wins)
  unsigned absmax_bits;   // bits of max |prob| (non-negative floats order like their bits)
  int reserved[14];
};
static_assert(sizeof(VoteHeader) == 64, "VoteHeader is the first 64 bytes of the workspace");

struct VoteWs {
  VoteHeader* hdr;
  long long* P;     // [S, C] fixed-point probability sums
  int* cnt;         // [S, C]
  int* occn;        // [S, C - 1] points of s inside box b (major)
  int* label_spp;   // [S]
  float* prob_spp;  // [S]
  size_t bytes;
};

inline size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

VoteWs carve(void* base, long long S, long long C) {
  VoteWs w;
  char* p = (char*)base;
  w.hdr = (VoteHeader*)p; p += sizeof(VoteHeader);
  w.P = (long long*)p; p += up16((size_t)(S * C) * 8);
  w.cnt = (int*)p; p += up16((size_t)(S * C) * 4);
  w.occn = (int*)p; p += up16((size_t)(S * (C > 1 ? C - 1 : 0)) * 4);
  w.label_spp = (int*)p; p += up16((size_t)S * 4);
  w.prob_spp = (float*)p; p += up16((size_t)S * 4);
  w.bytes = (size_t)(p - (char*)base);
  return w;
}

template <typename LabelT>
__global__ __launch_bounds__(kThreads) void k_vote_tally(long long n, int S, int C, int major,
                                                         const int* __restrict__ ids, const LabelT* __restrict__ label,
                                                         const float* __restrict__ prob, VoteHeader* hdr,
                                                         int* __restrict__ cnt) {
  const long long stride = (long long)gridDim.x * kThreads;
  int bad = 0;
  float amax = 0.f;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
    const int s = ids[i];
    const long long c = (long long)label[i];
    int why = 0;
    if (s < 0 || s >= S || c < 0 || c >= C) why = GAPRO_ERR_BAD_ARG;
    if (prob) {
      const float v = prob[i];
      if (!isfinite(v)) why = GAPRO_ERR_NOT_FINITE;
      else if (major && (v < 0.f || v > 1.f)) why = why ? why : GAPRO_ERR_BAD_ARG;
      else amax = fmaxf(amax, fabsf(v));
    }
    if (why) { bad = why < bad ? why : bad; continue; }
    atomicAdd(&cnt[(long long)s * C + c], 1);
  }
  if (bad) atomicMin(&hdr->status, bad);
  if (amax > 0.f) atomicMax(&hdr->absmax_bits, __float_as_uint(amax));
}

// one lane per (point, box) element of the [N, C - 1] occupancy: consecutive lanes read consecutive bytes
__global__ __launch_bounds__(kThreads) void k_vote_occ(long long n, int S, int C, const int* __restrict__ ids,
                                                       const unsigned char* __restrict__ occ, int* __restrict__ occn) {
  const int B = C - 1;
  const long long tot = n * B, stride = (long long)gridDim.x * kThreads;
  for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < tot; e += stride) {
    if (!occ[e]) continue;
    const long long i = e / B;
    const int s = ids[i];
    if (s >= 0 && s < S) atomicAdd(&occn[(long long)s * B + (e - i * B)], 1);
  }
}

template <typename LabelT>
__global__ __launch_bounds__(kThreads) void k_vote_sums(long long n, int C, const int* __restrict__ ids,
                                                        const LabelT* __restrict__ label,
                                                        const float* __restrict__ prob, const VoteHeader* hdr,
                                                        long long* __restrict__ P) {
  if (hdr->status != 0) return;
  const int k = fixed_point_shift((double)__uint_as_float(hdr->absmax_bits), n);
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
    const long long q = to_fixed((double)prob[i], k);
    if (q) atomicAdd((unsigned long long*)&P[(long long)ids[i] * C + (long long)label[i]], (unsigned long long)q);
  }
}

// gate: align = u8[C - 1, S] (NULL: every gate open); major = the occupancy counts of k_vote_occ, open at n[s]
__global__ __launch_bounds__(kThreads) void k_vote_final(long long n, int S, int C, int major, int has_prob,
                                                         const unsigned char* __restrict__ gate, VoteWs w) {
  if (w.hdr->status != 0) return;
  const int k = fixed_point_shift((double)__uint_as_float(w.hdr->absmax_bits), n);
  for (int s = blockIdx.x * kThreads + threadIdx.x; s < S; s += gridDim.x * kThreads) {
    const int* __restrict__ cnt = w.cnt + (long long)s * C;
    const long long* __restrict__ P = w.P + (long long)s * C;
    int ns = 0;
    for (int c = 0; c < C; ++c) ns += cnt[c];
    int best = 0, best_m = -1;
    long long p_all = 0;
    double acc = 0.0;
    for (int c = 0; c < C; ++c) {
      bool open = true;
      if (c >= 1) {
        if (major) open = w.occn[(long long)s * (C - 1) + (c - 1)] == ns;
        else if (gate) open = gate[(long long)(c - 1) * S + s] != 0;
      }
      const int m = open ? cnt[c] : 0;
      if (m > best_m) { best_m = m; best = c; }  // strict: the first maximum (torch.argmax)
      if (has_prob) {
        if (major) {
#pragma clang fp contract(off)
          const double mean = fixed_mean(P[c], k, (double)cnt[c] + 1e-4);
          const double share = ns > 0 ? (double)m / (double)ns : 0.0;  // ns == 0: S beyond the ranks present
          const double term = mean * share;
          acc = acc + term;
        } else {
          p_all += P[c];
        }
      }
    }
    w.label_spp[s] = best;
    if (has_prob) w.prob_spp[s] = major ? (float)acc : (ns > 0 ? (float)fixed_mean(p_all, k, (double)ns) : 0.f);
  }
}

__global__ __launch_bounds__(kThreads) void k_vote_back(long long n, const int* __restrict__ ids, VoteWs w,
                                                        long long* __restrict__ label_out,
                                                        float* __restrict__ prob_out) {
  if (w.hdr->status != 0) return;
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
    const int s = ids[i];
    label_out[i] = w.label_spp[s];
    if (prob_out) prob_out[i] = w.prob_spp[s];
  }
}

__global__ void k_vote_status(const VoteHeader* hdr, int* status) { *status = hdr->status; }

bool sizes_ok(long long n, long long S, long long C) {
  return n >= 1 && S >= 1 && C >= 1 && S <= n && S * C <= 0x7fffffffLL && n <= 0x7fffffffffLL / C;
}

}  // namespace

extern "C" {

size_t gapro_spp_vote_workspace_bytes(int64_t n_points, int32_t n_spps, int32_t n_classes) {
  if (!sizes_ok(n_points, n_spps, n_classes)) return 0;
  return carve(nullptr, n_spps, n_classes).bytes;
}

int gapro_spp_vote(gapro_ctx* ctx, void* stream_, int32_t mode, int64_t n_points, int32_t n_spps, int32_t n_classes,
                   const int32_t* d_ids, const void* d_label, int32_t label_is_i64, const float* d_prob,
                   const uint8_t* d_gate, void* d_ws, size_t ws_bytes, int64_t* d_label_out, float* d_prob_out,
                   int32_t* d_status) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  if ((mode != GAPRO_VOTE_ALIGN && mode != GAPRO_VOTE_MAJOR) || !sizes_ok(n_points, n_spps, n_classes))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_spp_vote: bad argument (mode %d, %lld points, %d superpoints, %d classes)",
                      (int)mode, (long long)n_points, (int)n_spps, (int)n_classes);
  const bool major = mode == GAPRO_VOTE_MAJOR;
  if (!d_ids || !d_label || !d_ws || !d_label_out || !d_status || (d_prob != nullptr) != (d_prob_out != nullptr) ||
      (major && (!d_prob || (n_classes > 1 && !d_gate))))
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_spp_vote: null argument");
  const VoteWs w = carve(d_ws, n_spps, n_classes);
  if (ws_bytes < w.bytes)
    return gapro_fail(ctx, GAPRO_ERR_WORKSPACE, "gapro_spp_vote: workspace of %zu bytes, %zu needed", ws_bytes, w.bytes);
  hipStream_t stream = (hipStream_t)stream_;
  const long long n = n_points;
  const int S = n_spps, C = n_classes, g = grid_for(n, 1, 4096);
  GAPRO_HIP_CHECK(ctx, hipMemsetAsync(d_ws, 0, w.bytes, stream));
  if (label_is_i64)
    hipLaunchKernelGGL(k_vote_tally<long long>, dim3(g), dim3(kThreads), 0, stream, n, S, C, (int)major, d_ids,
                       (const long long*)d_label, d_prob, w.hdr, w.cnt);
  else
    hipLaunchKernelGGL(k_vote_tally<int>, dim3(g), dim3(kThreads), 0, stream, n, S, C, (int)major, d_ids,
                       (const int*)d_label, d_prob, w.hdr, w.cnt);
  if (major && C > 1)
    hipLaunchKernelGGL(k_vote_occ, dim3(grid_for(n * (C - 1), 1, 4096)), dim3(kThreads), 0, stream, n, S, C, d_ids, d_gate,
                       w.occn);
  if (d_prob) {
    if (label_is_i64)
      hipLaunchKernelGGL(k_vote_sums<long long>, dim3(g), dim3(kThreads), 0, stream, n, C, d_ids,
                         (const long long*)d_label, d_prob, w.hdr, w.P);
    else
      hipLaunchKernelGGL(k_vote_sums<int>, dim3(g), dim3(kThreads), 0, stream, n, C, d_ids, (const int*)d_label,
                         d_prob, w.hdr, w.P);
  }
  hipLaunchKernelGGL(k_vote_final, dim3(grid_for(S, 1, 4096)), dim3(kThreads), 0, stream, n, S, C, (int)major,
                     d_prob ? 1 : 0, major ? nullptr : d_gate, w);
  hipLaunchKernelGGL(k_vote_back, dim3(g), dim3(kThreads), 0, stream, n, d_ids, w, (long long*)d_label_out,
                     d_prob_out);
  hipLaunchKernelGGL(k_vote_status, dim3(1), dim3(1), 0, stream, w.hdr, d_status);
  GAPRO_LAUNCH_CHECK(ctx);
  return GAPRO_OK;
}

}  // extern "C"
