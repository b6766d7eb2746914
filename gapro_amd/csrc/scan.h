// The integer scans of the plan kernels: the inclusive scan of a wave, the exclusive scan of a
// 256-thread workgroup, and the device-wide exclusive scan of n items in three launches (scan_enqueue):
//   k_devscan_sums   a workgroup per kScanBlock items: their sum, folded per wave first, one LDS atomic a wave;
//   k_devscan_carry  ONE workgroup: the sums become the totals before each block, 256 blocks a trip with a running
//                    carry; the total of all items goes to *total_out if there is one;
//   k_devscan_apply  the scan inside each block, 256 consecutive items at a time in index order.
// No look-back, no spin: no workgroup waits for another.  An item's value comes from a callable val(i) and its result
// goes to a callable emit(i, exclusive, value), both small structs passed to the kernels by value; emit may store where
// val read (item i only), so a scan in place is one of the uses.  The sums are int32: the caller keeps them below 2^31.
#pragma once
#include <hip/hip_runtime.h>

#include "wave_reduce.h"

constexpr int kScanThreads = 256, kScanWaves = kScanThreads / 64;
constexpr int kScanItems = 4;                          // items of a thread in the scan kernels
constexpr int kScanBlock = kScanThreads * kScanItems;  // items of a workgroup there

static inline long long scan_blocks(long long n) { return (n + kScanBlock - 1) / kScanBlock; }  // words of block_sums

// every lane's value -> the sum of the values of the lanes up to and including it
template <typename T>
__device__ inline T wave_inclusive(T v) {
  const int lane = threadIdx.x & 63;
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// Every thread's value -> the sum of the values of the threads before it in the workgroup; *all: the workgroup's sum.
// EVERY thread of a 256-thread workgroup calls (two barriers inside).  wave_tot is kScanWaves words of LDS; the next
// call may reuse it with no barrier in between: the leading barrier is behind every read of the call before.
template <typename T>
__device__ inline T block_exclusive(T v, T* wave_tot, T* all) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T incl = wave_inclusive(v);
  __syncthreads();  // the slots are free again
  if (lane == 63) wave_tot[wave] = incl;
  __syncthreads();
  T before = 0, sum = 0;
#pragma unroll
  for (int w = 0; w < kScanWaves; ++w) {
    const T t = wave_tot[w];
    before += w < wave ? t : 0;
    sum += t;
  }
  *all = sum;
  return before + incl - v;
}

template <typename Val>
__global__ __launch_bounds__(kScanThreads) void k_devscan_sums(Val val, long long n, int* __restrict__ block_sums) {
  __shared__ int total;
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  const long long base = (long long)blockIdx.x * kScanBlock;
  int mine = 0;
#pragma unroll
  for (int j = 0; j < kScanItems; ++j) {
    const long long i = base + j * kScanThreads + threadIdx.x;
    mine += i < n ? val(i) : 0;
  }
  mine = wave_sum(mine);
  if ((threadIdx.x & 63) == 0) atomicAdd(&total, mine);
  __syncthreads();
  if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// T is int.  A template only so that the kernel is compiled into the files that enqueue the scan and not into every
// file that includes this header for block_exclusive (a plain kernel in a header is).  Its one instantiation is a weak
// symbol in each of those files: the linker keeps one copy of the identical code.
template <typename T>
__global__ __launch_bounds__(kScanThreads) void k_devscan_carry(T* __restrict__ block_sums, long long n_blocks,
                                                                T* total_out) {
  __shared__ T wave_tot[kScanWaves];
  T running = 0;
  for (long long b0 = 0; b0 < n_blocks; b0 += kScanThreads) {  // uniform
    const long long b = b0 + threadIdx.x;
    const T v = b < n_blocks ? block_sums[b] : 0;
    T all;
    const T before = block_exclusive(v, wave_tot, &all);
    if (b < n_blocks) block_sums[b] = running + before;
    running += all;
  }
  if (total_out && threadIdx.x == 0) *total_out = running;
}

template <typename Val, typename Emit>
__global__ __launch_bounds__(kScanThreads) void k_devscan_apply(Val val, Emit emit, long long n,
                                                                const int* __restrict__ block_sums) {
  __shared__ int wave_tot[kScanWaves];
  const long long base = (long long)blockIdx.x * kScanBlock;
  int running = block_sums[blockIdx.x];
#pragma unroll
  for (int j = 0; j < kScanItems; ++j) {  // 256 consecutive items at a time, in index order
    const long long i = base + j * kScanThreads + threadIdx.x;
    const int v = i < n ? val(i) : 0;
    int all;
    const int before = running + block_exclusive(v, wave_tot, &all);
    running += all;
    if (i < n) emit(i, before, v);
  }
}

// the plain pair: the values of an int32 array, the results into one, which may be the same array
struct ScanFrom {
  const int* v;
  __device__ int operator()(long long i) const { return v[i]; }
};
struct ScanInto {
  int* out;
  __device__ void operator()(long long i, int before, int) const { out[i] = before; }
};

// enqueues the three launches over n >= 1 items; block_sums: scan_blocks(n) words; total_out: a device word or null
template <typename Val, typename Emit>
inline void scan_enqueue(hipStream_t stream, Val val, Emit emit, long long n, int* block_sums, int* total_out) {
  const long long n_blocks = scan_blocks(n);
  const dim3 grid((unsigned)n_blocks), wg(kScanThreads);
  hipLaunchKernelGGL(k_devscan_sums<Val>, grid, wg, 0, stream, val, n, block_sums);
  hipLaunchKernelGGL(k_devscan_carry<int>, dim3(1), wg, 0, stream, block_sums, n_blocks, total_out);
  hipLaunchKernelGGL((k_devscan_apply<Val, Emit>), grid, wg, 0, stream, val, emit, n, block_sums);
}
