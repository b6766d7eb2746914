// Launch arithmetic, workspace carving and the status words of the integer kernels (all of them run 256-thread
// workgroups).
#pragma once
#include <stddef.h>

#include "common.h"

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// workgroups of 256 threads for `items` items at `per_thread` items a thread: at least 1, at most `cap`
static inline int grid_for(long long items, int per_thread, int cap) {
  const long long per_block = 256LL * per_thread;
  long long g = (items + per_block - 1) / per_block;
  if (g < 1) g = 1;
  return (int)(g > cap ? cap : g);
}

// a workspace cut into parts, each aligned to 256 bytes; over a null base only bytes() means anything
struct Carver {
  char* base;
  size_t off;
  explicit Carver(void* b) : base((char*)b), off(0) {}
  template <typename T>
  T* take(size_t count) {
    T* q = (T*)(base + off);
    off += align_up(count * sizeof(T), 256);
    return q;
  }
  size_t bytes() const { return off; }
};

// status[0] the code, status[1] the flags of a call whose input is wrong
__device__ inline void raise_bad_arg(int* status, int flag) {
  atomicOr(status + 1, flag);
  atomicExch(status, (int)GAPRO_ERR_BAD_ARG);
}
