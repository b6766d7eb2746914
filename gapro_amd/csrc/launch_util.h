// Host-side launch arithmetic of the integer kernels (all of them run 256-thread workgroups).
#pragma once
#include <stddef.h>

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// workgroups of 256 threads for `items` items at `per_thread` items a thread: at least 1, at most `cap`
static inline int grid_for(long long items, int per_thread, int cap) {
  const long long per_block = 256LL * per_thread;
  long long g = (items + per_block - 1) / per_block;
  if (g < 1) g = 1;
  return (int)(g > cap ? cap : g);
}
