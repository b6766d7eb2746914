// The hash of a coordinate row and the size of the device table of the voxelisation (voxelize.hip; the host sees the
// same two through gapro_voxelize_hash / gapro_voxelize_plan, voxelize_host.cc).  Plain C++: no HIP header.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GAPRO_VOX_HD __host__ __device__
#else
#define GAPRO_VOX_HD
#endif

// the finaliser of MurmurHash3 (Appleby, public domain): every input bit reaches every output bit
GAPRO_VOX_HD static inline uint64_t gapro_vox_mix(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return x;
}

GAPRO_VOX_HD static inline uint64_t gapro_vox_hash(const int64_t* row, int cols) {
  uint64_t h = 0x9e3779b97f4a7c15ULL;
  for (int c = 0; c < cols; ++c) h = gapro_vox_mix(h ^ (uint64_t)row[c]);
  return h;
}

// slots of the table for n points: a power of two, at least 64 and 2 n, at most 2^31 (still more slots than points)
static inline int64_t gapro_vox_slots(int64_t n) {
  if (n < 1 || n > 0x7fffffffLL) return 0;
  int64_t t = 64;
  while (t < 2 * n && t < (1LL << 31)) t <<= 1;
  return t;
}
