// Voxelisation on the host (include/gapro_hip.h, "Voxelisation"): what a DataLoader worker calls, with
// no device in the process, behind the same count / fill split as the device path, and the header arithmetic both paths
// share.  An ordinary hash map whose values are handed out in insertion order: an independent second implementation of
// the definition (voxels numbered by their first point, rows ascending), not a port of the device's table.
// Host-only: no device, no HIP header.
#include <cstdint>
#include <cstring>
#include <new>
#include <unordered_map>
#include <vector>

#include "../../include/gapro_hip.h"
#include "voxel_hash.h"

namespace {

constexpr int64_t kMaxIndex = 0x7fffffffLL;

struct Key {
  int64_t v[4];
  bool operator==(const Key& o) const { return std::memcmp(v, o.v, sizeof(v)) == 0; }
};
struct KeyHash {
  size_t operator()(const Key& k) const { return (size_t)gapro_vox_hash(k.v, 4); }
};

struct HostVoxels {
  int64_t n = 0;
  int32_t cols = 0, mode = 0, max_active = 1;
  std::vector<int32_t> first, last, count;  // by voxel
};

}  // namespace

extern "C" {

int gapro_voxelize_table_shape(int32_t mode, int64_t n_voxels, int64_t max_active, int64_t* width) {
  if (width) *width = 0;
  if (mode < 0 || mode > 4 || n_voxels < 1 || n_voxels > kMaxIndex || max_active < 1 || max_active > kMaxIndex)
    return GAPRO_ERR_BAD_ARG;
  const bool rows = mode == 3 || mode == 4;
  if (mode == 0 && max_active > 1) return GAPRO_ERR_BAD_ARG;
  if (rows && max_active > GAPRO_VOXELIZE_MAX_ACTIVE) return GAPRO_ERR_BAD_ARG;
  const int64_t w = rows ? max_active + 1 : 2;
  if (n_voxels * w > kMaxIndex) return GAPRO_ERR_BAD_ARG;
  if (width) *width = w;
  return GAPRO_OK;
}

int64_t gapro_voxelize_plan(int64_t n_points) { return gapro_vox_slots(n_points); }

uint64_t gapro_voxelize_hash(const int64_t* row, int32_t cols) {
  return row && cols >= 1 && cols <= 4 ? gapro_vox_hash(row, cols) : 0;
}

int gapro_voxelize_host_count(const int64_t* coords, int64_t n_points, int32_t cols, int32_t mode, int32_t* input_map,
                              gapro_voxelize_header* header, void** handle) {
  if (handle) *handle = nullptr;
  if (!coords || !input_map || !header || !handle || n_points < 1 || n_points > kMaxIndex || (cols != 3 && cols != 4) ||
      mode < 0 || mode > 4)
    return GAPRO_ERR_BAD_ARG;
  *header = gapro_voxelize_header{GAPRO_OK, 0, 0, 0};
  if (cols == 4)
    for (int64_t i = 0; i < n_points; ++i)
      if (coords[4 * i] < 0) {
        header->status = GAPRO_ERR_BAD_ARG;
        header->flags = GAPRO_VOXELIZE_FLAG_BATCH;
        return GAPRO_OK;
      }
  HostVoxels* hv = new (std::nothrow) HostVoxels;
  if (!hv) return GAPRO_ERR_OOM;
  try {
    std::unordered_map<Key, int32_t, KeyHash> seen;
    seen.reserve((size_t)n_points);
    for (int64_t i = 0; i < n_points; ++i) {
      Key k{{0, 0, 0, 0}};
      for (int c = 0; c < cols; ++c) k.v[c] = coords[cols * i + c];
      const auto it = seen.emplace(k, (int32_t)hv->first.size());
      if (it.second) {
        hv->first.push_back((int32_t)i);
        hv->last.push_back((int32_t)i);
        hv->count.push_back(0);
      }
      const int32_t v = it.first->second;
      input_map[i] = v;
      hv->last[v] = (int32_t)i;
      if (++hv->count[v] > hv->max_active) hv->max_active = hv->count[v];
    }
  } catch (const std::bad_alloc&) {
    delete hv;
    return GAPRO_ERR_OOM;
  }
  hv->n = n_points;
  hv->cols = cols;
  hv->mode = mode;
  header->n_voxels = (int32_t)hv->first.size();
  header->max_active = hv->max_active;
  if (mode == 0 && hv->max_active > 1) {
    header->status = GAPRO_ERR_BAD_ARG;
    header->flags = GAPRO_VOXELIZE_FLAG_DUPLICATE;
  }
  *handle = hv;
  return GAPRO_OK;
}

int gapro_voxelize_host_fill(const void* handle, const int64_t* coords, const int32_t* input_map,
                             int64_t* output_coords, int32_t* output_map) {
  const HostVoxels* hv = (const HostVoxels*)handle;
  if (!hv || !coords || !input_map || !output_coords || !output_map) return GAPRO_ERR_BAD_ARG;
  const int64_t M = (int64_t)hv->first.size();
  int64_t width = 0;
  if (gapro_voxelize_table_shape(hv->mode, M, hv->max_active, &width) != GAPRO_OK) return GAPRO_ERR_BAD_ARG;
  const int cols = hv->cols;
  for (int64_t v = 0; v < M; ++v)
    std::memcpy(output_coords + v * cols, coords + (int64_t)hv->first[v] * cols, sizeof(int64_t) * cols);
  if (hv->mode <= 2) {
    for (int64_t v = 0; v < M; ++v) {
      output_map[2 * v] = 1;
      output_map[2 * v + 1] = hv->mode == 2 ? hv->last[v] : hv->first[v];
    }
    return GAPRO_OK;
  }
  std::memset(output_map, 0, sizeof(int32_t) * (size_t)(M * width));
  for (int64_t i = 0; i < hv->n; ++i) {  // in the order of the points: every row comes out ascending
    const int32_t v = input_map[i];
    if (v < 0 || v >= M) return GAPRO_ERR_BAD_ARG;
    int32_t* row = output_map + (int64_t)v * width;
    if (row[0] >= hv->count[v]) return GAPRO_ERR_BAD_ARG;  // not the count's input_map
    row[++row[0]] = (int32_t)i;
  }
  return GAPRO_OK;
}

void gapro_voxelize_host_free(void* handle) { delete (HostVoxels*)handle; }

}  // extern "C"
