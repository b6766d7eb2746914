// Debug: scan.h's three-launch exclusive scan over an int32 device array, for tests/test_scan_gpu.py.
#include "common.h"
#include "scan.h"

extern "C" int gapro_debug_scan(gapro_ctx* ctx, void* stream_, int64_t n, const int32_t* d_in, int32_t* d_out,
                                int32_t* d_block_sums, int32_t* d_total) {
  if (!ctx) return GAPRO_ERR_BAD_ARG;
  if (n < 1 || n > 0x7fffffffLL || !d_in || !d_out || !d_block_sums || !d_total)
    return gapro_fail(ctx, GAPRO_ERR_BAD_ARG, "gapro_debug_scan: bad argument");
  scan_enqueue((hipStream_t)stream_, ScanFrom{d_in}, ScanInto{d_out}, n, d_block_sums, d_total);
  GAPRO_LAUNCH_CHECK(ctx);
  return GAPRO_OK;
}
