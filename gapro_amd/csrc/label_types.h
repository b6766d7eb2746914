// Arrays that arrive as `const void*` with a type code, shared by the kernels that take labels and indices in the
// caller's dtypes: one template instance per GAPRO_LABEL_* code, one branch per index width.
#pragma once
#include "common.h"

#include <cstdint>

namespace {

// dtype code -> template instance: f gets a null pointer to the element type (non-const: inst_prep.hip writes through
// its labels; a caller that only reads adds the const itself)
template <class F>
bool with_label_type(int code, F&& f) {
  switch (code) {
    case GAPRO_LABEL_F64: f((double*)nullptr); return true;
    case GAPRO_LABEL_I32: f((int32_t*)nullptr); return true;
    case GAPRO_LABEL_I64: f((int64_t*)nullptr); return true;
    default: return false;
  }
}

// entry i of an int32 / int64 index array
__device__ inline long long idx_at(const void* a, int is_i64, long long i) {
  return is_i64 ? ((const long long*)a)[i] : (long long)((const int*)a)[i];
}

}  // namespace
