// w2v_mfma.hpp — the f32 matrix-core tile the shared-negatives kernel, the
// nearest-neighbour queries and k-means are built on.
#pragma once
#include <hip/hip_runtime.h>

namespace w2v {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kSnTile = 16;     // MFMA tile edge: context rows, output rows

__device__ __forceinline__ f32x4 mfma16x16x4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

}  // namespace w2v
