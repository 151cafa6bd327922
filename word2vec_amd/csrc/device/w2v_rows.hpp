// w2v_rows.hpp — embedding-row I/O of the per-pair kernels: a row spread over
// the wave one dword per lane per 64 elements, gathered, stored and added whole.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "w2v_limits.hpp"

namespace w2v {

// ---------------------------------------------------------------------------
// Row I/O: a row is NV floats per lane, element lane + 64 v (v < NV). Rows
// are NV * 64 floats apart at least (pitch >= NV * 64, w2v_dev_bind_model)
// and their columns past word_dim are zero, and stay zero: every delta there
// is g * 0. So every lane loads, stores and adds its whole row, with no
// per-element guard: no exec-mask branches around the memory instructions
// (an exec-masked zero-fill of a register whose load may be outstanding made
// the compiler wait for ALL this wave's memory operations — vmcnt(0), stores
// and memory-side atomics included — before every hot row's gather), and
// every store writes whole 128-B lines. The dot products add the padding's
// zeros, so the sums are bit-identical to the guarded form.
// ---------------------------------------------------------------------------
template <int NV>
__device__ __forceinline__ void load_row(const float* M, int64_t row, int64_t pitch, int lane, bool fresh,
                                         float (&r)[NV]) {
  const float* p = M + row * pitch + lane;
  if (fresh) {  // agent-scope relaxed loads: global_load_dword sc1, bypass the CU's L1
#pragma unroll
    for (int v = 0; v < NV; ++v) r[v] = __hip_atomic_load(p + kWave * v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {
#pragma unroll
    for (int v = 0; v < NV; ++v) r[v] = p[kWave * v];
  }
}

template <int NV>
__device__ __forceinline__ void store_row(float* M, int64_t row, int64_t pitch, int lane, const float (&r)[NV]) {
  float* p = M + row * pitch + lane;
#pragma unroll
  for (int v = 0; v < NV; ++v) p[kWave * v] = r[v];
}

// row += delta, memory-side (no-return global_atomic_add_f32, 256 contiguous B
// per instruction). The padding lanes are masked here: an atomic has no
// destination register (nothing to zero-fill, no wait), and a memory-side add
// of 0 would still cost the atomic unit a request (d 300: 320 adds per row
// instead of 300; measured 2.5 % of configs[2], profiles/r03d_guards_ab.log).
// Vectors of a row every lane of which is inside word_dim: pick_nv
// (w2v_dev.hip) takes the smallest row width >= ceil(d / 64) of {1, 2, 3, 4,
// 5, 6, 8, 12, 16, 24, 32}, so d > 64 x the next smaller width and those
// vectors need no lane mask (a mask is an exec-mask round trip per atomic).
template <int NV>
constexpr int kFullVecs = NV <= 6 ? NV - 1 : NV == 8 ? 6 : NV == 12 ? 8 : NV == 16 ? 12 : NV == 24 ? 16 : 24;

template <int NV>
__device__ __forceinline__ void atomic_add_row(float* M, int64_t row, int64_t pitch, int d, int lane,
                                               const float (&delta)[NV]) {
  float* p = M + row * pitch + lane;
#pragma unroll
  for (int v = 0; v < NV; ++v)
    if (v < kFullVecs<NV> || lane + kWave * v < d)
      (void)__hip_atomic_fetch_add(p + kWave * v, delta[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// M[row] += delta: atomically for hot rows; else read-modify-write (Hogwild).
template <int NV>
__device__ __forceinline__ void add_to_row(float* M, int64_t row, bool hot, int64_t pitch, int d, int lane,
                                           const float (&delta)[NV]) {
  if (hot) {
    atomic_add_row<NV>(M, row, pitch, d, lane, delta);
  } else {
    float cur[NV];
    load_row<NV>(M, row, pitch, lane, false, cur);
#pragma unroll
    for (int v = 0; v < NV; ++v) cur[v] += delta[v];
    store_row<NV>(M, row, pitch, lane, cur);
  }
}

}  // namespace w2v
