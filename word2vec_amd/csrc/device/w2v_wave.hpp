// w2v_wave.hpp — wave-level primitives of the gfx950 kernels: lane reads and
// broadcasts, the DPP full-wave sum, and the batched dot-product fold. Nothing
// here knows the training arguments; every device unit may include it alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "w2v_limits.hpp"

namespace w2v {

// ---------------------------------------------------------------------------
// Wave primitives
// ---------------------------------------------------------------------------
__device__ __forceinline__ int lane_id() { return (int)__lane_id(); }

template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}

// Full-wave sum, broadcast to every lane (all 64 lanes must be active).
__device__ __forceinline__ float wave_sum(float v) {
  v += dpp_f<0xb1>(v);   // quad_perm [1,0,3,2]
  v += dpp_f<0x4e>(v);   // quad_perm [2,3,0,1]
  v += dpp_f<0x124>(v);  // row_ror:4
  v += dpp_f<0x128>(v);  // row_ror:8
  v += dpp_f<0x142>(v);  // row_bcast:15
  v += dpp_f<0x143>(v);  // row_bcast:31
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

__device__ __forceinline__ int readlane_i(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ float readlane_f(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ int uniform_i(int v) { return __builtin_amdgcn_readfirstlane(v); }
// The first active lane's 64-bit value in every lane (two scalar broadcasts).
__device__ __forceinline__ unsigned long long uniform_u64(unsigned long long v) {
  return ((unsigned long long)(unsigned)uniform_i((int)(v >> 32)) << 32) | (unsigned)uniform_i((int)(unsigned)v);
}

// Lane-register arrays of NCH x 64 positions: element j is lane j % 64 of register j / 64.
template <int NCH>
__device__ __forceinline__ int pick_lane(const int (&v)[NCH], int j) {
  int r = 0;
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch)
    if (ch == (j >> 6)) r = readlane_i(v[ch], j & (kWave - 1));
  return r;
}

__device__ __forceinline__ unsigned long long ballot(bool p) { return __ballot(p); }

// Wait until this wave's outstanding memory operations (incl. no-return atomics) completed.
__device__ __forceinline__ void drain_vmem() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// Keep this wave's LDS accesses in program order (the LDS unit serves one
// wave's operations in order; this only stops the compiler reordering them).
__device__ __forceinline__ void wave_lds_order() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }

// ---------------------------------------------------------------------------
// The dot products of a batch of targets, reduced together. One wave_sum per
// target would cost 6 DPP adds + a readlane each, and gathering the sums back
// into lanes for the batch's sigma step 2 selects + a readlane per target:
// ~13 VALU per target on a kernel that at d = 100 keeps the VALU busy ~77 % of
// its cycles (profiles/r04c_c1_pmc_counters.json: SQ_ACTIVE_INST_VALU /
// SQ_WAVE_CYCLES per SIMD). Instead the NB (4 or 8) per-lane partials are
// folded pairwise, halving the vector count at each step:
//   xor 32  v_permlane32_swap(a, b): a = [a.lo | b.lo], b = [a.hi | b.hi];
//           a + b holds a's half-sums in lanes 0-31 and b's in lanes 32-63
//   xor 16  v_permlane16_swap (odd rows of the first operand with even rows
//           of the second): rows of a + b = [a, b, a', b'] sums
//   xor 8   keep / give selected by lane bit 3 plus a row_ror:8 DPP add
//   xor 4, 2, 1 (one vector left): quad_perm and row_half_mirror DPP adds
// so each group of 8 lanes (NB = 4: of 16) ends with one target's total:
// 18 VALU for 8 targets instead of ~104. The lanes of a group hold identical
// bits (a + b == b + a). Only the order of the 64-term sum changes.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void swap32(float& a, float& b) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  a = __uint_as_float(r[0]);
  b = __uint_as_float(r[1]);
}
__device__ __forceinline__ void swap16(float& a, float& b) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  a = __uint_as_float(r[0]);
  b = __uint_as_float(r[1]);
}
// 16-lane row r of a permlane16-folded vector holds pair member
// ((r & 1) << 1) | (r >> 1) (rows 0..3: members 0, 2, 1, 3; an involution).
__host__ __device__ constexpr int row_member(int r) { return ((r & 1) << 1) | (r >> 1); }
template <int N>
constexpr int kBatchN = N <= 4 ? 4 : 8;
// The first lane of target t's group after batch_dots<N>.
template <int N>
__device__ __forceinline__ constexpr int batch_lane(int t) {
  return kBatchN<N> == 8 ? 16 * row_member(t & 3) + 8 * (t >> 2) : 16 * row_member(t);
}
// The target whose total lane `lane` holds after batch_dots<N>.
template <int N>
__device__ __forceinline__ int batch_target(int lane) {
  return kBatchN<N> == 8 ? 4 * ((lane >> 3) & 1) + row_member(lane >> 4) : row_member(lane >> 4);
}

template <int N>
__device__ __forceinline__ float batch_dots(const float (&p)[N], int lane) {
  static_assert(N >= 1 && N <= 8, "batch of 1..8 targets");
  constexpr int NB = kBatchN<N>;
  float q[NB / 2];
#pragma unroll
  for (int k = 0; k < NB / 2; ++k) {  // xor 32
    float a = 2 * k < N ? p[2 * k] : 0.f, b = 2 * k + 1 < N ? p[2 * k + 1] : 0.f;
    swap32(a, b);
    q[k] = a + b;
  }
  float r[NB / 4];
#pragma unroll
  for (int k = 0; k < NB / 4; ++k) {  // xor 16
    float a = q[2 * k], b = q[2 * k + 1];
    swap16(a, b);
    r[k] = a + b;
  }
  float v;
  if (NB == 8) {  // xor 8: lanes with bit 3 clear keep r[0], set keep r[NB / 4 - 1]
    const bool hi = (lane & 8) != 0;
    const float keep = hi ? r[NB / 4 - 1] : r[0], give = hi ? r[0] : r[NB / 4 - 1];
    v = keep + dpp_f<0x128>(give);  // row_ror:8 (a lane 8 apart: the other bit-3 half)
  } else {
    v = r[0] + dpp_f<0x128>(r[0]);
  }
  v += dpp_f<0xb1>(v);   // quad_perm [1,0,3,2]
  v += dpp_f<0x4e>(v);   // quad_perm [2,3,0,1]
  v += dpp_f<0x141>(v);  // row_half_mirror: the other quad of the 8
  return v;
}

// Batches of N > 8 targets are folded in groups of 8 (batch_g, w2v_kernels.hpp).
template <int N>
constexpr int kGroups = (N + 7) / 8;
template <int N>
constexpr int kGroupN = N < 8 ? N : 8;

}  // namespace w2v
