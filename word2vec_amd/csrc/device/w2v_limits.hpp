// w2v_limits.hpp — the limits the kernels (w2v_kernels.hpp and the headers under it, w2v_shared.hpp)
// and the launch policy (w2v_policy.cpp) share. No HIP header: the policy is
// compiled by the host compiler too.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define W2V_HD __host__ __device__
#else
#define W2V_HD
#endif

namespace w2v {

constexpr int kWave = 64;
// Largest workgroup per row width: up to 16 waves share one LDS region of
// privatised rows while the register budget (<=128 VGPRs at 4 waves/SIMD)
// holds; wider rows keep 4-wave workgroups.
constexpr int max_block(int nv) { return nv <= 6 ? 1024 : 256; }
template <int NV>
constexpr int kMaxBlock = max_block(NV);
// Waves per SIMD the epoch kernel is compiled for: two 16-wave workgroups per
// CU when a row is <= 2 floats per lane (d <= 128: 64 VGPRs), else one.
constexpr int min_waves(int nv) { return nv <= 2 ? 8 : nv <= 16 ? 4 : 2; }  // d > 1024: 256 VGPRs
template <int NV>
constexpr int kMinWaves = min_waves(NV);

// LDS the shared-negatives kernel gives its row slots (w2v_shared.hpp kSnPriv; <= 32 rows):
// 20 KiB = 10 rows at d = 512 with four 2-wave workgroups per CU (38.9 KiB each).
constexpr int kSnPrivBytes = 20 * 1024;

// LDS-privatised rows of the per-pair kernel (layout: w2v_kernels.hpp): the
// output range holds at most kPrivMax rows, the context range kCtxMax.
constexpr int kPrivMax = 128;
constexpr int kCtxMax = 64;
// The region's header, in 32-bit words, then the pending deltas.
constexpr int kLdsDirtyOut = 0;   // [0, 4): dirty mask of the output rows (2 x 64 bits)
constexpr int kLdsDirtyCtx = 4;   // [4, 8): dirty mask of the context rows
constexpr int kLdsCenters = 8;    // centers of the workgroup
constexpr int kLdsLockOut = 9;    // [9, 13): lock bits of the output rows
constexpr int kLdsLockCtx = 13;   // [13, 15): lock bits of the context rows
constexpr int kLdsHeaderWords = 16;

constexpr int kWideChunks = 4;  // wide-window CBOW kernels: window <= 32 * kWideChunks - 1 in registers
constexpr int kMaxWideWindow = 32 * kWideChunks - 1;
// Ints of a wave's cbow_center_huge scratch slice for `window`: the unique
// ids (<= 2 window) and one 64-bit unique mask per 64 span positions.
W2V_HD inline int64_t huge_stride(int window) {
  const int64_t span = 2 * (int64_t)window + 1;
  return 2 * (int64_t)window + 2 * ((span + 63) / 64) + 2;
}

// Workgroup size of train_epoch_deep_kernel.
constexpr int kDeepBlock = 256;

}  // namespace w2v
