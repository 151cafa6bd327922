// w2v_tiles.hpp — what the two dense units share on the device: the queries
// (w2v_nn.hip, nn_score_kernel) and the word classes (w2v_kmeans.hip,
// km_assign_kernel) are one exact-f32 tile product on the matrix cores with a
// different epilogue behind it, instantiated for one list of widths, and their
// one-wave-per-row kernels share a walk and the unit-length rule.
#pragma once
#include <hip/hip_runtime.h>

#include "w2v_limits.hpp"
#include "w2v_mfma.hpp"

namespace w2v {

constexpr int kDenseWaves = 4;      // wavefronts per workgroup of every kernel of the two units
constexpr int kDenseMaxDim = 2048;  // the widest row of an index

// The tile product, template <int NB, int QT> in both kernels. NB > 0: the A
// fragments of rows up to 16 NB floats stay in registers and the next B tile's
// loads are in flight behind this tile's MFMAs. NB == 0: any width, both sides
// are re-read (L1 / L2) per B tile. QT: 16-row A tiles per wave. Every B
// fragment a wave loads feeds QT MFMAs, so QT = 2 halves the L1 / L2 traffic
// per FLOP and gives the MFMA pipe four independent accumulators (a dependent
// v_mfma_f32_16x16x4_f32 issues every 40 cycles, an independent one every 32).
//
// Order: a product has one accumulation order: blocks ascending; of a block's
// four products the first and third go into one accumulator, the second and
// fourth into another, and the two are added at the end. It does not depend on
// NB, QT, the tile slot or the launch; the bit-exact ties and repeats of both
// units rest on it, and on the two kernels' loops staying line for line alike.
// The loop is still written in each kernel: as a __forceinline__ type it ran
// 0.1 to 1.9 % slower than pasted (the compiler simplifies a callee before it
// inlines it, and the blocks reach the scheduler in another order; two
// nn_score_kernel instances also moved a register; profiles/README.md, r12a).

// The instances, X(KERNEL, NB, QT) in ascending NB: the block counts of the
// usual dims exactly (64, 100, 128, 200, 256, 300, 320 floats, then 384 and
// 512), with two A tiles per wave while their fragments fit the register file
// beside two B tiles (rows up to 320 floats) and one beyond. Past 512 floats:
// <0, 1>, which re-reads the fragments.
#define W2V_TILE_INSTANCES(X, KERNEL)                                                      \
  X(KERNEL, 4, 2) X(KERNEL, 7, 2) X(KERNEL, 8, 2) X(KERNEL, 13, 2) X(KERNEL, 16, 2)        \
  X(KERNEL, 19, 2) X(KERNEL, 20, 2) X(KERNEL, 24, 1) X(KERNEL, 32, 1)

// A rows (queries, matrix rows) a workgroup of the <., QT> instances owns.
constexpr int tile_block_rows(int qt) { return kDenseWaves * kSnTile * qt; }

#define W2V_TILE_PICK(KERNEL, NB, QT)        \
  if (nkb_ <= NB) {                          \
    *per_block_ = w2v::tile_block_rows(QT);  \
    return KERNEL<NB, QT>;                   \
  }
// The body of `Fn kernel_for(int cols, int* per_block)`: the instance of KERNEL<NB, QT> with the fewest
// resident blocks that covers a row of `cols` floats, and the A rows its workgroup owns.
#define W2V_TILE_KERNEL_FOR(KERNEL, cols, per_block) \
  const int nkb_ = (cols) / 16;                      \
  int* const per_block_ = (per_block);               \
  W2V_TILE_INSTANCES(W2V_TILE_PICK, KERNEL)          \
  *per_block_ = w2v::tile_block_rows(1);             \
  return KERNEL<0, 1>

// One wavefront per row: lane l owns the 16-B vectors at columns 4 l + 256 v.
constexpr int kRowVecs = kDenseMaxDim / (4 * kWave);  // vectors per lane covering the widest row

// f(c) for each of the lane's vectors inside a row of `cols` floats, for a row that is read once. A kernel that
// holds its row in f32x4[kRowVecs] unrolls over v itself: a helper there moved its registers (profiles/, r12a).
template <class F>
__device__ __forceinline__ void row_walk(int lane, int cols, F f) {
  for (int c = 4 * lane; c < cols; c += 4 * kWave) f(c);
}

__device__ __forceinline__ float sum_sq(f32x4 v) { return v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]; }

// What scales a vector of squared length s to unit length (evaluate.normalize's rule: a zero vector stays zero).
__device__ __forceinline__ float unit_scale(float s) { return 1.0f / fmaxf(sqrtf(s), 1e-12f); }

}  // namespace w2v
