// w2v_philox.hpp — the counter-based RNG of the throughput mode and the draws
// made with it: every random decision is a pure function of (key, epoch,
// sentence, position, slot, k). The training kernels and the scoring kernel
// draw through the same helpers, each from its own arguments (see DrawArgs).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "w2v_wave.hpp"

namespace w2v {

// ---------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al. SC'11), the throughput-mode RNG.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                       uint32_t k0, uint32_t k1, uint32_t& o0, uint32_t& o1,
                                       uint32_t& o2, uint32_t& o3) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  o0 = c0; o1 = c1; o2 = c2; o3 = c3;
}

// libstdc++ generate_canonical<float,24> of one 32-bit draw.
__device__ __forceinline__ float canonical_f(uint32_t x) {
  float r = (float)x * (1.0f / 4294967296.0f);
  return r >= 1.0f ? __int_as_float(0x3F7FFFFF) : r;
}

// What the draws read: the unigram table, the negative count and the stream's
// key and epoch. The helpers below take any `Args` with these six members: the
// training kernels pass their TrainArgs as it is (each field is then read from
// the kernel arguments at its point of use, which a copy made up front changes:
// scratch moved in several kernels of row widths 16 and 24), a kernel with
// other arguments fills a DrawArgs.
struct DrawArgs {
  const uint32_t* table;
  int64_t table_size;
  int32_t negative;
  uint32_t key0, key1, epoch;
};

// The subsampling draw of token i of sentence s: u for the keep test and the
// window shrink rw in [0, wmax).
template <class Args>
__device__ __forceinline__ void subsample_draw(const Args& a, uint32_t s, uint32_t i, uint32_t wmax, float& u,
                                               int& rw) {
  uint32_t o0, o1, o2, o3;
  philox(i, s, 0xFFFFFFFFu, a.epoch, a.key0, a.key1, o0, o1, o2, o3);
  u = canonical_f(o0);
  rw = (int)(((uint64_t)o1 * wmax) >> 32);
}

// Draw k of context slot `slot`: counter (position, sentence, slot << 8 | k's
// low byte, epoch ^ (k's high bits << 20)); for k < 256 (every negative up to
// 255) the last word is the epoch alone.
template <class Args>
__device__ __forceinline__ uint32_t philox_table_pos(const Args& a, uint32_t s, uint32_t i, uint32_t slot,
                                                     uint32_t k) {
  uint32_t o0, o1, o2, o3;
  philox(i, s, (slot << 8) | (k & 255u), a.epoch ^ ((k >> 8) << 20), a.key0, a.key1, o0, o1, o2, o3);
  const uint64_t x = ((uint64_t)o1 << 32) | o0;
  return (uint32_t)__umul64hi(x, (uint64_t)a.table_size);
}

// Draw table words for `ndraw` (slot, k) pairs starting at slot `slot0`:
// lane t -> slot0 + t / neg, k = t % neg.
template <bool REPLAY, class Args>
__device__ __forceinline__ int draw_negatives(const Args& a, uint32_t s, uint32_t i, int slot0, int ndraw,
                                              int lane, const uint32_t*& rp) {
  int w = 0;
  if (lane < ndraw) {
    uint32_t pos;
    if (REPLAY) {
      pos = rp[lane];
    } else {
      const int neg = a.negative;
      pos = philox_table_pos(a, s, i, (uint32_t)(slot0 + lane / neg), (uint32_t)(lane % neg));
    }
    w = (int)a.table[pos];
  }
  if (REPLAY) rp += ndraw;
  return w;
}

// Chunk ch of a slot's draws when negative >= 64 (ns_word_many): lane -> draw
// k = 64 ch + lane, -1 past the last.
template <bool REPLAY, class Args>
__device__ __forceinline__ int draw_chunk(const Args& a, uint32_t s, uint32_t i, int slot, int ch, int lane,
                                          const uint32_t* rp) {
  const int k = kWave * ch + lane;
  int w = -1;
  if (k < a.negative) {
    const uint32_t pos = REPLAY ? rp[k] : philox_table_pos(a, s, i, (uint32_t)slot, (uint32_t)k);
    w = (int)a.table[pos];
  }
  return w;
}

// NS target list of positive `word` against `negw_l` lanes [base, base + neg):
// lane t of tgt_l holds target t (positive first, then first occurrences of
// the negatives that differ from it — the set semantics of
// Word2Vec.cpp:253-257); returns the count.
__device__ __forceinline__ int ns_targets(int neg, int word, int negw_l, int base, int lane, int& tgt_l) {
  const int nk = __shfl(negw_l, (base + lane) & (kWave - 1));
  bool dup = (lane >= neg) || (nk == word);
  for (int j = 0; j < neg - 1; ++j) {
    const int v = readlane_i(nk, j);
    dup = dup || (lane > j && nk == v);
  }
  const unsigned long long uniq = ballot(!dup);
  // compaction in one forward permute: the k-th unique draw (in lane order)
  // goes to lane 1 + k; duplicates to lane 0, which then takes the positive
  // (a walk over the set bits cost ~4 VALU + 6 SALU per target)
  const int k = __builtin_amdgcn_mbcnt_hi((unsigned)(uniq >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)uniq, 0u));
  const int v = __builtin_amdgcn_ds_permute((dup ? 0 : 1 + k) << 2, nk);
  tgt_l = (lane == 0) ? word : v;
  return 1 + __popcll(uniq);
}

}  // namespace w2v
