// w2v_score.hip — sentence scores under the resident model (w2v_dev_score): the
// log-likelihood the training kernels ascend, read-only.
//
// Every token is a center with the full window (no subsampling, no window
// shrink). Skip-gram scores each context word given the center's W row, CBOW
// the center given the sum (or mean) of its distinct contexts' C rows; HS walks
// the predicted word's Huffman path over synapses1, NS takes the predicted word
// (label 1) and the distinct other words of `negative` Philox table draws
// (label 0) — the training kernels' row layout, gathers, paths and counters
// (w2v_kernels.hpp; the shared pieces: w2v_wave.hpp, w2v_philox.hpp,
// w2v_rows.hpp), with epoch 0 and the caller's key.
//
// One wave scores one work item: up to `item` consecutive centers of one
// sentence, dequeued from a head counter. The input row stays in registers, a
// batch of target rows is gathered with plain loads (nothing writes: no
// L1-bypassing loads, no LDS rows, no atomics on the model), their dots are
// folded together (batch_dots) and one lane per target evaluates
//   log sigma(z) = min(z, 0) - log1p(exp(-|z|))
// in fp32 and adds it to its own fp64 accumulator. One fixed-order cross-lane
// sum per item gives the item's partial; score_reduce_kernel adds a sentence's
// partials in item order. No float atomics: the same bits for any grid.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "w2v_dev_internal.hpp"
#include "w2v_launch.hpp"
#include "w2v_limits.hpp"
#include "w2v_philox.hpp"
#include "w2v_rows.hpp"
#include "w2v_score.hpp"
#include "w2v_wave.hpp"

namespace w2v {

// Target rows gathered per batch: as many of 8 / 4 / 2 as keep a batch within
// 48 VGPRs (64 at 32 floats per lane), so that no instantiation spills.
template <int NV>
constexpr int kScoreT = NV <= 6 ? 8 : NV <= 12 ? 4 : 2;
template <int NV>
constexpr int kScoreMinWaves = NV <= 16 ? 4 : 2;
constexpr int kScoreBlock = 256;

struct ScoreAcc {
  double ll = 0.0;                  // per lane
  unsigned long long targets = 0;   // wave-uniform
  unsigned nonfinite = 0;           // wave-uniform
};

// The terms of T targets: lane t of row_l / code_l holds target t's row of M
// and its code (HS: the Huffman code; NS: 1 - label); the term is
// log sigma((1 - 2 code) * (M[row] . x)).
template <int NV>
__device__ __forceinline__ void score_targets(const float* M, int64_t pitch, int T, int row_l, int code_l,
                                              const float (&x)[NV], int lane, ScoreAcc& acc) {
  constexpr int MT = kScoreT<NV>;
  constexpr int G = kGroupN<MT>;
  constexpr int grp = kBatchN<G> == 8 ? 7 : 15;  // lanes of a group hold one target's total
  for (int t0 = 0; t0 < T; t0 += MT) {
    const int Tb = min(MT, T - t0);
    float r[MT][NV];
#pragma unroll
    for (int t = 0; t < MT; ++t)
      if (t < Tb) load_row<NV>(M, readlane_i(row_l, t0 + t), pitch, lane, false, r[t]);
    float pd[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      pd[t] = 0.f;
      if (t < Tb) {
        pd[t] = r[t][0] * x[0];
#pragma unroll
        for (int v = 1; v < NV; ++v) pd[t] += r[t][v] * x[v];
      }
    }
#pragma unroll
    for (int h = 0; h < kGroups<MT>; ++h) {
      float q[G];
#pragma unroll
      for (int t = 0; t < G; ++t) q[t] = (8 * h + t < MT) ? pd[8 * h + t] : 0.f;
      const float z = batch_dots<G>(q, lane);
      const int t = 8 * h + batch_target<G>(lane);
      const int cl = __shfl(code_l, (t0 + t) & (kWave - 1));
      const bool mine = t < Tb && (lane & grp) == 0;
      const float zz = cl ? -z : z;
      const float term = fminf(zz, 0.f) - log1pf(expf(-fabsf(zz)));
      if (mine) acc.ll += (double)term;
      const unsigned long long bad = ballot(mine && !__builtin_isfinite(z));
      acc.nonfinite += (unsigned)__popcll(bad);
    }
  }
  acc.targets += (unsigned long long)T;
}

// HS: the path of `word` over synapses1, 64 nodes at a time.
template <int NV>
__device__ __forceinline__ void score_path(const ScoreArgs& a, int word, const float (&x)[NV], int lane,
                                           ScoreAcc& acc) {
  const int64_t cb = a.coff[word];
  const int L = (int)(a.coff[word + 1] - cb);
  for (int c0 = 0; c0 < L; c0 += kWave) {
    const int rem = min(kWave, L - c0);
    const int pt_l = (lane < rem) ? a.points[cb + c0 + lane] : 0;
    const int cd_l = (lane < rem) ? (int)a.codes[cb + c0 + lane] : 0;
    score_targets<NV>(a.S, a.pitch, rem, pt_l, cd_l, x, lane, acc);
  }
}

// The training kernels' draws (w2v_philox.hpp) with the caller's key, epoch 0.
__device__ __forceinline__ DrawArgs draw_args(const ScoreArgs& a) {
  return DrawArgs{a.table, a.table_size, a.negative, a.key0, a.key1, 0u};
}

// The span [lo, lo + span) of a center, kWideChunks positions per lane
// (position lo + 64 ch + lane), as cbow_center_wide holds it.
__device__ __forceinline__ void load_span(const int32_t* sent, int lo, int span, int lane, int (&id)[kWideChunks]) {
#pragma unroll
  for (int ch = 0; ch < kWideChunks; ++ch) {
    const int p = kWave * ch + lane;
    id[ch] = (kWave * ch < span && p < span) ? sent[lo + p] : 0;
  }
}

template <int NV, bool HS>
__device__ __forceinline__ void score_sg_center(const ScoreArgs& a, const DrawArgs& da, const int32_t* sent, int len,
                                                int i, uint32_t s, int lane, ScoreAcc& acc,
                                                unsigned long long (&cnt)[3]) {
  const int lo = max(0, i - a.window), hi = min(len, i + a.window + 1);
  const int span = hi - lo, nctx = span - 1;
  if (nctx <= 0) return;
  int id[kWideChunks];
  load_span(sent, lo, span, lane, id);
  float x[NV];
  load_row<NV>(a.W, pick_lane<kWideChunks>(id, i - lo), a.pitch, lane, false, x);
  cnt[0] += 1;
  cnt[1] += (unsigned long long)nctx;
  const int neg = a.negative;
  const int G = HS ? 1 : max(1, kWave / max(neg, 1));  // contexts whose draws fill one wave pass
  int negw_l = 0, slot = 0;
  for (int j = lo; j < hi; ++j) {
    if (j == i) continue;
    const int w = pick_lane<kWideChunks>(id, j - lo);
    if (HS) {
      score_path<NV>(a, w, x, lane, acc);
    } else {
      const int gs = slot % G;
      if (gs == 0) {
        const int nd = min(G, nctx - slot) * neg;
        const uint32_t* rp = nullptr;
        negw_l = draw_negatives<false>(da, s, (uint32_t)i, slot, nd, lane, rp);
        cnt[2] += (unsigned long long)nd;
      }
      int tgt_l;
      const int T = ns_targets(neg, w, negw_l, gs * neg, lane, tgt_l);
      score_targets<NV>(a.C, a.pitch, T, tgt_l, (lane == 0) ? 0 : 1, x, lane, acc);
    }
    ++slot;
  }
}

template <int NV, bool HS>
__device__ __forceinline__ void score_cbow_center(const ScoreArgs& a, const DrawArgs& da, const int32_t* sent,
                                                  int len, int i, uint32_t s, int lane, ScoreAcc& acc,
                                                  unsigned long long (&cnt)[3]) {
  constexpr int MT = kScoreT<NV>;
  const int lo = max(0, i - a.window), hi = min(len, i + a.window + 1);
  const int span = hi - lo, n = span - 1;  // n: context positions
  if (n <= 0) return;
  const int me = i - lo;
  int id[kWideChunks];
  load_span(sent, lo, span, lane, id);
  const int c = pick_lane<kWideChunks>(id, me);
  // the set of context ids (cbow_center_wide's test): a later position repeating an earlier one drops out
  bool dup[kWideChunks];
#pragma unroll
  for (int ch = 0; ch < kWideChunks; ++ch) {
    const int p = kWave * ch + lane;
    dup[ch] = !(p < span && p != me);
  }
  for (int j = 0; j < span; ++j) {
    if (j == me) continue;
    const int v = pick_lane<kWideChunks>(id, j);
#pragma unroll
    for (int ch = 0; ch < kWideChunks; ++ch) dup[ch] = dup[ch] || (j < kWave * ch + lane && v == id[ch]);
  }
  // the distinct ids, compacted in position order: the r-th is lane r % 64 of sid[r / 64]
  int sid[kWideChunks];
#pragma unroll
  for (int ch = 0; ch < kWideChunks; ++ch) sid[ch] = 0;
  int U = 0;
#pragma unroll
  for (int c2 = 0; c2 < kWideChunks; ++c2) {
    unsigned long long m = ballot(!dup[c2]);
    while (m) {
      const int b = __builtin_ctzll(m);
      m &= m - 1;
      const int v = readlane_i(id[c2], b);
#pragma unroll
      for (int ch = 0; ch < kWideChunks; ++ch)
        if (ch == (U >> 6) && lane == (U & (kWave - 1))) sid[ch] = v;
      ++U;
    }
  }
  cnt[0] += 1;
  cnt[1] += (unsigned long long)U;
  float h[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) h[v] = 0.f;
  for (int r0 = 0; r0 < U; r0 += MT) {
    float rr[MT][NV];
#pragma unroll
    for (int t = 0; t < MT; ++t)
      if (r0 + t < U) load_row<NV>(a.C, pick_lane<kWideChunks>(sid, r0 + t), a.pitch, lane, false, rr[t]);
#pragma unroll
    for (int t = 0; t < MT; ++t)
      if (r0 + t < U) {
#pragma unroll
        for (int v = 0; v < NV; ++v) h[v] += rr[t][v];
      }
  }
  if (a.cbow_mean) {
    const float nf = (float)n;
#pragma unroll
    for (int v = 0; v < NV; ++v) h[v] /= nf;
  }
  if (HS) {
    score_path<NV>(a, c, h, lane, acc);
  } else {
    const uint32_t* rp = nullptr;
    const int negw_l = draw_negatives<false>(da, s, (uint32_t)i, 0, a.negative, lane, rp);
    cnt[2] += (unsigned long long)a.negative;
    int tgt_l;
    const int T = ns_targets(a.negative, c, negw_l, 0, lane, tgt_l);
    score_targets<NV>(a.W, a.pitch, T, tgt_l, (lane == 0) ? 0 : 1, h, lane, acc);
  }
}

template <int NV, bool CBOW, bool HS>
__global__ __launch_bounds__(kScoreBlock, kScoreMinWaves<NV>) void score_kernel(ScoreArgs a) {
  const int lane = lane_id();
  const DrawArgs da = draw_args(a);
  unsigned long long cnt[3] = {0, 0, 0};  // centers, contexts, draws
  unsigned nonfinite = 0;
  for (;;) {
    unsigned long long kk = 0;
    if (lane == 0) kk = atomicAdd(a.ctr + kScoreHead, 1ull);
    kk = uniform_u64(kk);
    if ((int64_t)kk >= a.n_items) break;
    int64_t s = 0, hi = a.n_sent - 1;  // the last sentence whose first item is <= kk: the item's owner
    while (s < hi) {
      const int64_t mid = (s + hi + 1) >> 1;
      if (a.item_off[mid] <= (int64_t)kk) s = mid;
      else hi = mid - 1;
    }
    const int64_t base = a.soff[s];
    const int len = (int)(a.soff[s + 1] - base);
    const int32_t* sent = a.ids + base;
    const int i0 = (int)(((int64_t)kk - a.item_off[s]) * a.item);
    const int i1 = min(len, i0 + a.item);
    ScoreAcc acc;
    for (int i = i0; i < i1; ++i) {
      if (CBOW) score_cbow_center<NV, HS>(a, da, sent, len, i, (uint32_t)s, lane, acc, cnt);
      else score_sg_center<NV, HS>(a, da, sent, len, i, (uint32_t)s, lane, acc, cnt);
    }
    double v = acc.ll;  // fixed order: the same partial whichever wave scored the item
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) {
      a.part_ll[kk] = v;
      a.part_targets[kk] = (int64_t)acc.targets;
      a.part_nonfinite[kk] = acc.nonfinite;
    }
    nonfinite += acc.nonfinite;
  }
  if (lane == 0) {  // integer counters: any order gives the same sums
    if (cnt[0]) atomicAdd(a.ctr + kScoreCenters, cnt[0]);
    if (cnt[1]) atomicAdd(a.ctr + kScoreContexts, cnt[1]);
    if (cnt[2]) atomicAdd(a.ctr + kScoreDraws, cnt[2]);
    if (nonfinite) atomicAdd(a.ctr + kScoreNonFinite, (unsigned long long)nonfinite);
  }
}

// The second pass: a sentence's partials in item order; a non-finite dot
// product makes the sentence's score NaN.
__global__ void score_reduce_kernel(ScoreArgs a) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= a.n_sent) return;
  double ll = 0.0;
  int64_t tg = 0;
  unsigned bad = 0;
  const int64_t k1 = a.item_off[s + 1];
#pragma unroll 8
  for (int64_t k = a.item_off[s]; k < k1; ++k) {
    ll += a.part_ll[k];
    tg += a.part_targets[k];
    bad |= a.part_nonfinite[k];
  }
  a.ll[s] = bad ? __longlong_as_double(0x7FF8000000000000ll) : ll;
  a.targets[s] = tg;
}

namespace {

using ScoreFn = void (*)(ScoreArgs);

template <int NV>
ScoreFn pick_score(bool cbow, bool hs) {
  if (cbow) return hs ? &score_kernel<NV, true, true> : &score_kernel<NV, true, false>;
  return hs ? &score_kernel<NV, false, true> : &score_kernel<NV, false, false>;
}

ScoreFn score_fn(int nv, bool cbow, bool hs) {
#define W2V_SCORE_NV(N) \
  if (nv == N) return pick_score<N>(cbow, hs);
  W2V_FOR_EACH_NV(W2V_SCORE_NV)
#undef W2V_SCORE_NV
  return nullptr;
}

}  // namespace

int score_launch(const ScoreArgs& a, int nv, bool cbow, bool hs, int64_t max_waves, int n_cu, hipStream_t stream) {
  const ScoreFn fn = score_fn(nv, cbow, hs);
  if (!fn) return set_error(W2V_ERR_UNSUPPORTED, "w2v_dev_score: no kernel for this row width");
  W2V_HIP_TRY(hipMemsetAsync(a.ctr, 0, kScoreCounters * sizeof(unsigned long long), stream));
  if (a.n_items > 0) {
    int per_cu = 0;
    W2V_HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, kScoreBlock, 0));
    const int wpb = kScoreBlock / kWave;
    int64_t waves = (int64_t)std::max(per_cu, 1) * n_cu * wpb;
    if (max_waves > 0) waves = std::min(waves, max_waves);
    waves = std::max<int64_t>(1, std::min(waves, a.n_items));
    const int threads = (int)std::min<int64_t>(wpb, waves) * kWave;
    const int64_t grid = (waves * kWave + threads - 1) / threads;
    hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3((unsigned)threads), 0, stream, a);
    W2V_HIP_TRY(hipGetLastError());
  }
  if (a.n_sent > 0) {
    hipLaunchKernelGGL(score_reduce_kernel, dim3((unsigned)((a.n_sent + 255) / 256)), dim3(256), 0, stream, a);
    W2V_HIP_TRY(hipGetLastError());
  }
  return W2V_OK;
}

}  // namespace w2v
