// w2v_kernels.hpp — gfx950 (CDNA4) training kernels for the Word2Vec hot path.
//
// What they compute is the reference's per-sentence update, unchanged:
//   skip-gram  Word2Vec.cpp:319-353 (center W row is the input, fixed over the
//              window; each context word is predicted; W[center] += grad once)
//   CBOW       Word2Vec.cpp:273-317 (sum of C rows over the SET of context ids,
//              /n if cbow_mean; scatter grad back to every unique id)
//   NS         Word2Vec.cpp:251-271 (unique negatives from the unigram table,
//              the positive overrides a colliding negative)
//   HS         Word2Vec.cpp:232-249 (walk the Huffman path of the predicted word)
// and the epoch loop Word2Vec.cpp:371-395 (sentences in the shuffled order,
// alpha recomputed from the shared word counter every 10th sentence).
//
// How they map to MI355X:
//   * one 64-lane wavefront owns one sentence at a time and walks it in order,
//     exactly like one OpenMP thread of the reference; wavefronts dequeue
//     sentences from a global head counter (Hogwild across sentences, as the
//     reference is across threads). A one-wave grid is the deterministic
//     sequential schedule used for parity.
//   * an embedding row is spread over the wave one dword per lane per 64
//     elements (element lane + 64 v): every row gather is NV fully coalesced
//     256-B wave instructions, and a row update is NV 256-B contiguous
//     instructions — the shape at which MI355X float atomics run at full rate.
//     The rows of all targets of one context (<= MAXT) are gathered together.
//   * dot products reduce across the wave with DPP (row rotations + row
//     broadcasts, no LDS), the result read back with v_readlane into an SGPR,
//     so the sigmoid and gradient scalar are wave-uniform.
//   * updates `row += g * x` (and W[center] += grad, C[ctx] += grad) are
//     either plain stores of the updated row (lock-free Hogwild) or memory-side
//     global_atomic_add_f32 of g * x — the same fp32 rounding as the
//     reference's `row = row + g*x`, but no update is lost when thousands of
//     wavefronts hit one row. Rows inside the "hot" range (frequent words: the
//     low vocab indices, the top of the Huffman tree) take the atomic path;
//     their gathers use L1-bypassing agent-scope loads so a wavefront sees its
//     own atomics. Per-XCD L2s are not coherent inside a launch, so what
//     another XCD wrote may be read late (delayed SGD) but is never lost.
//   * Philox4x32-10 counter-based draws make every random decision a pure
//     function of (key, epoch, sentence, position, slot, k); in Philox mode
//     subsampling decisions for 64 tokens are made at once (one lane per
//     token) and only kept centers are walked. Replay mode consumes the
//     reference's own mt19937 stream recorded on the host, in its draw order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "w2v_limits.hpp"
#include "w2v_philox.hpp"
#include "w2v_rows.hpp"
#include "w2v_wave.hpp"

namespace w2v {

// (kMaxBlock, kMinWaves and the other limits the launch policy shares: w2v_limits.hpp)

struct TrainArgs {
  float* W;
  float* C;
  float* S;             // synapses1
  int64_t pitch;        // row pitch in floats (multiple of 4)
  int32_t dim;          // word_dim
  int32_t window;
  int32_t negative;
  int32_t cbow_mean;
  int32_t iter;
  float init_alpha;
  float min_alpha;
  double train_words;
  const int32_t* ids;
  const int64_t* soff;
  const int64_t* order;  // sentence ids to visit; null = identity over all sentences
  int64_t n_sent;        // entries of `order` to process (work items)
  int64_t n_corpus;      // sentences in the corpus (ids from `order` outside it are skipped)
  const float* keep;
  const uint32_t* table;
  int64_t table_size;
  const uint8_t* codes;
  const int32_t* points;
  const int64_t* coff;
  const uint32_t* replay;      // replay stream
  const int64_t* replay_off;   // per sentence, this epoch
  unsigned long long* words;   // progress (current_words)
  unsigned int* work;          // dequeue head
  unsigned long long* stats;   // centers, contexts, targets, draws, sentences
  uint32_t key0, key1, epoch;
  float fixed_alpha;           // > 0: use instead of the schedule
  // Row bounds are 32-bit (ids are int32): a row index read back from a lane
  // sits in an SGPR, and gfx950's scalar unit compares 32-bit values only
  // (64-bit bounds moved every hot / private test onto the VALU).
  int32_t hot_wc;              // W / C rows [0, hot_wc) update with atomics (shared-negatives: sc1 traffic)
  int32_t hot_s;               // synapses1 rows [hot_s, V-1) update with atomics
  const float* hot_sc;         // per hot node j >= hot_s: its deltas' scale, hot_sc[j - hot_s] (null: 1; hot_node_scales)
  int32_t strict;              // 1: drain own atomics before re-reading (sequential schedule)
  const float* priv_M;         // output matrix whose hottest rows are privatised in LDS (or null)
  int32_t priv_lo;             // privatised rows [priv_lo, priv_lo + priv_n)
  int32_t priv_n;
  float priv_avg;              // > 0: average, not sum, the workgroups' deltas of a privatised row (see flush_private)
  int32_t flush_every;         // the privatised deltas are flushed every this many centers of the workgroup
  const float* ctx_M;          // CBOW: context matrix whose rows [0, ctx_n) are privatised too (or null)
  int32_t ctx_n;
  int32_t ctx_flush_every;     // centers of the workgroup between flushes of the context rows
  int32_t* wide_ids;           // CBOW, window > kMaxWideWindow: per wave a slice of wide_stride ints (cbow_center_huge)
  int64_t wide_stride;
  int64_t item0;               // shared-negatives kernel: work items are order[item0 + k] (or item0 + k)
  int64_t hot_atomic;          // shared-negatives kernel: W / C rows [0, hot_atomic) take memory-side atomic deltas
  int32_t nseg;                // work items per sentence (parallel Philox schedule; 1 = whole sentences)
  int32_t seg_len;             // tokens per item when nseg > 1 (a multiple of 64)
  // Flush scales of the privatised rows (flush_private), computed on the host
  // per launch from the corpus statistics (launch_train, priv_scales): row p of
  // the output range gets priv_sc[p], row p of the context range ctx_sc[p].
  float priv_sc[128];          // kPrivMax
  float ctx_sc[64];            // kCtxMax
};

struct Counters {
  unsigned long long centers = 0, contexts = 0, targets = 0, draws = 0, sentences = 0;
  // Phase timing (diagnostic builds only: make prof, -DW2V_PP_PROF=1;
  // tools/pp_prof.sh): s_memtime since the previous stamp, summed per phase.
#ifdef W2V_PP_PROF
  unsigned long long t = 0, acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  __device__ void stamp(int k) {
    const unsigned long long now = __builtin_amdgcn_s_memtime();
    acc[k] += now - t;
    t = now;
  }
#else
  __device__ void stamp(int) {}
#endif
};

// stats[kNonFinite] counts sigma arguments (row . input dot products) that
// were not finite: the model diverged (w2v_dev_train_epoch returns
// W2V_ERR_DIVERGED). Counted per batch of targets, one atomic per offending
// batch (batch_grad_l).
constexpr int kNonFinite = 5;

// One wave's counts into the launch's statistics (called by one lane).
__device__ __forceinline__ void report_counters(const TrainArgs& a, const Counters& cnt) {
  atomicAdd(&a.stats[0], cnt.centers);
  atomicAdd(&a.stats[1], cnt.contexts);
  atomicAdd(&a.stats[2], cnt.targets);
  atomicAdd(&a.stats[3], cnt.draws);
  atomicAdd(&a.stats[4], cnt.sentences);
}

// The learning rate from the shared word counter (Word2Vec.cpp:379-380),
// floored at min_alpha. The double arithmetic and its operand order are the
// reference's: part of the parity.
__device__ __forceinline__ float scheduled_alpha(const TrainArgs& a) {
  const unsigned long long cw = __hip_atomic_load(a.words, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const float al = (float)(a.init_alpha * (1.0 - 1.0 / a.iter * (double)cw / a.train_words));
  return (a.min_alpha < al) ? al : a.min_alpha;
}

// ---------------------------------------------------------------------------
// LDS-privatised rows of the per-pair kernel (when priv_n + ctx_n > 0), per workgroup:
//   words [0,4) dirty mask of the output rows (2 x 64 bits), [4,8) of the
//   context rows, [8] centers of the workgroup, [9, 13) lock bits of the
//   output rows, [13, 15) of the context rows (priv_lock), then (from
//   kLdsHeaderWords) the pending deltas: priv_n output rows, then ctx_n
//   context rows, NV * 64 floats each. The output range holds at most
//   kPrivMax rows, the context range kCtxMax. The offsets are the kLds*
//   constants of w2v_limits.hpp.
// ---------------------------------------------------------------------------

struct PrivRows {  // one privatised row range [lo, lo + n) of matrix M (n == 0: none)
  float* delta = nullptr;
  unsigned long long* dirty = nullptr;
  unsigned* lock = nullptr;  // one bit per row (priv_lock)
  float* M = nullptr;
  int lo = 0;
  int n = 0;
  bool ctx = false;  // the context range (flush scales a.ctx_sc) or the output range (a.priv_sc)
  __device__ bool has(int row) const { return (unsigned)(row - lo) < (unsigned)n; }  // one scalar compare
};

template <int NV>
__device__ __forceinline__ PrivRows out_rows(const TrainArgs& a, float* lds) {
  PrivRows p;
  if (lds == nullptr || a.priv_n == 0) return p;
  p.dirty = reinterpret_cast<unsigned long long*>(lds + kLdsDirtyOut);
  p.lock = reinterpret_cast<unsigned*>(lds) + kLdsLockOut;
  p.delta = lds + kLdsHeaderWords;
  p.M = const_cast<float*>(a.priv_M);
  p.lo = a.priv_lo;
  p.n = a.priv_n;
  return p;
}

template <int NV>
__device__ __forceinline__ PrivRows ctx_rows(const TrainArgs& a, float* lds) {
  PrivRows p;
  if (lds == nullptr || a.ctx_n == 0) return p;
  p.dirty = reinterpret_cast<unsigned long long*>(lds + kLdsDirtyCtx);
  p.lock = reinterpret_cast<unsigned*>(lds) + kLdsLockCtx;
  p.delta = lds + kLdsHeaderWords + (int64_t)a.priv_n * (NV * kWave);
  p.M = const_cast<float*>(a.ctx_M);
  p.lo = 0;
  p.n = a.ctx_n;
  p.ctx = true;
  return p;
}

// A privatised row's value is the global row plus this workgroup's pending delta.
template <int NV>
__device__ __forceinline__ void priv_read(const PrivRows& pr, int64_t row, int lane, float (&r)[NV]) {
  const float* q = pr.delta + (row - pr.lo) * (NV * kWave) + lane;
#pragma unroll
  for (int v = 0; v < NV; ++v) r[v] += q[kWave * v];
}

// Add delta into the row's pending delta, then mark the row dirty (after the
// adds: a wave's LDS operations are ordered). The add is a ds_read + v_add +
// ds_write under a per-row LDS lock bit that lane 0 takes with one single-lane
// ds_or_rtn_b32 (a wave's own LDS operations execute in order, so the release
// after the writes publishes them); flush_private takes the same lock, so no
// add is lost or flushed twice. Not a float LDS atomic: gfx950 runs ds_add_f32
// one lane at a time, 192 cycles per wave instruction against 10.5 for a
// ds_read + ds_write pair (tools/lds_atomic_bench.hip).
__device__ __forceinline__ void priv_lock(const PrivRows& pr, int p, int lane) {
  unsigned* w = pr.lock + (p >> 5);
  const unsigned bit = 1u << (p & 31);
  for (;;) {
    unsigned old = 0;
    if (lane == 0) old = atomicOr(w, bit);
    old = (unsigned)__builtin_amdgcn_readfirstlane((int)old);
    if (!(old & bit)) break;
    __builtin_amdgcn_s_sleep(1);
  }
  asm volatile("" ::: "memory");  // the row's LDS reads stay after the acquire
}
__device__ __forceinline__ void priv_unlock(const PrivRows& pr, int p, int lane) {
  asm volatile("" ::: "memory");  // the row's LDS writes stay before the release
  if (lane == 0) atomicAnd(pr.lock + (p >> 5), ~(1u << (p & 31)));
}
template <int NV>
__device__ __forceinline__ void priv_add(const PrivRows& pr, int64_t row, int lane, const float (&delta)[NV]) {
  const int64_t p = row - pr.lo;
  float* q = pr.delta + p * (NV * kWave) + lane;
  priv_lock(pr, (int)p, lane);
  float cur[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) cur[v] = q[kWave * v];
#pragma unroll
  for (int v = 0; v < NV; ++v) q[kWave * v] = cur[v] + delta[v];  // padding: 0 + 0
  priv_unlock(pr, (int)p, lane);
  if (lane == 0) atomicOr(pr.dirty + (p >> 6), 1ull << (p & 63));
}

// NS's sigma, Word2Vec.cpp:263: f = 1.0 / (1 + exp(-f)) — a float sum 1 + e
// divided in double and rounded back to the float f. For a float x, the
// double quotient 1.0 / x rounded to float IS the correctly rounded float
// quotient 1.0f / x (double rounding is innocuous for division when the wider
// format has >= 2p + 2 bits, 53 >= 50; checked exhaustively for x in [1,
// 2^30)), and HIP's f32 division is correctly rounded (no fast math): the same
// bits as the f64 division at a fraction of its VALU cost.
__device__ __forceinline__ float ns_sigmoid(float e) { return 1.0f / (1.0f + e); }

// g of one target (Word2Vec.cpp:240-242 HS, :263-264 NS) from its dot product
// fl and its code cl (HS: the Huffman code; NS: 1 - label). Each lane
// evaluates a different target of the batch (batch_grad_l): one exp / division
// sequence for the batch instead of one per target (the same operations on
// the same values: bit-identical).
template <bool HSF>
__device__ __forceinline__ float grad_of(float fl, int cl, float alpha) {
  const float e = expf(-fl);
  if (HSF) {  // the reference's double form (Word2Vec.cpp:240-242)
    const float s = (float)(1.0 / (1.0 + (double)e));
    return (float)((1.0 - (double)cl - (double)s) * (double)alpha);
  }
  return ((float)(1 - cl) - ns_sigmoid(e)) * alpha;
}

// g of a batch in batch_dots' layout: lane L evaluates target batch_target(L)
// (its code, held in lane c0 + t of code_l, fetched with one permute); counts
// the batch's non-finite scores.
template <int N, bool HSF>
__device__ __forceinline__ float batch_grad_l(float fl, int T, int code_l, int c0, float alpha, int lane,
                                              unsigned long long* stats) {
  const int t = batch_target<N>(lane);
  const int cl = __shfl(code_l, (c0 + t) & (kWave - 1));
  if (stats) {
    constexpr int grp = kBatchN<N> == 8 ? 7 : 15;
    const unsigned long long bad = ballot(t < T && (lane & grp) == 0 && !__builtin_isfinite(fl));
    if (bad && lane == 0) atomicAdd(stats + kNonFinite, (unsigned long long)__popcll(bad));
  }
  return grad_of<HSF>(fl, cl, alpha);
}

// A batch of N > 8 targets (the deep HS pipeline of the low-occupancy
// kernel, train_epoch_deep_kernel) in groups of 8: group h's dots are folded
// and evaluated exactly as a batch of 8 would be (batch_dots / batch_grad_l),
// so each target's sum, sigma and g are the bits a batch of <= 8 gives. For N
// <= 8 this is the single batch_dots + batch_grad_l of before.
template <int N, bool HSF>
__device__ __forceinline__ void batch_g(const float (&pd)[N], int T, int code_l, int c0, float alpha, int lane,
                                        unsigned long long* stats, float (&gl)[kGroups<N>]) {
  constexpr int G = kGroupN<N>;
#pragma unroll
  for (int h = 0; h < kGroups<N>; ++h) {
    float q[G];
#pragma unroll
    for (int t = 0; t < G; ++t) q[t] = (8 * h + t < N) ? pd[8 * h + t] : 0.f;
    gl[h] = batch_grad_l<G, HSF>(batch_dots<G>(q, lane), T - 8 * h, code_l, c0 + 8 * h, alpha, lane, stats);
  }
}
// g of target t from batch_g's per-group lanes
template <int N>
__device__ __forceinline__ float batch_gt(const float (&gl)[kGroups<N>], int t) {
  return readlane_f(gl[t / 8], batch_lane<kGroupN<N>>(t % 8));
}

// ---------------------------------------------------------------------------
// The per-target update (Word2Vec.cpp:238-246 HS; :261-268 NS), for up to
// MAXT distinct rows at once. Lane (t0 + t) of row_l / code_l holds target t's
// row and code (HS: Huffman code; NS: 1 - label). Rows are gathered together,
// then updated in target order so grad accumulates in the reference's order.
// Rows in [hot_lo, hot_hi) take the atomic path.
// Not written as hs_gather + hs_score + hs_apply: that keeps every gt[t] live across the batch, and at
// row width 5 took the skip-gram NS kernel from 115 VGPRs and no scratch to 128 VGPRs and 72 B of scratch
// per lane (the other NS kernels spilled too). Here each gt is used at once.
// ---------------------------------------------------------------------------
template <int NV, int MAXT, bool HSF>
__device__ __forceinline__ void apply_targets(float* M, int64_t pitch, int d, int lane, int T, int row_l,
                                              int code_l, int t0, const float (&x)[NV], float (&g)[NV],
                                              float alpha, int64_t hot_lo, int64_t hot_hi, const PrivRows& pr,
                                              unsigned long long* stats) {
  float r[MAXT][NV];
  int rows[MAXT];
  bool hot[MAXT], priv[MAXT];
#pragma unroll
  for (int t = 0; t < MAXT; ++t) {
    rows[t] = readlane_i(row_l, t0 + t);
    priv[t] = pr.has(rows[t]);
    hot[t] = !priv[t] && rows[t] >= hot_lo && rows[t] < hot_hi;
    if (t < T) load_row<NV>(M, rows[t], pitch, lane, hot[t] || priv[t], r[t]);
  }
#pragma unroll
  for (int t = 0; t < MAXT; ++t) {  // privatised rows: global value + this workgroup's pending delta
    if (t < T && priv[t]) {
      priv_read<NV>(pr, rows[t], lane, r[t]);
    }
  }
  float pd[MAXT];
#pragma unroll
  for (int t = 0; t < MAXT; ++t) {
    pd[t] = 0.f;
    if (t < T) {  // the first product starts the sum (0 + p would cost an add per target)
      pd[t] = r[t][0] * x[0];
#pragma unroll
      for (int v = 1; v < NV; ++v) pd[t] += r[t][v] * x[v];
    }
  }
  float g_l[kGroups<MAXT>];
  batch_g<MAXT, HSF>(pd, T, code_l, t0, alpha, lane, stats, g_l);
#pragma unroll
  for (int t = 0; t < MAXT; ++t) {
    if (t < T) {
      const float gt = batch_gt<MAXT>(g_l, t);
      float delta[NV];
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        g[v] += gt * r[t][v];  // grad uses the pre-update row (:244 / :266)
        delta[v] = gt * x[v];
      }
      if (priv[t]) {  // into the workgroup's pending delta; flushed after the center
        priv_add<NV>(pr, rows[t], lane, delta);
      } else if (hot[t]) {
        atomic_add_row<NV>(M, rows[t], pitch, d, lane, delta);
      } else {
#pragma unroll
        for (int v = 0; v < NV; ++v) r[t][v] += delta[v];
        store_row<NV>(M, rows[t], pitch, lane, r[t]);
      }
    }
  }
}

// Move the workgroup's pending deltas of the dirty privatised rows into HBM
// (memory-side float atomics). The dirty mask is taken with an atomic swap and
// each row's delta under the row's lock, so an add racing the flush from
// another wave of the workgroup is neither lost nor flushed twice (its dirty
// bit is set after its adds and survives until the next flush).
//
// Scale: a row that n workgroups update within one flush interval receives
// the mean of their deltas scaled to at most priv_avg concurrent
// contributions (local SGD on the few rows every wave updates; without it
// ~10^4 concurrent stale updates of those rows diverge). n is the expected
// count, computed on the host from the corpus statistics (launch_train:
// n = workgroups x P(a workgroup touches the row in flush_every centers)), so
// the scale is a fixed function of the row's frequency rank, not of the
// schedule (a.priv_sc / a.ctx_sc; 1 when priv_avg == 0).
template <int NV>
__device__ __forceinline__ void flush_private(const TrainArgs& a, const PrivRows& pr, int lane) {
  if (pr.n == 0) return;
  unsigned long long mw[2] = {0ull, 0ull};
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    unsigned long long m = 0;
    if (lane == 0 && 64 * w < pr.n) m = atomicExch(pr.dirty + w, 0ull);
    mw[w] = uniform_u64(m);
  }
  for (int w = 0; w < 2; ++w)
  for (unsigned long long m = mw[w]; m;) {
    const int p = 64 * w + __builtin_ctzll(m);
    m &= m - 1;
    const float sc = pr.ctx ? a.ctx_sc[p & (kCtxMax - 1)] : a.priv_sc[p];
    float* q = pr.delta + p * (NV * kWave) + lane;
    float* dst = pr.M + (pr.lo + p) * a.pitch + lane;
    float val[NV];
    priv_lock(pr, p, lane);  // take the row under its lock (priv_add)
#pragma unroll
    for (int v = 0; v < NV; ++v) val[v] = q[kWave * v];
#pragma unroll
    for (int v = 0; v < NV; ++v) q[kWave * v] = 0.0f;
    priv_unlock(pr, p, lane);
#pragma unroll
    for (int v = 0; v < NV; ++v)
      if (val[v] != 0.0f)  // 0 past word_dim: skipped
        (void)__hip_atomic_fetch_add(dst + kWave * v, val[v] * sc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// HS on the path of `word` (synapses1 rows), software-pipelined: the path's
// nodes are known up front and distinct, so batch b + 1's rows are gathered
// BEFORE batch b's updates are issued. vmcnt retires in order on gfx950, so a
// gather issued after a batch's stores and memory-side atomics would wait for
// all of them (~3000 cycles per atomic with every CU issuing); issued before
// them it waits only for its own loads. Same arithmetic, same order of the
// gradient sum as apply_targets (target order), so the sequential schedule
// stays bit-exact.
template <int NV, int MT>
__device__ __forceinline__ void hs_gather(const TrainArgs& a, int T, int row_l, int t0, const PrivRows& pr, int lane,
                                          float (&r)[MT][NV]) {
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    if (t < T) {
      const int row = readlane_i(row_l, t0 + t);
      load_row<NV>(a.S, row, a.pitch, lane, pr.has(row) || row >= a.hot_s, r[t]);
    }
  }
}

// Scores of a gathered batch: privatised rows get the pending delta, then
// g += gt * row (pre-update row, :244) in target order; returns gt per target.
template <int NV, int MT>
__device__ __forceinline__ void hs_score(const TrainArgs& a, int T, int row_l, int code_l, int t0, const PrivRows& pr,
                                         int lane, const float (&x)[NV], float (&g)[NV], float alpha,
                                         float (&r)[MT][NV], float (&gt)[MT]) {
#pragma unroll
  for (int t = 0; t < MT; ++t)
    if (t < T) {
      const int row = readlane_i(row_l, t0 + t);
      if (pr.has(row)) priv_read<NV>(pr, row, lane, r[t]);
    }
  float pd[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    pd[t] = 0.f;
    if (t < T) {  // the first product starts the sum (0 + p would cost an add per target)
      pd[t] = r[t][0] * x[0];
#pragma unroll
      for (int v = 1; v < NV; ++v) pd[t] += r[t][v] * x[v];
    }
  }
  float g_l[kGroups<MT>];
  batch_g<MT, true>(pd, T, code_l, t0, alpha, lane, a.stats, g_l);
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    gt[t] = 0.f;
    if (t < T) {
      gt[t] = batch_gt<MT>(g_l, t);
#pragma unroll
      for (int v = 0; v < NV; ++v) g[v] += gt[t] * r[t][v];
    }
  }
}

// The updates of a scored batch: LDS delta (privatised), memory-side atomic
// (hot), or the updated row stored (Hogwild).
template <int NV, int MT>
__device__ __forceinline__ void hs_apply(const TrainArgs& a, int T, int row_l, int t0, const PrivRows& pr, int lane,
                                         const float (&x)[NV], float (&r)[MT][NV], const float (&gt)[MT]) {
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    if (t < T) {
      const int row = readlane_i(row_l, t0 + t);
      float delta[NV];
#pragma unroll
      for (int v = 0; v < NV; ++v) delta[v] = gt[t] * x[v];
      if (pr.has(row)) {
        priv_add<NV>(pr, row, lane, delta);
      } else if (row >= a.hot_s) {
        if (a.hot_sc) {  // damped to the hot-node average (wave-uniform row: one scalar load)
          const float s = a.hot_sc[row - a.hot_s];
#pragma unroll
          for (int v = 0; v < NV; ++v) delta[v] *= s;
        }
        atomic_add_row<NV>(a.S, row, a.pitch, a.dim, lane, delta);
      } else {
#pragma unroll
        for (int v = 0; v < NV; ++v) r[t][v] += delta[v];
        store_row<NV>(a.S, row, a.pitch, lane, r[t]);
      }
    }
  }
}

template <int NV, int MAXT>
__device__ __forceinline__ void hs_word(const TrainArgs& a, int word, int lane, const float (&x)[NV],
                                        float (&g)[NV], float alpha, Counters& cnt, float* lds) {
  constexpr int MT = MAXT / 2 > 0 ? MAXT / 2 : 1;  // two buffers of MT rows: the same registers as one of MAXT
  const PrivRows pr = (a.priv_M == a.S) ? out_rows<NV>(a, lds) : PrivRows();
  const int64_t cb = a.coff[word];
  const int L = (int)(a.coff[word + 1] - cb);
  for (int c0 = 0; c0 < L; c0 += kWave) {
    const int rem = min(kWave, L - c0);
    const int pt_l = (lane < rem) ? a.points[cb + c0 + lane] : 0;
    const int cd_l = (lane < rem) ? (int)a.codes[cb + c0 + lane] : 0;
    float ra[MT][NV], rb[MT][NV], gt[MT];
    if (a.strict) drain_vmem();
    hs_gather<NV, MT>(a, min(MT, rem), pt_l, 0, pr, lane, ra);
    for (int t0 = 0; t0 < rem; t0 += 2 * MT) {
      const int Ta = min(MT, rem - t0), Tb = min(MT, rem - t0 - MT);  // Tb <= 0: no second batch
      hs_score<NV, MT>(a, Ta, pt_l, cd_l, t0, pr, lane, x, g, alpha, ra, gt);
      if (Tb > 0) hs_gather<NV, MT>(a, Tb, pt_l, t0 + MT, pr, lane, rb);
      hs_apply<NV, MT>(a, Ta, pt_l, t0, pr, lane, x, ra, gt);
      if (Tb > 0) {
        hs_score<NV, MT>(a, Tb, pt_l, cd_l, t0 + MT, pr, lane, x, g, alpha, rb, gt);
        const int Tn = min(MT, rem - t0 - 2 * MT);
        if (Tn > 0) hs_gather<NV, MT>(a, Tn, pt_l, t0 + 2 * MT, pr, lane, ra);
        hs_apply<NV, MT>(a, Tb, pt_l, t0 + MT, pr, lane, x, rb, gt);
      }
    }
    cnt.targets += (unsigned long long)rem;
  }
}

// The T targets of tgt_l / code_l, MAXT rows per batch.
template <int NV, int MAXT>
__device__ __forceinline__ void apply_list(const TrainArgs& a, float* M, int T, int tgt_l, int code_l,
                                           const float (&x)[NV], float (&g)[NV], float alpha, Counters& cnt,
                                           const PrivRows& pr) {
  for (int t0 = 0; t0 < T; t0 += MAXT) {
    if (a.strict) drain_vmem();
    apply_targets<NV, MAXT, false>(M, a.pitch, a.dim, lane_id(), min(MAXT, T - t0), tgt_l, code_l, t0, x, g, alpha,
                                   0, a.hot_wc, pr, a.stats);
  }
  cnt.targets += (unsigned long long)T;
}

// NS with positive `word` against `negw_l` lanes [base, base + neg).
template <int NV, int MAXT>
__device__ __forceinline__ void ns_word(const TrainArgs& a, float* M, int word, int negw_l, int base, int lane,
                                        const float (&x)[NV], float (&g)[NV], float alpha, Counters& cnt,
                                        float* lds) {
  const PrivRows pr = (a.priv_M == M) ? out_rows<NV>(a, lds) : PrivRows();
  int tgt_l;
  const int T = ns_targets(a.negative, word, negw_l, base, lane, tgt_l);
  apply_list<NV, MAXT>(a, M, T, tgt_l, (lane == 0) ? 0 : 1, x, g, alpha, cnt, pr);
}

// ---------------------------------------------------------------------------
// NS with more draws than a wave has lanes (negative >= 64; the reference
// takes any value, Word2Vec.cpp:254-255). The targets keep the set semantics
// and the order of ns_targets — the positive, then the first occurrence of
// every negative that differs from it, in draw order — taken 64 draws at a
// time: chunk ch holds draws k = 64 ch + lane; a draw is a duplicate if an
// earlier draw of its chunk or any draw of an earlier chunk (drawn again: the
// same counter gives the same word) is the same word. Each chunk's new
// targets are applied before the next chunk's are found (a duplicate test
// needs only the words, not the rows).
// ---------------------------------------------------------------------------
template <int NV, int MAXT, bool REPLAY>
__device__ __forceinline__ void ns_word_many(const TrainArgs& a, float* M, int word, uint32_t s, uint32_t i, int slot,
                                          int lane, const float (&x)[NV], float (&g)[NV], float alpha,
                                          Counters& cnt, float* lds, const uint32_t*& rp) {
  const PrivRows pr = (a.priv_M == M) ? out_rows<NV>(a, lds) : PrivRows();
  const int neg = a.negative;
  const int nch = (neg + kWave - 1) / kWave;
  apply_list<NV, MAXT>(a, M, 1, word, 0, x, g, alpha, cnt, pr);  // the positive (label 1)
  for (int ch = 0; ch < nch; ++ch) {
    const int w = draw_chunk<REPLAY>(a, s, i, slot, ch, lane, rp);
    bool dup = (w < 0) || (w == word);
    for (int j = 0; j < kWave - 1; ++j) {
      const int v = readlane_i(w, j);
      dup = dup || (lane > j && v == w);
    }
    for (int c2 = 0; c2 < ch; ++c2) {
      const int wp = draw_chunk<REPLAY>(a, s, i, slot, c2, lane, rp);
      for (int j = 0; j < kWave; ++j) dup = dup || (readlane_i(wp, j) == w);
    }
    unsigned long long uniq = ballot(!dup);
    int tgt_l = 0, m = 0;
    while (uniq) {
      const int b = __builtin_ctzll(uniq);
      uniq &= uniq - 1;
      const int v = readlane_i(w, b);
      if (lane == m) tgt_l = v;
      ++m;
    }
    if (m > 0) apply_list<NV, MAXT>(a, M, m, tgt_l, 1, x, g, alpha, cnt, pr);  // negatives (label 0)
  }
  cnt.draws += (unsigned long long)neg;
  if (REPLAY) rp += neg;
}

// ---------------------------------------------------------------------------
// Skip-gram center (Word2Vec.cpp:329-351) with its window [lo, hi).
// ---------------------------------------------------------------------------
template <int NV, int MAXT, bool HS, bool NS, bool REPLAY>
__device__ __forceinline__ void sg_center(const TrainArgs& a, float* lds, const int32_t* sent, int len, int i, int c, int rw,
                                          uint32_t s, float alpha, const uint32_t*& rp, Counters& cnt, int lane) {
  const int lo = max(0, i - a.window + rw), hi = min(len, i + a.window + 1 - rw);
  const int span = hi - lo;
  // An empty window (a one-token sentence) trains nothing and is not counted,
  // as for CBOW. Its W.row(center) += 0 must not run either: on a plain
  // (Hogwild) row it is a load and a store of the unchanged row, and a store
  // that lands after another wave's update of that row takes the update back.
  if (span <= 1) return;
  const bool hot_c = c < a.hot_wc;
  float x[NV], g[NV];
  if (a.strict) drain_vmem();
  load_row<NV>(a.W, c, a.pitch, lane, hot_c, x);
#pragma unroll
  for (int v = 0; v < NV; ++v) g[v] = 0.f;
  const int ctx_l = (lane < span) ? sent[lo + lane] : 0;
  cnt.centers += 1;
  cnt.contexts += (unsigned long long)(span - 1);
  const int nctx = span - 1;
  const int neg = a.negative;
  const int G = NS ? max(1, kWave / max(neg, 1)) : 1;
  int negw_l = 0;
  int slot = 0;
  for (int j = lo; j < hi; ++j) {
    if (j == i) continue;
    const int w = (j - lo < kWave) ? readlane_i(ctx_l, j - lo) : uniform_i(sent[j]);  // window > 31: span > 64
    if (HS) hs_word<NV, MAXT>(a, w, lane, x, g, alpha, cnt, lds);
    if (NS && neg >= kWave) {
      ns_word_many<NV, MAXT, REPLAY>(a, a.C, w, s, (uint32_t)i, slot, lane, x, g, alpha, cnt, lds, rp);
    } else if (NS) {
      const int gs = slot % G;
      if (gs == 0) {
        const int nd = min(G, nctx - slot) * neg;
        negw_l = draw_negatives<REPLAY>(a, s, (uint32_t)i, slot, nd, lane, rp);
        cnt.draws += (unsigned long long)nd;
      }
      ns_word<NV, MAXT>(a, a.C, w, negw_l, gs * neg, lane, x, g, alpha, cnt, lds);
    }
    ++slot;
  }
  cnt.stamp(3);
  add_to_row<NV>(a.W, c, hot_c, a.pitch, a.dim, lane, g);  // W.row(center) += neu1_grad (:351)
  cnt.stamp(4);
}

// ---------------------------------------------------------------------------
// CBOW center (Word2Vec.cpp:286-315): the unique context ids in ascending
// order (std::set), then cbow_tail. row_of(r) is the r-th of them.
// ---------------------------------------------------------------------------
template <int NV, int MAXT, bool HS, bool NS, bool REPLAY, class RowOf>
__device__ __forceinline__ void cbow_tail(const TrainArgs& a, float* lds, int i, int c, int n, int U, RowOf row_of,
                                         uint32_t s, float alpha, const uint32_t*& rp, Counters& cnt, int lane) {
  cnt.centers += 1;
  cnt.contexts += (unsigned long long)U;
  float h[NV], g[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) h[v] = g[v] = 0.f;
  const PrivRows cx = ctx_rows<NV>(a, lds);  // the hottest context rows: global value + pending delta
  if (a.strict) drain_vmem();
  for (int r0 = 0; r0 < U; r0 += MAXT) {
    float rr[MAXT][NV];
#pragma unroll
    for (int t = 0; t < MAXT; ++t)
      if (r0 + t < U) {
        const int row = row_of(r0 + t);
        load_row<NV>(a.C, row, a.pitch, lane, row < a.hot_wc || cx.has(row), rr[t]);
      }
#pragma unroll
    for (int t = 0; t < MAXT; ++t)
      if (r0 + t < U) {
        const int row = row_of(r0 + t);
        if (cx.has(row)) priv_read<NV>(cx, row, lane, rr[t]);
#pragma unroll
        for (int v = 0; v < NV; ++v) h[v] += rr[t][v];
      }
  }
  const float nf = (float)n;
  if (a.cbow_mean) {
#pragma unroll
    for (int v = 0; v < NV; ++v) h[v] /= nf;
  }
  cnt.stamp(2);
  if (HS) hs_word<NV, MAXT>(a, c, lane, h, g, alpha, cnt, lds);
  if (NS && a.negative >= kWave) {
    ns_word_many<NV, MAXT, REPLAY>(a, a.W, c, s, (uint32_t)i, 0, lane, h, g, alpha, cnt, lds, rp);
  } else if (NS) {
    const int nd = a.negative;
    const int negw_l = draw_negatives<REPLAY>(a, s, (uint32_t)i, 0, nd, lane, rp);
    cnt.draws += (unsigned long long)nd;
    ns_word<NV, MAXT>(a, a.W, c, negw_l, 0, lane, h, g, alpha, cnt, lds);
  }
  cnt.stamp(3);
  if (a.cbow_mean) {
#pragma unroll
    for (int v = 0; v < NV; ++v) g[v] /= nf;
  }
  // C.row(id) += neu1_grad for every unique id (:315). The plain (Hogwild)
  // rows of a batch are all gathered before any of them is stored: with
  // in-order vmcnt a row-by-row read-modify-write would make each gather wait
  // for the previous row's store.
  for (int r0 = 0; r0 < U; r0 += MAXT) {
    float cur[MAXT][NV];
#pragma unroll
    for (int t = 0; t < MAXT; ++t)
      if (r0 + t < U) {
        const int row = row_of(r0 + t);
        if (!cx.has(row) && row >= a.hot_wc) load_row<NV>(a.C, row, a.pitch, lane, false, cur[t]);
      }
#pragma unroll
    for (int t = 0; t < MAXT; ++t)
      if (r0 + t < U) {
        const int row = row_of(r0 + t);
        if (cx.has(row)) {
          priv_add<NV>(cx, row, lane, g);
        } else if (row < a.hot_wc) {
          atomic_add_row<NV>(a.C, row, a.pitch, a.dim, lane, g);
        } else {
#pragma unroll
          for (int v = 0; v < NV; ++v) cur[t][v] += g[v];
          store_row<NV>(a.C, row, a.pitch, lane, cur[t]);
        }
      }
  }
  cnt.stamp(4);
}

template <int NV, int MAXT, bool HS, bool NS, bool REPLAY>
__device__ __forceinline__ void cbow_center(const TrainArgs& a, float* lds, const int32_t* sent, int len, int i, int c, int rw,
                                            uint32_t s, float alpha, const uint32_t*& rp, Counters& cnt, int lane) {
  const int lo = max(0, i - a.window + rw), hi = min(len, i + a.window + 1 - rw);
  const int n = hi - lo - 1;  // neu1_num, positional
  if (n <= 0) return;
  const int span = hi - lo;
  const int me = i - lo;
  const bool valid = lane < span && lane != me;
  const int id = valid ? sent[lo + lane] : 0;
  // std::set semantics: unique ids, visited in ascending order.
  bool dup = !valid;
  for (int j = 0; j < span; ++j) {
    const int v = readlane_i(id, j);
    dup = dup || (j != me && j < lane && v == id);
  }
  const unsigned long long uniq = ballot(!dup);
  const int U = __popcll(uniq);
  int rank = 0;
  {
    unsigned long long m = uniq;
    while (m) {
      const int b = __builtin_ctzll(m);
      m &= m - 1;
      rank += (readlane_i(id, b) < id) ? 1 : 0;
    }
  }
  int sid = 0;
  {
    unsigned long long m = uniq;
    while (m) {
      const int b = __builtin_ctzll(m);
      m &= m - 1;
      const int v = readlane_i(id, b), rk = readlane_i(rank, b);
      if (lane == rk) sid = v;
    }
  }
  cnt.stamp(1);
  cbow_tail<NV, MAXT, HS, NS, REPLAY>(a, lds, i, c, n, U, [&](int r) { return readlane_i(sid, r); }, s, alpha, rp,
                                      cnt, lane);
}

// CBOW center for windows wider than a wave (2 * window + 1 > 64, window <=
// 32 * NCH - 1): the same set semantics and visiting order as cbow_center, the
// span's positions held NCH per lane (position lo + 64 ch + lane).
template <int NV, int MAXT, bool HS, bool NS, bool REPLAY, int NCH>
__device__ __forceinline__ void cbow_center_wide(const TrainArgs& a, float* lds, const int32_t* sent, int len, int i,
                                                 int c, int rw, uint32_t s, float alpha, const uint32_t*& rp,
                                                 Counters& cnt, int lane) {
  const int lo = max(0, i - a.window + rw), hi = min(len, i + a.window + 1 - rw);
  const int n = hi - lo - 1;
  if (n <= 0) return;
  const int span = hi - lo;
  const int me = i - lo;
  int id[NCH];
  bool dup[NCH];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const int p = kWave * ch + lane;
    const bool valid = p < span && p != me;
    id[ch] = valid ? sent[lo + p] : 0;
    dup[ch] = !valid;
  }
  for (int j = 0; j < span; ++j) {  // a later position repeating an earlier valid id is a duplicate
    if (j == me) continue;
    const int v = pick_lane<NCH>(id, j);
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) dup[ch] = dup[ch] || (j < kWave * ch + lane && v == id[ch]);
  }
  unsigned long long uq[NCH];
  int U = 0;
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    uq[ch] = ballot(!dup[ch]);
    U += __popcll(uq[ch]);
  }
  int rank[NCH], sid[NCH];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) rank[ch] = sid[ch] = 0;
#pragma unroll
  for (int c2 = 0; c2 < NCH; ++c2) {
    unsigned long long m = uq[c2];
    while (m) {
      const int b = __builtin_ctzll(m);
      m &= m - 1;
      const int v = readlane_i(id[c2], b);
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) rank[ch] += (v < id[ch]) ? 1 : 0;
    }
  }
#pragma unroll
  for (int c2 = 0; c2 < NCH; ++c2) {
    unsigned long long m = uq[c2];
    while (m) {
      const int b = __builtin_ctzll(m);
      m &= m - 1;
      const int v = readlane_i(id[c2], b), rk = readlane_i(rank[c2], b);
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch)
        if (ch == (rk >> 6) && lane == (rk & (kWave - 1))) sid[ch] = v;
    }
  }
  cbow_tail<NV, MAXT, HS, NS, REPLAY>(a, lds, i, c, n, U, [&](int r) { return pick_lane<NCH>(sid, r); }, s, alpha,
                                      rp, cnt, lane);
}

// CBOW center for windows past kMaxWideWindow (the reference takes any window,
// Word2Vec.cpp:285): the same set semantics and
// ascending visiting order as cbow_center, with the span read from the
// sentence 64 positions at a time. Pass 1 marks each position that is not a
// repeat of an earlier valid one (a scalar walk over the earlier positions)
// and keeps each chunk's unique mask in this wave's slice of a global scratch;
// pass 2 ranks every unique id among all of them (the count of smaller ones)
// and writes it to slot `rank`, so the slice holds the ids in ascending order
// for cbow_tail. O(span^2 / 64) scalar steps per center: the price of a window
// no register set holds.
template <int NV, int MAXT, bool HS, bool NS, bool REPLAY>
__device__ __forceinline__ void cbow_center_huge(const TrainArgs& a, float* lds, const int32_t* sent, int len, int i,
                                                 int c, int rw, uint32_t s, float alpha, const uint32_t*& rp,
                                                 Counters& cnt, int lane) {
  const int lo = max(0, i - a.window + rw), hi = min(len, i + a.window + 1 - rw);
  const int n = hi - lo - 1;
  if (n <= 0) return;
  const int span = hi - lo;
  const int me = i - lo;
  const int nch = (span + kWave - 1) / kWave;
  const int64_t wave = (int64_t)blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
  int32_t* ids_out = a.wide_ids + wave * a.wide_stride;
  int32_t* masks = ids_out + 2 * (int64_t)a.window;  // 2 ints per chunk
  int U = 0;
  for (int ch = 0; ch < nch; ++ch) {
    const int p = kWave * ch + lane;
    const bool valid = p < span && p != me;
    const int id = valid ? sent[lo + p] : -1;
    bool dup = !valid;
    const int jmax = min(span, kWave * ch + kWave - 1);
    for (int j = 0; j < jmax; ++j) {
      if (j == me) continue;
      const int v = uniform_i(sent[lo + j]);
      dup = dup || (j < p && v == id);
    }
    const unsigned long long uq = ballot(!dup);
    U += __popcll(uq);
    if (lane == 0) {
      masks[2 * ch] = (int32_t)(uint32_t)uq;
      masks[2 * ch + 1] = (int32_t)(uint32_t)(uq >> 32);
    }
  }
  drain_vmem();
  const auto mask_of = [&](int ch) {  // chunk ch's unique mask, as pass 1 left it
    return ((unsigned long long)(uint32_t)__hip_atomic_load(masks + 2 * ch + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) << 32) |
           (uint32_t)__hip_atomic_load(masks + 2 * ch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  for (int ch = 0; ch < nch; ++ch) {
    const int p = kWave * ch + lane;
    const int id = (p < span) ? sent[lo + p] : -1;
    const bool uniq = (mask_of(ch) >> lane) & 1ull;
    int rank = 0;
    for (int c2 = 0; c2 < nch; ++c2) {
      unsigned long long m = uniform_u64(mask_of(c2));
      while (m) {
        const int b = __builtin_ctzll(m);
        m &= m - 1;
        rank += (uniform_i(sent[lo + kWave * c2 + b]) < id) ? 1 : 0;
      }
    }
    if (uniq) ids_out[rank] = id;
  }
  drain_vmem();
  cbow_tail<NV, MAXT, HS, NS, REPLAY>(
      a, lds, i, c, n, U,
      [&](int r) { return uniform_i(__hip_atomic_load(ids_out + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)); },
      s, alpha, rp, cnt, lane);
}

template <int NV, int MAXT, bool CBOW, bool HS, bool NS, bool REPLAY, bool WIDE>
__device__ __forceinline__ void center(const TrainArgs& a, float* lds, const int32_t* sent, int len, int i, int c,
                                       int rw, uint32_t s, float alpha, const uint32_t*& rp, Counters& cnt,
                                       int lane) {
  cnt.stamp(0);
  if (CBOW && WIDE && a.window > kMaxWideWindow)
    cbow_center_huge<NV, MAXT, HS, NS, REPLAY>(a, lds, sent, len, i, c, rw, s, alpha, rp, cnt, lane);
  else if (CBOW && WIDE)
    cbow_center_wide<NV, MAXT, HS, NS, REPLAY, kWideChunks>(a, lds, sent, len, i, c, rw, s, alpha, rp, cnt, lane);
  else if (CBOW)
    cbow_center<NV, MAXT, HS, NS, REPLAY>(a, lds, sent, len, i, c, rw, s, alpha, rp, cnt, lane);
  else
    sg_center<NV, MAXT, HS, NS, REPLAY>(a, lds, sent, len, i, c, rw, s, alpha, rp, cnt, lane);
  if (lds != nullptr) {
    // Bounded staleness with aggregation: the workgroup's waves share one
    // center count, and the wave that completes every flush_every-th center
    // drains the deltas all of them accumulated (one atomic per dirty row
    // instead of one per update and wave).
    unsigned* done = reinterpret_cast<unsigned*>(lds) + kLdsCenters;
    unsigned n = 0;
    if (lane == 0) n = atomicAdd(done, 1u) + 1u;
    n = (unsigned)__builtin_amdgcn_readfirstlane((int)n);
    cnt.stamp(7);
    if (a.priv_n > 0 && n % (unsigned)a.flush_every == 0u) flush_private<NV>(a, out_rows<NV>(a, lds), lane);
    cnt.stamp(5);
    if (a.ctx_n > 0 && n % (unsigned)a.ctx_flush_every == 0u) flush_private<NV>(a, ctx_rows<NV>(a, lds), lane);
    cnt.stamp(6);
  }
}

// ---------------------------------------------------------------------------
// The epoch kernel: wavefronts dequeue sentences (Word2Vec.cpp:375-394).
// ---------------------------------------------------------------------------
template <int NV, int MAXT, bool CBOW, bool HS, bool NS, bool REPLAY, bool WIDE>
__device__ __forceinline__ void train_epoch(const TrainArgs& a) {
  extern __shared__ float w2v_lds[];
  const int lane = lane_id();
  float* lds = (a.priv_n + a.ctx_n) > 0 ? w2v_lds : nullptr;
  if (lds) {
    const int64_t words = kLdsHeaderWords + (int64_t)(a.priv_n + a.ctx_n) * (NV * kWave);
    for (int64_t k = threadIdx.x; k < words; k += blockDim.x) lds[k] = 0.0f;
    __syncthreads();
  }
  Counters cnt;
#ifdef W2V_PP_PROF
  cnt.t = __builtin_amdgcn_s_memtime();
#endif
  float alpha = a.init_alpha;
  bool first = true;
  const uint32_t wmax = (uint32_t)(a.window < 1 ? 1 : a.window);
  // A work item is one sentence, or (nseg > 1: parallel Philox schedule) one
  // seg_len-token segment of it, so that the last round of a launch is short
  // (a few thousand waves, ~1000-token sentences: whole-sentence items leave
  // most waves idle while the last sentences finish). Segment g of a sentence
  // trains the centers [g * seg_len, (g + 1) * seg_len) with the whole sentence
  // as their windows, exactly what the whole-sentence wave does for them.
  const uint32_t nseg = (uint32_t)(a.nseg > 1 ? a.nseg : 1);
  const int64_t n_items = a.n_sent * (int64_t)nseg;
  for (;;) {
    uint32_t kk = 0;
    if (lane == 0) kk = atomicAdd(a.work, 1u);
    kk = (uint32_t)uniform_i((int)kk);
    if ((int64_t)kk >= n_items) break;
    const uint32_t k = kk / nseg, seg = kk - k * nseg;
    const int64_t s = a.order ? a.order[k] : (int64_t)k;
    if (s < 0 || s >= a.n_corpus) continue;  // a caller-supplied device order is not host-checked
    if (a.fixed_alpha > 0.0f) {
      alpha = a.fixed_alpha;
    } else if (first || (k % 10u) == 0u) {
      alpha = scheduled_alpha(a);
      first = false;
    }
    const int64_t base = a.soff[s];
    const int len = (int)(a.soff[s + 1] - base);
    const int32_t* sent = a.ids + base;
    const uint32_t* rp = nullptr;
    if (REPLAY) {
      rp = a.replay + a.replay_off[s];
      for (int i = 0; i < len; ++i) {
        const int c = sent[i];
        const float u = __int_as_float((int)rp[0]);
        ++rp;
        if (a.keep[c] < u) continue;
        const int rw = (int)rp[0];
        ++rp;
        center<NV, MAXT, CBOW, HS, NS, REPLAY, WIDE>(a, lds, sent, len, i, c, rw, (uint32_t)s, alpha, rp, cnt, lane);
      }
    } else {
      const int seg_lo = nseg > 1 ? min(len, (int)seg * a.seg_len) : 0;
      const int seg_hi = nseg > 1 ? min(len, seg_lo + a.seg_len) : len;
      for (int i0 = seg_lo; i0 < seg_hi; i0 += kWave) {
        const int ii = i0 + lane;
        const bool in = ii < seg_hi;
        const int c_l = in ? sent[ii] : 0;
        const float p_l = in ? a.keep[c_l] : 0.f;
        float u_l;
        int rw_l;
        subsample_draw(a, (uint32_t)s, (uint32_t)ii, wmax, u_l, rw_l);
        unsigned long long kept = ballot(in && !(p_l < u_l));
        while (kept) {
          const int b = __builtin_ctzll(kept);
          kept &= kept - 1;
          const int c = readlane_i(c_l, b), rw = readlane_i(rw_l, b);
          center<NV, MAXT, CBOW, HS, NS, REPLAY, WIDE>(a, lds, sent, len, i0 + b, c, rw, (uint32_t)s, alpha, rp,
                                                        cnt, lane);
        }
      }
    }
    if (REPLAY || nseg == 1) {
      if (lane == 0) atomicAdd(a.words, (unsigned long long)len);
      cnt.sentences += 1;
    } else {
      const int seg_lo = min(len, (int)seg * a.seg_len), seg_hi = min(len, seg_lo + a.seg_len);
      if (lane == 0 && seg_hi > seg_lo) atomicAdd(a.words, (unsigned long long)(seg_hi - seg_lo));
      cnt.sentences += (seg == 0) ? 1 : 0;
    }
  }
  flush_private<NV>(a, out_rows<NV>(a, lds), lane);
  flush_private<NV>(a, ctx_rows<NV>(a, lds), lane);
#ifdef W2V_PP_PROF
  cnt.stamp(0);
  if (lane == 0 && (threadIdx.x / kWave) % 4 == 0 && (blockIdx.x == 0 || blockIdx.x == gridDim.x / 2))
    printf("PPPROF block %u wave %d centers %llu: %llu %llu %llu %llu %llu %llu %llu %llu\n", blockIdx.x,
           (int)(threadIdx.x / kWave), cnt.centers, cnt.acc[0], cnt.acc[1], cnt.acc[2], cnt.acc[3], cnt.acc[4],
           cnt.acc[5], cnt.acc[6], cnt.acc[7]);
#endif
  if (lane == 0) report_counters(a, cnt);
}

template <int NV, int MAXT, bool CBOW, bool HS, bool NS, bool REPLAY, bool WIDE>
__global__ __launch_bounds__(kMaxBlock<NV>, kMinWaves<NV>) void train_epoch_kernel(TrainArgs a) {
  train_epoch<NV, MAXT, CBOW, HS, NS, REPLAY, WIDE>(a);
}

// The same epoch for a launch that runs few waves (round 6: large-vocabulary
// HS capped at kHsRootPressure root updates in flight, 1-6 waves per CU):
// workgroups of <= 4 waves and a 256-VGPR budget (2 waves per SIMD), so a
// Huffman path is gathered kDeepMaxT / 2 nodes at a time instead of 4 —
// a wave that has the CU to itself is latency-bound on its path's round
// trips. Same arithmetic in the same order as train_epoch_kernel.
template <int NV>
constexpr int kDeepMaxT = NV <= 2 ? 32 : NV <= 4 ? 24 : NV <= 6 ? 16 : NV <= 16 ? 8 : 4;
template <int NV, int MAXT, bool CBOW, bool HS, bool NS, bool REPLAY, bool WIDE>
__global__ __launch_bounds__(kDeepBlock, 2) void train_epoch_deep_kernel(TrainArgs a) {
  train_epoch<NV, MAXT, CBOW, HS, NS, REPLAY, WIDE>(a);
}

// Sequential target updates for w2v_dev_apply_rows (one wave): target t is
// row t of M, applied in order (rows are distinct; plain read-modify-write).
template <int NV>
__global__ __launch_bounds__(64) void apply_rows_kernel(float* M, int64_t pitch, int d, const float* x_in,
                                                        float* grad_io, const uint8_t* codes, int n, float alpha,
                                                        int hs_form) {
  const int lane = lane_id();
  float x[NV], g[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int e = lane + kWave * v;
    x[v] = (e < d) ? x_in[e] : 0.f;
    g[v] = (e < d) ? grad_io[e] : 0.f;
  }
  for (int t = 0; t < n; ++t) {
    const int code = (int)codes[t];
    if (hs_form)
      apply_targets<NV, 1, true>(M, pitch, d, lane, 1, t, code, 0, x, g, alpha, 0, 0, PrivRows(), nullptr);
    else
      apply_targets<NV, 1, false>(M, pitch, d, lane, 1, t, code, 0, x, g, alpha, 0, 0, PrivRows(), nullptr);
  }
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int e = lane + kWave * v;
    if (e < d) grad_io[e] = g[v];
  }
}

}  // namespace w2v
