// w2v_nn.hip — nearest-neighbour and analogy queries on the GPU behind the
// C-ABI (include/w2v_dev.h, w2v_nn_*): cosine scores of a block of queries
// against every candidate row as an exact-f32 GEMM on the matrix cores, with
// the top-k fused behind it, so the queries x vocabulary score matrix never
// reaches HBM.
//
// An index holds a row-major fp32 matrix (owned: a copy of the caller's rows at
// a pitch of dim rounded up to 16, zero padding; attached: a handle's resident
// W or C at its own pitch), inv_norm[r] = 1 / max(|row r|, 1e-12) and scratch.
//
// Kernels:
//   nn_norm_kernel     one wavefront per row: whole-row 16-B loads, DPP sum.
//   nn_query_kernel    one wavefront per query: the by-row form's
//                      q = sum_t w_t row[id_t] inv_norm[id_t] (or the caller's
//                      vector), scaled to unit length, into the padded buffer.
//   nn_score_kernel    the hot path. A workgroup of 4 wavefronts owns 128
//                      queries (two 16-query tiles per wave, their A fragments
//                      resident in registers; one tile per wave for rows of 321
//                      to 512 floats, and past 512 the fragments are re-read
//                      per candidate tile) and one strip of candidate rows. Per 16-row candidate tile a
//                      wave gathers the rows straight into the B fragment
//                      layout (lane (col, q): row col, columns 16 kb + 4q..+3,
//                      one 16-B load per block; the next tile's loads are in
//                      flight while this tile's MFMAs run), forms the 16 x 16
//                      score tile with v_mfma_f32_16x16x4_f32 over the columns,
//                      scales by the candidates' inv_norm and compares with
//                      each query's threshold (its current k-th best, in
//                      registers): after warm-up almost every score fails that
//                      one compare. The few that pass are inserted, one at a
//                      time by the whole wave, into the query's sorted list in
//                      LDS (lane j holds entry j, k <= 64). The wave's lists
//                      are its own: the kernel has no barrier.
//   nn_merge_kernel    one wavefront per query: strips x k partials -> k.
//
// Order: score descending, then row id ascending, everywhere, so the answer
// does not depend on the strip count or on arrival order. A row's score has
// one accumulation order (stated in w2v_tiles.hpp): it does not depend on the
// tile slot, the strip or the launch, so duplicate rows tie bit-exactly and a
// call repeats bit-identically. A non-finite score fails the threshold
// compare (NaN and -inf fail `>`; +inf is rejected beside it); rows past the
// candidate limit and the tail slots of the last tile are masked.
//
// Traffic: the grid is ordered query-block-fastest, so the workgroups in
// flight together walk the same one or two strips across all query blocks at
// about the same pace: the rows they are on sit in each XCD's L2, behind it
// the Infinity Cache, and the matrix comes from HBM about once per XCD, not
// once per query block. Two query tiles per wave halve what each FLOP asks of
// L1 / L2.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <string>

#include "w2v_dev.h"
#include "w2v_dev_internal.hpp"
#include "w2v_nn_internal.hpp"
#include "w2v_tiles.hpp"
#include "w2v_wave.hpp"

namespace w2v {

constexpr int kNnMaxK = 64;
constexpr int kNnMaxTerms = 8;
constexpr int kNnExclRegs = 8;                    // excluded ids per query kept in registers
constexpr int64_t kNnStripBytes = 16 << 20;       // auto strip: rows of this many bytes at most ...
constexpr int64_t kNnStripMinRows = 256;          //   ... and this many rows at least ...
constexpr int64_t kNnGridTarget = 256;            //   ... cut finer while the grid has fewer workgroups
constexpr int64_t kNnPartialBytes = 512ll << 20;  // partial (score, id) pairs per query chunk
constexpr int64_t kNnChunkQueries = 32768;        // queries per chunk at most

__global__ __launch_bounds__(256) void nn_norm_kernel(const float* rows, int64_t n_rows, int64_t pitch, int cols,
                                                      float* inv_norm) {
  const int lane = lane_id();
  const int64_t r = (int64_t)blockIdx.x * kDenseWaves + (threadIdx.x >> 6);
  if (r >= n_rows) return;  // wave-uniform
  const float* p = rows + r * pitch;
  float s = 0.f;
  row_walk(lane, cols, [&](int c) { s += sum_sq(*reinterpret_cast<const f32x4*>(p + c)); });
  s = wave_sum(s);
  if (lane == 0) inv_norm[r] = unit_scale(s);
}

// q[gq] (cols floats, in place for the vector form) <- the unit-length query.
__global__ __launch_bounds__(256) void nn_query_kernel(const float* rows, int64_t pitch, const float* inv_norm,
                                                       const int32_t* ids, const float* weights, int terms, float* q,
                                                       int64_t nq, int cols) {
  const int lane = lane_id();
  const int64_t gq = (int64_t)blockIdx.x * kDenseWaves + (threadIdx.x >> 6);
  if (gq >= nq) return;  // wave-uniform
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[kRowVecs];
  float* out = q + gq * cols;
#pragma unroll
  for (int v = 0; v < kRowVecs; ++v) {
    const int c = 4 * lane + 4 * kWave * v;
    acc[v] = (ids == nullptr && c < cols) ? *reinterpret_cast<const f32x4*>(out + c) : zero;
  }
  if (ids != nullptr) {
    for (int t = 0; t < terms; ++t) {
      const int id = ids[gq * terms + t];
      if (id < 0) continue;  // wave-uniform
      const float w = weights[gq * terms + t] * inv_norm[id];
      const float* p = rows + (int64_t)id * pitch;
#pragma unroll
      for (int v = 0; v < kRowVecs; ++v) {
        const int c = 4 * lane + 4 * kWave * v;
        if (c < cols) acc[v] += w * *reinterpret_cast<const f32x4*>(p + c);
      }
    }
  }
  float s = 0.f;
#pragma unroll
  for (int v = 0; v < kRowVecs; ++v) s += sum_sq(acc[v]);
  s = wave_sum(s);
  const float sc = unit_scale(s);
#pragma unroll
  for (int v = 0; v < kRowVecs; ++v) {
    const int c = 4 * lane + 4 * kWave * v;
    if (c < cols) *reinterpret_cast<f32x4*>(out + c) = acc[v] * sc;
  }
}

struct NnArgs {
  const float* rows;
  const float* inv_norm;
  const float* q;        // padded queries: a multiple of the query block rows of `cols` floats
  const int32_t* excl;   // nq x n_excl row ids a query never returns (-1: none)
  int32_t n_excl;
  int64_t pitch;
  int32_t cols;          // columns the scores cover: dim rounded up to 16
  int64_t limit;         // candidates [0, limit)
  int64_t strip_rows;
  int64_t strips;
  int64_t nq;
  int32_t nqb;           // query blocks
  int32_t k;
  float* p_score;        // [query][strip][k]
  int32_t* p_id;
};

// (s, id) ranks ahead of (t, jd): higher score, then lower row id.
__device__ __forceinline__ bool nn_ahead(float s, int id, float t, int jd) { return s > t || (s == t && id < jd); }

// Insert (s, id) into one query's sorted list (lane j holds entry j) unless k
// entries rank ahead of it; returns the list's k-th score afterwards.
__device__ __forceinline__ float nn_insert(float* ls, int* li, int k, int lane, float s, int id) {
  const bool in = lane < k;
  wave_lds_order();
  const float es = in ? ls[lane] : 0.f;
  const int ei = in ? li[lane] : 0;
  const int pos = __popcll(ballot(in && nn_ahead(es, ei, s, id)));  // empty entries (-inf) are never ahead
  const float last = readlane_f(es, k - 1);
  if (pos >= k) return last;
  wave_lds_order();
  if (in && lane >= pos && lane + 1 < k) {
    ls[lane + 1] = es;
    li[lane + 1] = ei;
  }
  if (lane == pos) {
    ls[pos] = s;
    li[pos] = id;
  }
  wave_lds_order();
  return pos == k - 1 ? s : readlane_f(es, k - 2);
}

// NB, QT and the order of the tile product: w2v_tiles.hpp. A: the query tiles,
// B: the candidate tiles. km_assign_kernel (w2v_kmeans.hip) has the same loop.
template <int NB, int QT>
__global__ __launch_bounds__(256) void nn_score_kernel(NnArgs a) {
  extern __shared__ float nn_lds[];
  constexpr int NR = NB > 0 ? NB : 1;
  constexpr int NQ = QT * kSnTile;  // queries per wave
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6);
  const int q4 = lane >> 4, col = lane & 15;
  const int64_t strip = blockIdx.x / (unsigned)a.nqb;
  const int qb = (int)(blockIdx.x % (unsigned)a.nqb);
  const int64_t q0 = ((int64_t)qb * kDenseWaves + wave) * NQ;
  if (q0 >= a.nq) return;  // wave-uniform; the kernel has no barrier
  const int k = a.k;
  float* const ls = nn_lds + wave * (2 * NQ * k);
  int* const li = reinterpret_cast<int*>(ls + NQ * k);
  const float ninf = -std::numeric_limits<float>::infinity();
  for (int i = lane; i < NQ * k; i += kWave) {
    ls[i] = ninf;
    li[i] = -1;
  }
  const int nkb = a.cols >> 4;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const float* const qp = a.q + (q0 + col) * a.cols + 4 * q4;  // tile u: + u * 16 * cols
  f32x4 qf[QT][NR];
  if (NB > 0) {
#pragma unroll
    for (int u = 0; u < QT; ++u)
#pragma unroll
      for (int kb = 0; kb < NR; ++kb)
        qf[u][kb] = kb < nkb ? *reinterpret_cast<const f32x4*>(qp + (int64_t)u * kSnTile * a.cols + 16 * kb) : zero;
  }
  const int64_t r0 = strip * a.strip_rows;
  const int64_t r1 = min(a.limit, r0 + a.strip_rows);
  float thr[QT][4];
  bool mine[QT][4];
  // up to kNnExclRegs excluded ids per query live in registers: lane (col, q4)
  // holds entries q4 and q4 + 4 of query 16 u + col (-1: none); longer lists
  // are read from memory for the few scores that pass the threshold
  int exr[QT][2];
  const bool ex_regs = a.n_excl <= kNnExclRegs;
#pragma unroll
  for (int u = 0; u < QT; ++u) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      thr[u][r] = ninf;
      mine[u][r] = q0 + u * kSnTile + 4 * q4 + r < a.nq;
    }
    const int64_t gq = q0 + u * kSnTile + col;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int e = q4 + 4 * j;
      exr[u][j] = (ex_regs && e < a.n_excl && gq < a.nq) ? a.excl[gq * a.n_excl + e] : -1;
    }
  }

  // candidate row of this lane's tile slot, clamped into the matrix (masked below)
  auto row_of = [&](int64_t t) { return min(t + col, a.limit - 1); };
  f32x4 cur[NR], nxt[NR];
  if (NB > 0) {
    const float* cp = a.rows + row_of(r0) * a.pitch + 4 * q4;
#pragma unroll
    for (int kb = 0; kb < NR; ++kb) nxt[kb] = kb < nkb ? *reinterpret_cast<const f32x4*>(cp + 16 * kb) : zero;
  }
  for (int64_t t = r0; t < r1; t += kSnTile) {
    const int64_t row = row_of(t);
    const float inv = a.inv_norm[row];
    f32x4 acc0[QT], acc1[QT];
#pragma unroll
    for (int u = 0; u < QT; ++u) acc0[u] = acc1[u] = zero;
    if (NB > 0) {
#pragma unroll
      for (int kb = 0; kb < NR; ++kb) cur[kb] = nxt[kb];
      if (t + kSnTile < r1) {  // the next tile's rows, in flight behind this tile's MFMAs
        const float* cp = a.rows + row_of(t + kSnTile) * a.pitch + 4 * q4;
#pragma unroll
        for (int kb = 0; kb < NR; ++kb)
          if (kb < nkb) nxt[kb] = *reinterpret_cast<const f32x4*>(cp + 16 * kb);
      }
      // straight-line over all NB blocks: those past the row's width hold zeros on both sides
      // (never loaded). A width whose block count is instantiated wastes nothing; any other runs
      // the next larger instance and issues its extra blocks on zeros
#pragma unroll
      for (int kb = 0; kb < NR; ++kb) {
#pragma unroll
        for (int u = 0; u < QT; ++u) {
          acc0[u] = mfma16x16x4(qf[u][kb][0], cur[kb][0], acc0[u]);
          acc1[u] = mfma16x16x4(qf[u][kb][1], cur[kb][1], acc1[u]);
        }
#pragma unroll
        for (int u = 0; u < QT; ++u) {
          acc0[u] = mfma16x16x4(qf[u][kb][2], cur[kb][2], acc0[u]);
          acc1[u] = mfma16x16x4(qf[u][kb][3], cur[kb][3], acc1[u]);
        }
      }
    } else {
      const float* cp = a.rows + row * a.pitch + 4 * q4;
      for (int kb = 0; kb < nkb; ++kb) {
        const f32x4 ca = *reinterpret_cast<const f32x4*>(cp + 16 * kb);
#pragma unroll
        for (int u = 0; u < QT; ++u) {
          const f32x4 qa = *reinterpret_cast<const f32x4*>(qp + (int64_t)u * kSnTile * a.cols + 16 * kb);
          acc0[u] = mfma16x16x4(qa[0], ca[0], acc0[u]);
          acc1[u] = mfma16x16x4(qa[1], ca[1], acc1[u]);
          acc0[u] = mfma16x16x4(qa[2], ca[2], acc0[u]);
          acc1[u] = mfma16x16x4(qa[3], ca[3], acc1[u]);
        }
      }
    }
    // lane holds the scores of queries 16 u + 4 q4 + r against candidate t + col
    const bool valid = t + col < r1;
    float s[QT][4];
    bool pass[QT][4], any = false;
#pragma unroll
    for (int u = 0; u < QT; ++u) {
      const f32x4 acc = acc0[u] + acc1[u];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[u][r] = acc[r] * inv;
        pass[u][r] = valid && mine[u][r] && s[u][r] > thr[u][r] && s[u][r] < std::numeric_limits<float>::infinity();
        any = any || pass[u][r];
      }
    }
    if (ballot(any) == 0ull) continue;
#pragma unroll
    for (int u = 0; u < QT; ++u) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        unsigned long long m = ballot(pass[u][r]);
        while (m) {
          const int b = __builtin_ctzll(m);
          m &= m - 1;
          const int qc = 4 * (b >> 4) + r;  // the query's slot in tile u
          const int qi = u * kSnTile + qc;
          const int id = (int)t + (b & 15);
          const float sv = readlane_f(s[u][r], b);
          bool ex = col == qc && (exr[u][0] == id || exr[u][1] == id);
          if (!ex_regs) {
            for (int e0 = 0; e0 < a.n_excl; e0 += kWave) {
              const int e = e0 + lane;
              ex = ex || (e < a.n_excl && a.excl[(q0 + qi) * a.n_excl + e] == id);
            }
          }
          if (ballot(ex) != 0ull) continue;
          const float nt = nn_insert(ls + qi * k, li + qi * k, k, lane, sv, id);
          if (q4 == (b >> 4)) thr[u][r] = nt;
        }
      }
    }
  }
  wave_lds_order();
  for (int qi = 0; qi < NQ; ++qi) {
    if (q0 + qi >= a.nq) break;
    if (lane < k) {
      const int64_t o = ((q0 + qi) * a.strips + strip) * k + lane;
      a.p_score[o] = ls[qi * k + lane];
      a.p_id[o] = li[qi * k + lane];
    }
  }
}

// One wavefront per query: the k best of its n = strips x k partial entries
// (row ids are unique across strips, so the order is total), -1 / -inf past
// the last candidate.
__global__ __launch_bounds__(256) void nn_merge_kernel(const float* p_score, const int32_t* p_id, int64_t n, int k,
                                                       int64_t nq, float* o_score, int32_t* o_id) {
  const int lane = lane_id();
  const int64_t gq = (int64_t)blockIdx.x * kDenseWaves + (threadIdx.x >> 6);
  if (gq >= nq) return;  // wave-uniform
  const float* ps = p_score + gq * n;
  const int32_t* pi = p_id + gq * n;
  const float ninf = -std::numeric_limits<float>::infinity();
  float prev_s = std::numeric_limits<float>::infinity();
  int prev_i = -1;
  for (int j = 0; j < k; ++j) {
    float bs = ninf;
    int bi = -1;
    for (int64_t e = lane; e < n; e += kWave) {
      const int id = pi[e];
      if (id < 0) continue;
      const float s = ps[e];
      if (nn_ahead(prev_s, prev_i, s, id) && (bi < 0 || nn_ahead(s, id, bs, bi))) {
        bs = s;
        bi = id;
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const float os = __shfl_xor(bs, off);
      const int oi = __shfl_xor(bi, off);
      if (oi >= 0 && (bi < 0 || nn_ahead(os, oi, bs, bi))) {
        bs = os;
        bi = oi;
      }
    }
    if (lane == 0) {
      o_score[gq * k + j] = bi >= 0 ? bs : ninf;
      o_id[gq * k + j] = bi;
    }
    if (bi < 0) {  // wave-uniform: no candidate left
      for (int jj = j + 1 + lane; jj < k; jj += kWave) {
        o_score[gq * k + jj] = ninf;
        o_id[gq * k + jj] = -1;
      }
      break;
    }
    prev_s = bs;
    prev_i = bi;
  }
}

}  // namespace w2v

// struct w2v_nn: w2v_nn_internal.hpp (shared with w2v_kmeans.hip)

namespace {

int compute_norms(w2v_nn* x) {
  const unsigned grid = (unsigned)((x->n_rows + w2v::kDenseWaves - 1) / w2v::kDenseWaves);
  hipLaunchKernelGGL(w2v::nn_norm_kernel, dim3(grid), dim3(256), 0, x->stream, x->rows, x->n_rows, x->pitch, x->cols,
                     x->inv_norm.get());
  W2V_HIP_TRY(hipGetLastError());
  W2V_HIP_TRY(hipStreamSynchronize(x->stream));
  return W2V_OK;
}

using ScoreFn = void (*)(w2v::NnArgs);
// The instance for rows of `cols` floats (w2v_tiles.hpp) and the queries its workgroup owns.
ScoreFn score_kernel_for(int cols, int* query_block) { W2V_TILE_KERNEL_FOR(w2v::nn_score_kernel, cols, query_block); }
int query_block_for(int cols) {
  int qb = 0;
  (void)score_kernel_for(cols, &qb);
  return qb;
}

// One chunk of queries already staged in x->q (vector form: raw, ids ==
// nullptr) or described by x->ids / x->wts (by-row form), to out[0 .. n k).
int run_chunk(w2v_nn* x, int64_t n, bool by_row, int32_t terms, const int32_t* excl_d, int32_t n_excl, int64_t limit,
              int32_t k, int64_t strip_rows, int64_t strips, int32_t* out_ids, float* out_scores) {
  const unsigned qgrid = (unsigned)((n + w2v::kDenseWaves - 1) / w2v::kDenseWaves);
  hipLaunchKernelGGL(w2v::nn_query_kernel, dim3(qgrid), dim3(256), 0, x->stream, x->rows, x->pitch,
                     x->inv_norm.get(), by_row ? x->ids.get() : (const int32_t*)nullptr, x->wts.get(), terms,
                     x->q.get(), n, x->cols);
  W2V_HIP_TRY(hipGetLastError());
  w2v::NnArgs a{};
  a.rows = x->rows;
  a.inv_norm = x->inv_norm.get();
  a.q = x->q.get();
  a.excl = excl_d;
  a.n_excl = n_excl;
  a.pitch = x->pitch;
  a.cols = x->cols;
  a.limit = limit;
  a.strip_rows = strip_rows;
  a.strips = strips;
  a.nq = n;
  const int qblock = query_block_for(x->cols);
  a.nqb = (int32_t)((n + qblock - 1) / qblock);
  a.k = k;
  a.p_score = x->p_score.get();
  a.p_id = x->p_id.get();
  const size_t lds = (size_t)2 * qblock * k * sizeof(float);  // a (score, id) list of k per query
  int qb_ = 0;
  hipLaunchKernelGGL(score_kernel_for(x->cols, &qb_), dim3((unsigned)(strips * a.nqb)), dim3(256), lds, x->stream, a);
  W2V_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(w2v::nn_merge_kernel, dim3(qgrid), dim3(256), 0, x->stream, x->p_score.get(), x->p_id.get(),
                     strips * k, k, n, x->o_score.get(), x->o_id.get());
  W2V_HIP_TRY(hipGetLastError());
  W2V_HIP_TRY(hipMemcpyAsync(out_ids, x->o_id.get(), (size_t)n * k * sizeof(int32_t), hipMemcpyDeviceToHost, x->stream));
  W2V_HIP_TRY(hipMemcpyAsync(out_scores, x->o_score.get(), (size_t)n * k * sizeof(float), hipMemcpyDeviceToHost, x->stream));
  W2V_HIP_TRY(hipStreamSynchronize(x->stream));
  return W2V_OK;
}

// The shared part of the two query forms: q != nullptr is the vector form.
int run_query(w2v_nn* x, const float* q, const int32_t* ids, const float* weights, int32_t terms, int64_t nq,
              const int32_t* exclude, int32_t n_excl, int64_t restrict_rows, int32_t k, int32_t* out_ids,
              float* out_scores) {
  const int64_t limit = restrict_rows > 0 ? std::min(restrict_rows, x->n_rows) : x->n_rows;
  const int64_t qblock = query_block_for(x->cols);
  const int64_t nqb = std::max<int64_t>(1, (std::min(nq, w2v::kNnChunkQueries) + qblock - 1) / qblock);
  int64_t strip_rows = x->strip_rows_set;
  if (strip_rows == 0) {
    // long strips keep the per-strip top-k warm-up (k (1 + ln(rows / k)) insertions per query) small
    // beside the MFMAs; fewer query blocks take shorter ones, down to kNnStripMinRows, to fill the chip
    const int64_t by_bytes = w2v::kNnStripBytes / (x->pitch * (int64_t)sizeof(float));
    const int64_t by_grid = limit * nqb / w2v::kNnGridTarget;
    strip_rows = std::max(w2v::kNnStripMinRows, (std::min(by_bytes, by_grid) + 15) / 16 * 16);
  }
  const int64_t strips = (limit + strip_rows - 1) / strip_rows;
  // a query block is the least a launch takes: its partial lists must fit their budget
  if (strips * k * qblock * (int64_t)sizeof(float) > w2v::kNnPartialBytes)
    return w2v::set_error(W2V_ERR_ARG, "w2v_nn query: " + std::to_string(strips) + " strips of " + std::to_string(strip_rows) +
                   " rows at k " + std::to_string(k) + " need more than " +
                   std::to_string(w2v::kNnPartialBytes >> 20) + " MiB of partial lists per query block; set a larger "
                   "strip (w2v_nn_set_strip_rows; 0 = automatic)");
  if (strips * nqb > (int64_t)0x7fffffff)
    return w2v::set_error(W2V_ERR_ARG, "w2v_nn query: too many strips x query blocks for one grid; set a larger strip (w2v_nn_set_strip_rows)");
  x->plan_strips = strips;
  x->plan_strip_rows = strip_rows;
  if (nq == 0) return W2V_OK;
  W2V_HIP_TRY(hipSetDevice(x->device));
  // queries per chunk: what keeps the partial buffers within their budget
  int64_t chunk = w2v::kNnPartialBytes / (strips * k * (int64_t)sizeof(float));
  chunk = std::max<int64_t>(qblock, std::min(chunk, w2v::kNnChunkQueries) / qblock * qblock);
  chunk = std::min(chunk, (nq + qblock - 1) / qblock * qblock);
  int rc;
  const size_t q_n = (size_t)chunk * x->cols, q_bytes = q_n * sizeof(float);
  if ((rc = x->q.reserve(q_n))) return rc;
  if ((rc = x->p_score.reserve((size_t)chunk * strips * k))) return rc;
  if ((rc = x->p_id.reserve((size_t)chunk * strips * k))) return rc;
  if ((rc = x->o_score.reserve((size_t)chunk * k))) return rc;
  if ((rc = x->o_id.reserve((size_t)chunk * k))) return rc;
  const int32_t n_ids = q ? n_excl : terms;  // ids per query in x->ids: the exclusions, or the terms
  if (n_ids > 0 && (rc = x->ids.reserve((size_t)chunk * n_ids))) return rc;
  if (!q && (rc = x->wts.reserve((size_t)chunk * terms))) return rc;
  for (int64_t c0 = 0; c0 < nq; c0 += chunk) {
    const int64_t n = std::min(chunk, nq - c0);
    W2V_HIP_TRY(hipMemsetAsync(x->q.get(), 0, q_bytes, x->stream));  // padding columns and tail queries are zero
    if (q) {
      W2V_HIP_TRY(hipMemcpy2DAsync(x->q.get(), (size_t)x->cols * sizeof(float), q + c0 * x->dim, (size_t)x->dim * sizeof(float),
                             (size_t)x->dim * sizeof(float), (size_t)n, hipMemcpyHostToDevice, x->stream));
      if (n_excl > 0)
        W2V_HIP_TRY(hipMemcpyAsync(x->ids.get(), exclude + c0 * n_excl, (size_t)n * n_excl * sizeof(int32_t),
                             hipMemcpyHostToDevice, x->stream));
    } else {
      W2V_HIP_TRY(hipMemcpyAsync(x->ids.get(), ids + c0 * terms, (size_t)n * terms * sizeof(int32_t), hipMemcpyHostToDevice,
                           x->stream));
      W2V_HIP_TRY(hipMemcpyAsync(x->wts.get(), weights + c0 * terms, (size_t)n * terms * sizeof(float), hipMemcpyHostToDevice,
                           x->stream));
    }
    rc = run_chunk(x, n, q == nullptr, terms, n_ids > 0 ? x->ids.get() : nullptr, n_ids, limit, k,
                   strip_rows, strips, out_ids + c0 * k, out_scores + c0 * k);
    if (rc) return rc;
  }
  return W2V_OK;
}

int check_common(const char* fn, w2v_nn* x, int64_t nq, int64_t restrict_rows, int32_t k, const int32_t* out_ids,
                 const float* out_scores) {
  const std::string f(fn);
  if (!x) return w2v::set_error(W2V_ERR_ARG, f + ": null index");
  if (nq < 0) return w2v::set_error(W2V_ERR_ARG, f + ": nq must be >= 0");
  if (k < 1 || k > w2v::kNnMaxK) return w2v::set_error(W2V_ERR_ARG, f + ": k must be in [1, " + std::to_string(w2v::kNnMaxK) + "], got " + std::to_string(k));
  if (restrict_rows < 0) return w2v::set_error(W2V_ERR_ARG, f + ": restrict_rows must be >= 0 (0 = all rows)");
  if (nq > 0 && (!out_ids || !out_scores)) return w2v::set_error(W2V_ERR_ARG, f + ": null output");
  return W2V_OK;
}

}  // namespace

extern "C" {

int w2v_nn_limits(int32_t* max_dim, int32_t* max_k, int32_t* max_terms) {
  if (max_dim) *max_dim = w2v::kDenseMaxDim;
  if (max_k) *max_k = w2v::kNnMaxK;
  if (max_terms) *max_terms = w2v::kNnMaxTerms;
  return W2V_OK;
}

int w2v_nn_create(int32_t device, const float* rows, int64_t n_rows, int32_t dim, w2v_nn** out) {
  if (!out) return w2v::set_error(W2V_ERR_ARG, "w2v_nn_create: null output");
  *out = nullptr;
  if (!rows) return w2v::set_error(W2V_ERR_ARG, "w2v_nn_create: null matrix");
  if (dim < 1 || dim > w2v::kDenseMaxDim)
    return w2v::set_error(W2V_ERR_ARG, "w2v_nn_create: dim must be in [1, " + std::to_string(w2v::kDenseMaxDim) + "], got " + std::to_string(dim));
  if (n_rows < 1 || n_rows > (int64_t)0x7fffffff)
    return w2v::set_error(W2V_ERR_ARG, "w2v_nn_create: n_rows must be in [1, 2^31), got " + std::to_string(n_rows));
  w2v::Range range_("w2v_nn_create");
  if (device >= 0) W2V_HIP_TRY(hipSetDevice(device));
  int dev = 0;
  W2V_HIP_TRY(hipGetDevice(&dev));
  std::unique_ptr<w2v_nn> x(new w2v_nn());
  x->device = dev;
  x->n_rows = n_rows;
  x->dim = dim;
  x->cols = (dim + 15) & ~15;
  x->pitch = x->cols;
  W2V_HIP_TRY(hipStreamCreateWithFlags(&x->stream, hipStreamNonBlocking));
  const size_t n = (size_t)n_rows * x->pitch;
  int rc;
  if ((rc = x->rows_own.alloc(n)) || (rc = x->inv_norm.alloc((size_t)n_rows))) return rc;
  x->rows = x->rows_own.get();
  W2V_HIP_TRY(hipMemsetAsync(x->rows_own.get(), 0, n * sizeof(float), x->stream));
  W2V_HIP_TRY(hipMemcpy2DAsync(x->rows_own.get(), (size_t)x->pitch * sizeof(float), rows, (size_t)dim * sizeof(float),
                               (size_t)dim * sizeof(float), (size_t)n_rows, hipMemcpyHostToDevice, x->stream));
  if ((rc = compute_norms(x.get()))) return rc;
  *out = x.release();
  return W2V_OK;
}

int w2v_nn_attach(w2v_dev* h, int32_t which, w2v_nn** out) {
  w2v::Range range_("w2v_nn_attach");
  if (!out) return w2v::set_error(W2V_ERR_ARG, "w2v_nn_attach: null output");
  *out = nullptr;
  if (!h) return w2v::set_error(W2V_ERR_ARG, "w2v_nn_attach: null handle");
  if (which != 0 && which != 1) return w2v::set_error(W2V_ERR_ARG, "w2v_nn_attach: which must be 0 (W) or 1 (C)");
  const w2v::DevInfo info = w2v::dev_info(h);
  if (info.V < 1) return w2v::set_error(W2V_ERR_STATE, "w2v_nn_attach: the handle has no vocabulary yet");
  W2V_HIP_TRY(hipSetDevice(info.device));
  std::unique_ptr<w2v_nn> x(new w2v_nn());
  x->device = info.device;
  x->h = h;
  x->which = which;
  x->n_rows = info.V;
  x->dim = info.dim;
  x->cols = (info.dim + 15) & ~15;
  W2V_HIP_TRY(hipStreamCreateWithFlags(&x->stream, hipStreamNonBlocking));
  int rc;
  if ((rc = x->inv_norm.alloc((size_t)x->n_rows)) || (rc = w2v_nn_refresh(x.get()))) return rc;
  *out = x.release();
  return W2V_OK;
}

int w2v_nn_refresh(w2v_nn* x) {
  if (!x) return w2v::set_error(W2V_ERR_ARG, "w2v_nn_refresh: null index");
  W2V_HIP_TRY(hipSetDevice(x->device));
  if (x->h) {
    int rc = w2v_dev_synchronize(x->h);  // the training enqueued on the handle's stream
    if (rc) return rc;
    float *dW = nullptr, *dC = nullptr, *dS = nullptr;
    int64_t pitch = 0;
    if ((rc = w2v_dev_model_layout(x->h, &dW, &dC, &dS, &pitch))) return rc;
    float* m = x->which == 0 ? dW : dC;
    if (!m) return w2v::set_error(W2V_ERR_STATE, "w2v_nn: the handle's configuration has no such matrix");
    if (pitch < x->cols || pitch % 4 != 0) return w2v::set_error(W2V_ERR_STATE, "w2v_nn: unexpected row pitch");
    x->rows = m;
    x->pitch = pitch;
  }
  return compute_norms(x);
}

void w2v_nn_destroy(w2v_nn* x) { delete x; }

int w2v_nn_set_strip_rows(w2v_nn* x, int64_t rows) {
  if (!x) return w2v::set_error(W2V_ERR_ARG, "w2v_nn_set_strip_rows: null index");
  if (rows < 0 || rows % 16 != 0) return w2v::set_error(W2V_ERR_ARG, "w2v_nn_set_strip_rows: rows must be 0 (auto) or a positive multiple of 16");
  x->strip_rows_set = rows;
  return W2V_OK;
}

int w2v_nn_plan(w2v_nn* x, int64_t* strips, int32_t* query_block, int64_t* strip_rows) {
  if (!x) return w2v::set_error(W2V_ERR_ARG, "w2v_nn_plan: null index");
  if (strips) *strips = x->plan_strips;
  if (query_block) *query_block = query_block_for(x->cols);
  if (strip_rows) *strip_rows = x->plan_strip_rows;
  return W2V_OK;
}

int w2v_nn_query_vectors(w2v_nn* x, const float* q, int64_t nq, const int32_t* exclude, int32_t n_excl,
                         int64_t restrict_rows, int32_t k, int32_t* out_ids, float* out_scores) {
  w2v::Range range_("w2v_nn_query_vectors");
  const int rc = check_common("w2v_nn_query_vectors", x, nq, restrict_rows, k, out_ids, out_scores);
  if (rc) return rc;
  if (nq > 0 && !q) return w2v::set_error(W2V_ERR_ARG, "w2v_nn_query_vectors: null queries");
  if (n_excl < 0) return w2v::set_error(W2V_ERR_ARG, "w2v_nn_query_vectors: n_excl must be >= 0");
  if (!exclude) n_excl = 0;
  return run_query(x, q, nullptr, nullptr, 0, nq, exclude, n_excl, restrict_rows, k, out_ids, out_scores);
}

int w2v_nn_query_rows(w2v_nn* x, const int32_t* ids, const float* weights, int32_t terms, int64_t nq,
                      int64_t restrict_rows, int32_t k, int32_t* out_ids, float* out_scores) {
  w2v::Range range_("w2v_nn_query_rows");
  const int rc = check_common("w2v_nn_query_rows", x, nq, restrict_rows, k, out_ids, out_scores);
  if (rc) return rc;
  if (terms < 1 || terms > w2v::kNnMaxTerms)
    return w2v::set_error(W2V_ERR_ARG, "w2v_nn_query_rows: terms must be in [1, " + std::to_string(w2v::kNnMaxTerms) + "], got " + std::to_string(terms));
  if (nq > 0 && (!ids || !weights)) return w2v::set_error(W2V_ERR_ARG, "w2v_nn_query_rows: null ids or weights");
  for (int64_t i = 0; i < nq * terms; ++i)
    if (ids[i] >= x->n_rows)
      return w2v::set_error(W2V_ERR_ARG, "w2v_nn_query_rows: row id " + std::to_string(ids[i]) + " outside [0, " + std::to_string(x->n_rows) + ")");
  return run_query(x, nullptr, ids, weights, terms, nq, nullptr, 0, restrict_rows, k, out_ids, out_scores);
}

}  // extern "C"
