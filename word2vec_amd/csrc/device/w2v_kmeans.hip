// w2v_kmeans.hip — word classes (word2vec's -classes) behind the C-ABI
// (include/w2v_dev.h, w2v_nn_assign / w2v_nn_centroids / w2v_nn_classes):
// spherical k-means over the rows of an index, on the GPU.
//
// Kernels:
//   km_init_kernel    one wavefront per row: class r mod K (or the caller's
//                     class) for a finite row, -1 for a row with a non-finite
//                     element. The result also serves as the rows' finite flag.
//   km_update_kernel  the update step, memory-bound. One workgroup per (class,
//                     column slab). Wave w scans every fourth 1024-row chunk of
//                     the class array (four 16-B loads per lane, the next chunk
//                     in flight), compacts the members it finds by ballot into
//                     its own LDS queue and adds their rows, eight row loads in
//                     flight, into registers in queue order. The four partials
//                     are added in wave order through LDS. No float atomics: the
//                     order of a centroid's sum is a function of the class
//                     array and the constants below only (not of the slab
//                     count: a column's terms and their order are the same in
//                     every slab).
//   km_unit_kernel    one wavefront per centroid: x / max(|x|, 1e-12), and the
//                     centroid's validity (every element finite, one non-zero).
//   km_assign_kernel  the hot path: nn_score_kernel (w2v_nn.hip) with the roles
//                     swapped. A wave keeps the A fragments of two 16-row tiles
//                     of the matrix in registers (one tile for rows of 321 to
//                     512 floats; past 512 floats the fragments are re-read per
//                     centroid tile), loaded straight from the matrix at its
//                     own pitch, and walks the unit centroids 16 at a time in
//                     the B fragment layout (the next tile's loads in flight
//                     behind this tile's MFMAs). Products are
//                     v_mfma_f32_16x16x4_f32 in the one order w2v_tiles.hpp
//                     states. The running
//                     best (score, class) of a row lives in registers: `>`
//                     rejects NaN and the invalid / tail centroids are masked,
//                     +inf is rejected beside it, and centroids arrive in
//                     ascending id, so equal scores keep the lowest id; the 16
//                     lanes that share a row are reduced in the same order at
//                     the end, and inv_norm[row] multiplies once. No LDS, no
//                     barrier, no partial buffer. Rows whose class changed are
//                     counted with one integer atomic per wave.
//   km_count_kernel   member counts (integer atomics: exact).
//
// Every step normalises the centroids it is given, w2v_nn_classes included
// (its update's unit centroids pass through km_unit_kernel once more, as they
// would coming back from the caller), so the whole run is bit for bit the
// composition of w2v_nn_centroids and w2v_nn_assign. It also times its two
// steps with events (w2v_nn_class_times; tools/classes_bench.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <limits>
#include <string>
#include <vector>

#include "w2v_dev.h"
#include "w2v_dev_internal.hpp"
#include "w2v_nn_internal.hpp"
#include "w2v_tiles.hpp"
#include "w2v_wave.hpp"

namespace w2v {

constexpr int kKmMaxClasses = 65536;
constexpr int kKmMaxIterations = 1000;
constexpr int kKmScan = 1024;        // update: rows of the class array a wave scans per step
constexpr int kKmQueue = 128;        // update: a wave's member queue (flushed from 64 on)
constexpr int kKmBatch = 8;          // update: member rows in flight per wave
constexpr int kKmSlabCols = 512;     // update: columns per workgroup at most (two 16-B vectors per lane)
constexpr int kKmGridTarget = 256;   // update: cut rows into column slabs while the grid has fewer workgroups

__global__ __launch_bounds__(256) void km_init_kernel(const float* rows, int64_t n_rows, int64_t pitch, int cols,
                                                      const int32_t* in, int n_classes, int32_t* out) {
  const int lane = lane_id();
  const int64_t r = (int64_t)blockIdx.x * kDenseWaves + (threadIdx.x >> 6);
  if (r >= n_rows) return;  // wave-uniform
  const float* p = rows + r * pitch;
  bool fin = true;
  row_walk(lane, cols, [&](int c) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p + c);
    fin = fin && __builtin_isfinite(v[0]) && __builtin_isfinite(v[1]) && __builtin_isfinite(v[2]) &&
          __builtin_isfinite(v[3]);
  });
  const bool ok = ballot(!fin) == 0ull;
  if (lane == 0) out[r] = ok ? (in ? in[r] : (int32_t)(r % n_classes)) : -1;
}

// out[g] <- in[g] / max(|in[g]|, 1e-12) for g < n (in place or not), zero rows
// for n <= g < n16; valid[g]: every element finite and one of them non-zero.
__global__ __launch_bounds__(256) void km_unit_kernel(const float* in, float* out, int n, int n16, int cols,
                                                      int32_t* valid) {
  const int lane = lane_id();
  const int g = (int)(blockIdx.x * kDenseWaves + (threadIdx.x >> 6));
  if (g >= n16) return;  // wave-uniform
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[kRowVecs];
  bool fin = true, nz = false;
  float s = 0.f;
#pragma unroll
  for (int v = 0; v < kRowVecs; ++v) {
    const int c = 4 * lane + 4 * kWave * v;
    acc[v] = (g < n && c < cols) ? *reinterpret_cast<const f32x4*>(in + (int64_t)g * cols + c) : zero;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      fin = fin && __builtin_isfinite(acc[v][e]);
      nz = nz || acc[v][e] != 0.f;
    }
    s += sum_sq(acc[v]);
  }
  s = wave_sum(s);
  const float sc = unit_scale(s);
#pragma unroll
  for (int v = 0; v < kRowVecs; ++v) {
    const int c = 4 * lane + 4 * kWave * v;
    if (c < cols) *reinterpret_cast<f32x4*>(out + (int64_t)g * cols + c) = acc[v] * sc;
  }
  const bool ok = ballot(!fin) == 0ull && ballot(nz) != 0ull;
  if (lane == 0) valid[g] = (g < n && ok) ? 1 : 0;
}

struct KmUpdateArgs {
  const float* rows;
  int64_t pitch;
  int64_t n_rows;
  const int32_t* cls;  // padded to a multiple of kKmScan entries, -1 past n_rows
  int32_t cols;
  int32_t slab_cols;   // a multiple of 16, <= kKmSlabCols
  int32_t nslab;
  float* sums;         // [class][cols]
};

__global__ __launch_bounds__(256) void km_update_kernel(KmUpdateArgs a) {
  extern __shared__ float km_lds[];  // [kDenseWaves][slab_cols] partial sums, then [kDenseWaves][kKmQueue] member rows
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6);
  const int c = (int)(blockIdx.x / (unsigned)a.nslab);
  const int slab = (int)(blockIdx.x % (unsigned)a.nslab);
  const int c0 = slab * a.slab_cols, c1 = min(a.cols, c0 + a.slab_cols);
  int* const queue = reinterpret_cast<int*>(km_lds + kDenseWaves * a.slab_cols) + wave * kKmQueue;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const int cl0 = c0 + 4 * lane, cl1 = cl0 + 4 * kWave;
  const bool on0 = cl0 < c1, on1 = cl1 < c1;
  f32x4 acc0 = zero, acc1 = zero;
  int np = 0;  // queued members (wave-uniform)
  // add the queued rows in queue order, kKmBatch loads in flight
  auto flush = [&]() {
    wave_lds_order();
    for (int b = 0; b < np; b += kKmBatch) {
      f32x4 v0[kKmBatch], v1[kKmBatch];
#pragma unroll
      for (int i = 0; i < kKmBatch; ++i) {
        v0[i] = v1[i] = zero;
        if (b + i < np) {  // wave-uniform
          const float* p = a.rows + (int64_t)uniform_i(queue[b + i]) * a.pitch;
          if (on0) v0[i] = *reinterpret_cast<const f32x4*>(p + cl0);
          if (on1) v1[i] = *reinterpret_cast<const f32x4*>(p + cl1);
        }
      }
#pragma unroll
      for (int i = 0; i < kKmBatch; ++i) {
        if (b + i < np) {
          acc0 += v0[i];
          acc1 += v1[i];
        }
      }
    }
    np = 0;
    wave_lds_order();
  };
  constexpr int kVecs = kKmScan / (4 * kWave);  // 16-B loads per lane and chunk
  const int64_t nchunk = (a.n_rows + kKmScan - 1) / kKmScan;
  int4 cur[kVecs], nxt[kVecs];
  if (wave < nchunk) {
#pragma unroll
    for (int j = 0; j < kVecs; ++j)
      nxt[j] = *reinterpret_cast<const int4*>(a.cls + (int64_t)wave * kKmScan + 4 * kWave * j + 4 * lane);
  }
  for (int64_t ch = wave; ch < nchunk; ch += kDenseWaves) {
#pragma unroll
    for (int j = 0; j < kVecs; ++j) cur[j] = nxt[j];
    if (ch + kDenseWaves < nchunk) {
#pragma unroll
      for (int j = 0; j < kVecs; ++j)
        nxt[j] = *reinterpret_cast<const int4*>(a.cls + (ch + kDenseWaves) * kKmScan + 4 * kWave * j + 4 * lane);
    }
#pragma unroll
    for (int j = 0; j < kVecs; ++j) {
      const int v[4] = {cur[j].x, cur[j].y, cur[j].z, cur[j].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool hit = v[e] == c;
        const unsigned long long m = ballot(hit);
        if (m == 0ull) continue;
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        if (hit) queue[np + rank] = (int)(ch * kKmScan) + 4 * kWave * j + 4 * lane + e;
        np += __popcll(m);
        if (np >= kKmQueue - kWave) flush();
      }
    }
  }
  flush();
  float* const part = km_lds + wave * a.slab_cols;
  if (on0) *reinterpret_cast<f32x4*>(part + 4 * lane) = acc0;
  if (on1) *reinterpret_cast<f32x4*>(part + 4 * kWave + 4 * lane) = acc1;
  __syncthreads();
  for (int k = (int)threadIdx.x; k < c1 - c0; k += (int)blockDim.x) {
    float s = km_lds[k];
#pragma unroll
    for (int w = 1; w < kDenseWaves; ++w) s += km_lds[w * a.slab_cols + k];
    a.sums[(int64_t)c * a.cols + c0 + k] = s;
  }
}

__global__ __launch_bounds__(256) void km_count_kernel(const int32_t* cls, int64_t n, unsigned long long* counts) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && cls[i] >= 0) atomicAdd(counts + cls[i], 1ull);
}

struct KmAssignArgs {
  const float* rows;
  const float* inv_norm;
  int64_t pitch;
  int64_t n_rows;
  int32_t cols;          // columns the scores cover: dim rounded up to 16
  const float* cen;      // k16 x cols unit centroids (zero rows past the last class)
  const int32_t* valid;  // k16 flags
  int32_t k16;           // classes rounded up to 16
  const int32_t* flag;   // per row: < 0 = a non-finite row (member of nothing)
  const int32_t* prev;   // the classes to count changes against (may be null)
  int32_t* out_cls;
  float* out_score;
  unsigned long long* moved;
};

// NB, QT and the order of the tile product: w2v_tiles.hpp. A: the row tiles, B:
// the centroid tiles. nn_score_kernel (w2v_nn.hip) has the same loop.
template <int NB, int QT>
__global__ __launch_bounds__(256) void km_assign_kernel(KmAssignArgs a) {
  constexpr int NR = NB > 0 ? NB : 1;
  constexpr int NQ = QT * kSnTile;  // rows per wave
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6);
  const int q4 = lane >> 4, col = lane & 15;
  const int64_t r0 = ((int64_t)blockIdx.x * kDenseWaves + wave) * NQ;
  if (r0 >= a.n_rows) return;  // wave-uniform; the kernel has no barrier
  const int nkb = a.cols >> 4;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const float ninf = -std::numeric_limits<float>::infinity();
  // the row of this lane's slot in tile u, clamped into the matrix (not written below)
  const float* rp[QT];
#pragma unroll
  for (int u = 0; u < QT; ++u) rp[u] = a.rows + min(r0 + u * kSnTile + col, a.n_rows - 1) * a.pitch + 4 * q4;
  f32x4 qf[QT][NR];
  if (NB > 0) {
#pragma unroll
    for (int u = 0; u < QT; ++u)
#pragma unroll
      for (int kb = 0; kb < NR; ++kb) qf[u][kb] = kb < nkb ? *reinterpret_cast<const f32x4*>(rp[u] + 16 * kb) : zero;
  }
  float best[QT][4];
  int bc[QT][4];
#pragma unroll
  for (int u = 0; u < QT; ++u)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      best[u][r] = ninf;
      bc[u][r] = -1;
    }
  const float* const cp0 = a.cen + (int64_t)col * a.cols + 4 * q4;  // tile t: + t * cols
  f32x4 cur[NR], nxt[NR];
  if (NB > 0) {
#pragma unroll
    for (int kb = 0; kb < NR; ++kb) nxt[kb] = kb < nkb ? *reinterpret_cast<const f32x4*>(cp0 + 16 * kb) : zero;
  }
  for (int t = 0; t < a.k16; t += kSnTile) {
    const bool ok = a.valid[t + col] != 0;
    f32x4 acc0[QT], acc1[QT];
#pragma unroll
    for (int u = 0; u < QT; ++u) acc0[u] = acc1[u] = zero;
    if (NB > 0) {
#pragma unroll
      for (int kb = 0; kb < NR; ++kb) cur[kb] = nxt[kb];
      if (t + kSnTile < a.k16) {  // the next tile's centroids, in flight behind this tile's MFMAs
        const float* cp = cp0 + (int64_t)(t + kSnTile) * a.cols;
#pragma unroll
        for (int kb = 0; kb < NR; ++kb)
          if (kb < nkb) nxt[kb] = *reinterpret_cast<const f32x4*>(cp + 16 * kb);
      }
      // straight-line over all NB blocks: those past the row's width hold zeros on both sides
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
      const float* cp = cp0 + (int64_t)t * a.cols;
      for (int kb = 0; kb < nkb; ++kb) {
        const f32x4 ca = *reinterpret_cast<const f32x4*>(cp + 16 * kb);
#pragma unroll
        for (int u = 0; u < QT; ++u) {
          const f32x4 qa = *reinterpret_cast<const f32x4*>(rp[u] + 16 * kb);
          acc0[u] = mfma16x16x4(qa[0], ca[0], acc0[u]);
          acc1[u] = mfma16x16x4(qa[1], ca[1], acc1[u]);
          acc0[u] = mfma16x16x4(qa[2], ca[2], acc0[u]);
          acc1[u] = mfma16x16x4(qa[3], ca[3], acc1[u]);
        }
      }
    }
    // lane holds the products of rows 16 u + 4 q4 + r with centroid t + col
#pragma unroll
    for (int u = 0; u < QT; ++u) {
      const f32x4 acc = acc0[u] + acc1[u];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (ok && acc[r] > best[u][r] && acc[r] < std::numeric_limits<float>::infinity()) {
          best[u][r] = acc[r];
          bc[u][r] = t + col;
        }
      }
    }
  }
  // the 16 lanes that share a row: higher score, then lower class id
  bool changed = false;
#pragma unroll
  for (int u = 0; u < QT; ++u) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float s = best[u][r];
      int id = bc[u][r];
#pragma unroll
      for (int off = 1; off < kSnTile; off <<= 1) {
        const float os = __shfl_xor(s, off);
        const int oi = __shfl_xor(id, off);
        if (oi >= 0 && (id < 0 || os > s || (os == s && oi < id))) {
          s = os;
          id = oi;
        }
      }
      const int64_t row = r0 + u * kSnTile + 4 * q4 + r;
      if (col == 4 * u + r && row < a.n_rows) {  // one lane per row writes
        const int cl = a.flag[row] >= 0 ? id : -1;
        a.out_cls[row] = cl;
        a.out_score[row] = cl >= 0 ? s * a.inv_norm[row] : ninf;
        changed = changed || (a.prev != nullptr && a.prev[row] != cl);
      }
    }
  }
  const unsigned long long mv = ballot(changed);
  if (lane == 0 && mv != 0ull) atomicAdd(a.moved, (unsigned long long)__popcll(mv));
}

}  // namespace w2v

namespace {

using w2v::DevBuf;

int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// Device state of one call (the calls are synchronous; nothing is kept).
struct KmState {
  int32_t k = 0, k16 = 0;
  DevBuf<float> raw;   // k16 x cols: the caller's centroids, or the update's unit centroids
  DevBuf<float> unit;  // k16 x cols: what the assignment scores against
  DevBuf<float> sums;  // k x cols
  DevBuf<int32_t> valid;
  DevBuf<float> score;
  DevBuf<unsigned long long> moved, counts;
};

// A class array on the device: padded for the update's 16-B scan, -1 past n_rows.
int alloc_classes(w2v_nn* x, DevBuf<int32_t>& b) {
  const size_t n = (size_t)round_up(x->n_rows, w2v::kKmScan);
  int rc = b.alloc(n);
  if (rc) return rc;
  W2V_HIP_TRY(hipMemsetAsync(b.get(), 0xff, n * sizeof(int32_t), x->stream));
  return W2V_OK;
}

int init_state(w2v_nn* x, KmState& st, int32_t k) {
  st.k = k;
  st.k16 = (int32_t)round_up(k, 16);
  const size_t n = (size_t)st.k16 * x->cols;
  int rc;
  if ((rc = st.raw.alloc(n)) || (rc = st.unit.alloc(n)) || (rc = st.sums.alloc((size_t)k * x->cols)) ||
      (rc = st.valid.alloc((size_t)st.k16)) || (rc = st.score.alloc((size_t)x->n_rows)) || (rc = st.moved.alloc(1)) ||
      (rc = st.counts.alloc((size_t)k)))
    return rc;
  return W2V_OK;
}

// out[r] = in[r] (null: r mod k) for finite rows, -1 for the others.
int launch_init(w2v_nn* x, const int32_t* in, int32_t k, int32_t* out) {
  const unsigned grid = (unsigned)((x->n_rows + w2v::kDenseWaves - 1) / w2v::kDenseWaves);
  hipLaunchKernelGGL(w2v::km_init_kernel, dim3(grid), dim3(256), 0, x->stream, x->rows, x->n_rows, x->pitch, x->cols, in,
                     k, out);
  W2V_HIP_TRY(hipGetLastError());
  return W2V_OK;
}

int launch_unit(w2v_nn* x, KmState& st, const float* in, float* out) {
  const unsigned grid = (unsigned)((st.k16 + w2v::kDenseWaves - 1) / w2v::kDenseWaves);
  hipLaunchKernelGGL(w2v::km_unit_kernel, dim3(grid), dim3(256), 0, x->stream, in, out, st.k, st.k16, x->cols,
                     st.valid.get());
  W2V_HIP_TRY(hipGetLastError());
  return W2V_OK;
}

// The update step: st.raw <- the unit centroids of the (masked) classes cls.
int step_centroids(w2v_nn* x, KmState& st, const int32_t* cls) {
  w2v::KmUpdateArgs a{};
  a.rows = x->rows;
  a.pitch = x->pitch;
  a.n_rows = x->n_rows;
  a.cls = cls;
  a.cols = x->cols;
  // whole rows per workgroup (at most kKmSlabCols columns); few classes are cut into column slabs to fill the chip
  const int min_slabs = (x->cols + w2v::kKmSlabCols - 1) / w2v::kKmSlabCols;
  const int want = (w2v::kKmGridTarget + st.k - 1) / st.k;
  const int slabs = std::min(std::max(want, min_slabs), std::max(min_slabs, x->cols / 64));
  a.slab_cols = (int32_t)round_up((x->cols + slabs - 1) / slabs, 16);
  a.nslab = (x->cols + a.slab_cols - 1) / a.slab_cols;
  a.sums = st.sums.get();
  const size_t lds = ((size_t)w2v::kDenseWaves * a.slab_cols + (size_t)w2v::kDenseWaves * w2v::kKmQueue) * sizeof(float);
  hipLaunchKernelGGL(w2v::km_update_kernel, dim3((unsigned)(st.k * a.nslab)), dim3(256), lds, x->stream, a);
  W2V_HIP_TRY(hipGetLastError());
  return launch_unit(x, st, st.sums.get(), st.raw.get());
}

using AssignFn = void (*)(w2v::KmAssignArgs);
// The instance for rows of `cols` floats (w2v_tiles.hpp) and the rows its workgroup owns.
AssignFn assign_kernel_for(int cols, int* rows_per_block) { W2V_TILE_KERNEL_FOR(w2v::km_assign_kernel, cols, rows_per_block); }

// The assign step against st.raw (any length): st.unit <- its unit centroids,
// out / st.score <- each row's class and score, st.moved <- rows with out != prev.
int step_assign(w2v_nn* x, KmState& st, const int32_t* flag, const int32_t* prev, int32_t* out) {
  int rc = launch_unit(x, st, st.raw.get(), st.unit.get());
  if (rc) return rc;
  W2V_HIP_TRY(hipMemsetAsync(st.moved.get(), 0, sizeof(unsigned long long), x->stream));
  w2v::KmAssignArgs a{};
  a.rows = x->rows;
  a.inv_norm = x->inv_norm.get();
  a.pitch = x->pitch;
  a.n_rows = x->n_rows;
  a.cols = x->cols;
  a.cen = st.unit.get();
  a.valid = st.valid.get();
  a.k16 = st.k16;
  a.flag = flag;
  a.prev = prev;
  a.out_cls = out;
  a.out_score = st.score.get();
  a.moved = st.moved.get();
  int per_block = 0;
  const AssignFn fn = assign_kernel_for(x->cols, &per_block);
  hipLaunchKernelGGL(fn, dim3((unsigned)((x->n_rows + per_block - 1) / per_block)), dim3(256), 0, x->stream, a);
  W2V_HIP_TRY(hipGetLastError());
  return W2V_OK;
}

int count_members(w2v_nn* x, KmState& st, const int32_t* cls, int64_t* out_count) {
  W2V_HIP_TRY(hipMemsetAsync(st.counts.get(), 0, (size_t)st.k * sizeof(unsigned long long), x->stream));
  hipLaunchKernelGGL(w2v::km_count_kernel, dim3((unsigned)((x->n_rows + 255) / 256)), dim3(256), 0, x->stream, cls,
                     x->n_rows, st.counts.get());
  W2V_HIP_TRY(hipGetLastError());
  W2V_HIP_TRY(hipMemcpyAsync(out_count, st.counts.get(), (size_t)st.k * sizeof(int64_t), hipMemcpyDeviceToHost, x->stream));
  return W2V_OK;
}

// st.raw (cols wide) to the caller's dense n_classes x dim.
int download_centroids(w2v_nn* x, KmState& st, float* out) {
  W2V_HIP_TRY(hipMemcpy2DAsync(out, (size_t)x->dim * sizeof(float), st.raw.get(), (size_t)x->cols * sizeof(float),
                               (size_t)x->dim * sizeof(float), (size_t)st.k, hipMemcpyDeviceToHost, x->stream));
  return W2V_OK;
}

// Device time of the two steps of the calling thread's last w2v_nn_classes,
// summed over its iterations (w2v_nn_class_times; tools/classes_bench.py).
thread_local double t_update_ms = 0.0, t_assign_ms = 0.0;

// Three events: before the update, between the steps, after the assign.
struct StepEvents {
  hipEvent_t e[3] = {nullptr, nullptr, nullptr};
  int create() {
    for (hipEvent_t& ev : e) W2V_HIP_TRY(hipEventCreate(&ev));
    return W2V_OK;
  }
  ~StepEvents() {
    for (hipEvent_t ev : e)
      if (ev) (void)hipEventDestroy(ev);
  }
};

int check_classes(const char* fn, w2v_nn* x, int32_t n_classes) {
  const std::string f(fn);
  if (!x) return w2v::set_error(W2V_ERR_ARG, f + ": null index");
  const int64_t most = std::min<int64_t>(x->n_rows, w2v::kKmMaxClasses);
  if (n_classes < 1 || n_classes > most)
    return w2v::set_error(W2V_ERR_ARG, f + ": n_classes must be in [1, " + std::to_string(most) + "] (the rows, at most " +
                                           std::to_string(w2v::kKmMaxClasses) + "), got " + std::to_string(n_classes));
  return W2V_OK;
}

}  // namespace

extern "C" {

int w2v_nn_class_limits(int32_t* max_classes, int32_t* max_iterations) {
  if (max_classes) *max_classes = w2v::kKmMaxClasses;
  if (max_iterations) *max_iterations = w2v::kKmMaxIterations;
  return W2V_OK;
}

int w2v_nn_class_times(double* update_ms, double* assign_ms) {
  if (update_ms) *update_ms = t_update_ms;
  if (assign_ms) *assign_ms = t_assign_ms;
  return W2V_OK;
}

int w2v_nn_assign(w2v_nn* x, const float* centroids, int32_t n_classes, int32_t* out_class, float* out_score) {
  w2v::Range range_("w2v_nn_assign");
  int rc = check_classes("w2v_nn_assign", x, n_classes);
  if (rc) return rc;
  if (!centroids) return w2v::set_error(W2V_ERR_ARG, "w2v_nn_assign: null centroids");
  if (!out_class) return w2v::set_error(W2V_ERR_ARG, "w2v_nn_assign: null class output");
  W2V_HIP_TRY(hipSetDevice(x->device));
  KmState st;
  DevBuf<int32_t> flag, cls;
  if ((rc = init_state(x, st, n_classes)) || (rc = alloc_classes(x, flag)) || (rc = alloc_classes(x, cls))) return rc;
  W2V_HIP_TRY(hipMemsetAsync(st.raw.get(), 0, st.raw.size() * sizeof(float), x->stream));  // the padding columns
  W2V_HIP_TRY(hipMemcpy2DAsync(st.raw.get(), (size_t)x->cols * sizeof(float), centroids, (size_t)x->dim * sizeof(float),
                               (size_t)x->dim * sizeof(float), (size_t)n_classes, hipMemcpyHostToDevice, x->stream));
  if ((rc = launch_init(x, nullptr, 1, flag.get())) || (rc = step_assign(x, st, flag.get(), nullptr, cls.get()))) return rc;
  W2V_HIP_TRY(hipMemcpyAsync(out_class, cls.get(), (size_t)x->n_rows * sizeof(int32_t), hipMemcpyDeviceToHost, x->stream));
  if (out_score)
    W2V_HIP_TRY(hipMemcpyAsync(out_score, st.score.get(), (size_t)x->n_rows * sizeof(float), hipMemcpyDeviceToHost, x->stream));
  W2V_HIP_TRY(hipStreamSynchronize(x->stream));
  return W2V_OK;
}

int w2v_nn_centroids(w2v_nn* x, const int32_t* cls, int32_t n_classes, float* out_centroids, int64_t* out_count) {
  w2v::Range range_("w2v_nn_centroids");
  int rc = check_classes("w2v_nn_centroids", x, n_classes);
  if (rc) return rc;
  if (!cls) return w2v::set_error(W2V_ERR_ARG, "w2v_nn_centroids: null classes");
  if (!out_centroids) return w2v::set_error(W2V_ERR_ARG, "w2v_nn_centroids: null centroid output");
  for (int64_t r = 0; r < x->n_rows; ++r)
    if (cls[r] < -1 || cls[r] >= n_classes)
      return w2v::set_error(W2V_ERR_ARG, "w2v_nn_centroids: class " + std::to_string(cls[r]) + " of row " + std::to_string(r) +
                                             " outside [-1, " + std::to_string(n_classes) + ")");
  W2V_HIP_TRY(hipSetDevice(x->device));
  KmState st;
  DevBuf<int32_t> in, masked;
  if ((rc = init_state(x, st, n_classes)) || (rc = alloc_classes(x, in)) || (rc = alloc_classes(x, masked))) return rc;
  W2V_HIP_TRY(hipMemcpyAsync(in.get(), cls, (size_t)x->n_rows * sizeof(int32_t), hipMemcpyHostToDevice, x->stream));
  if ((rc = launch_init(x, in.get(), n_classes, masked.get())) || (rc = step_centroids(x, st, masked.get())) ||
      (rc = download_centroids(x, st, out_centroids)))
    return rc;
  if (out_count && (rc = count_members(x, st, masked.get(), out_count))) return rc;
  W2V_HIP_TRY(hipStreamSynchronize(x->stream));
  return W2V_OK;
}

int w2v_nn_classes(w2v_nn* x, int32_t n_classes, int32_t iterations, int32_t* out_class, float* out_score,
                   float* out_centroids, int64_t* out_count, int64_t* out_moved, int32_t* iterations_run) {
  w2v::Range range_("w2v_nn_classes");
  int rc = check_classes("w2v_nn_classes", x, n_classes);
  if (rc) return rc;
  if (iterations < 1 || iterations > w2v::kKmMaxIterations)
    return w2v::set_error(W2V_ERR_ARG, "w2v_nn_classes: iterations must be in [1, " + std::to_string(w2v::kKmMaxIterations) +
                                           "], got " + std::to_string(iterations));
  if (!out_class) return w2v::set_error(W2V_ERR_ARG, "w2v_nn_classes: null class output");
  W2V_HIP_TRY(hipSetDevice(x->device));
  KmState st;
  DevBuf<int32_t> start, a, b;  // the start (also the rows' finite flag) and the two turns of the loop
  if ((rc = init_state(x, st, n_classes)) || (rc = alloc_classes(x, start)) || (rc = alloc_classes(x, a)) ||
      (rc = alloc_classes(x, b)) || (rc = launch_init(x, nullptr, n_classes, start.get())))
    return rc;
  if (out_moved) std::fill(out_moved, out_moved + iterations, (int64_t)0);
  StepEvents ev;
  if ((rc = ev.create())) return rc;
  t_update_ms = t_assign_ms = 0.0;
  const int32_t* cur = start.get();
  int32_t done = 0;
  for (int32_t it = 0; it < iterations; ++it) {
    int32_t* next = (it & 1) ? b.get() : a.get();
    W2V_HIP_TRY(hipEventRecord(ev.e[0], x->stream));
    if ((rc = step_centroids(x, st, cur))) return rc;
    W2V_HIP_TRY(hipEventRecord(ev.e[1], x->stream));
    if ((rc = step_assign(x, st, start.get(), cur, next))) return rc;
    W2V_HIP_TRY(hipEventRecord(ev.e[2], x->stream));
    unsigned long long moved = 0;
    W2V_HIP_TRY(hipMemcpyAsync(&moved, st.moved.get(), sizeof(moved), hipMemcpyDeviceToHost, x->stream));
    W2V_HIP_TRY(hipStreamSynchronize(x->stream));
    float up = 0.f, as = 0.f;
    W2V_HIP_TRY(hipEventElapsedTime(&up, ev.e[0], ev.e[1]));
    W2V_HIP_TRY(hipEventElapsedTime(&as, ev.e[1], ev.e[2]));
    t_update_ms += up;
    t_assign_ms += as;
    cur = next;
    done = it + 1;
    if (out_moved) out_moved[it] = (int64_t)moved;
    if (moved == 0) break;  // the next iteration would repeat this one
  }
  W2V_HIP_TRY(hipMemcpyAsync(out_class, cur, (size_t)x->n_rows * sizeof(int32_t), hipMemcpyDeviceToHost, x->stream));
  if (out_score)
    W2V_HIP_TRY(hipMemcpyAsync(out_score, st.score.get(), (size_t)x->n_rows * sizeof(float), hipMemcpyDeviceToHost, x->stream));
  if (out_centroids && (rc = download_centroids(x, st, out_centroids))) return rc;
  if (out_count && (rc = count_members(x, st, cur, out_count))) return rc;
  W2V_HIP_TRY(hipStreamSynchronize(x->stream));
  if (iterations_run) *iterations_run = done;
  return W2V_OK;
}

}  // extern "C"
