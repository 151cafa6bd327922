// w2v_phrase.hip — phrase detection on the GPU (include/w2v_ingest.h,
// w2v_phrase_*): word2phrase's rule over the ingested token ids, exact and
// deterministic (DESIGN.md §4.6 has the definition).
//
// One pass over a stream ids[0, n) cut into sentences by offsets[0..S]:
//   * the unigram histogram cnt[w] and the first position first[w] are kept
//     with the stream (count_kernel: adds aggregated per workgroup in an LDS
//     table first, so a Zipf head does not serialise on a few addresses; the
//     first position is an atomic min issued only when smaller);
//   * insert: every position that is not a sentence start and whose two words
//     both have cnt >= min_count finds or claims the slot of its pair in an
//     open-addressing table keyed by the exact 64-bit key (a << 32 | b) + 1
//     (compare-and-swap on the key; 0 = empty: no second hash, no collision
//     failure) and records slot[i]. Idempotent: when a position finds no slot
//     or the table passes half full, the table doubles (rehash kernel) and the
//     insert runs again;
//   * count: one add per eligible position on its slot, LDS-aggregated;
//   * score: float32, (pab - min_count) / cnt[a] / cnt[b] * N, strict compare
//     with the threshold -> cand[i];
//   * joins: join[i] = cand[i] && !join[i-1], i.e. cand[i] and an odd number
//     of consecutive candidates ending at i. The run length is a segmented
//     scan, computed as i - (inclusive max-scan of (cand[i] ? -1 : i)): the
//     last non-candidate at or before i (position 0 opens a sentence and is
//     never a candidate);
//   * rewrite: the exclusive scan of !join gives the output positions; a kept
//     token followed by a joined one becomes that pair's phrase id. Phrase ids
//     number the joined pairs by the position of their first joined
//     occurrence (atomic min per slot, then select + radix sort), never by
//     slot number: the result does not depend on the table size, on growth or
//     on the launch. offsets'[s] = outpos[offsets[s]] (a sentence start is
//     never joined);
//   * the new stream's histogram.
// The probe loop, count_kernel, the select + sort and the growth step are
// w2v_table.hpp's, shared with w2v_ingest.hip.
// Only integer atomics (compare-and-swap, add, min). hipcub's element counts
// are int: a stream holds fewer than 2^31 - 64 tokens and the table at most
// 2^30 slots.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <string>
#include <vector>

#include "w2v_dev_internal.hpp"
#include "w2v_ingest.h"
#include "w2v_table.hpp"

namespace w2v {
namespace phrase {

using namespace w2v::table;  // kNone: slot[i] of a position that holds no eligible pair

constexpr ull kNever = ~0ull;   // first / firstjoin of a word / pair never seen / joined
constexpr int kMaxProbe = 512;  // a longer chain counts as a full table (the table grows)
constexpr int64_t kMaxTokens = (int64_t)INT32_MAX - 64;
constexpr int64_t kMaxWords = (int64_t)1 << 31;

struct Table {
  uint64_t* key;   // (a << 32 | b) + 1, 0 = empty
  ull* count;      // eligible positions holding the pair
  ull* joined;     // ... of which joined
  ull* firstjoin;  // smallest joined position (kNever: none)
  int32_t* pid;    // the pair's phrase id (valid where firstjoin != kNever)
  uint64_t mask;
};

// start[offsets[s]] = 1 for every non-empty sentence s.
__global__ void starts_kernel(const int64_t* offsets, int64_t n_sent, uint8_t* start) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n_sent; s += stride) {
    const int64_t o = offsets[s];
    if (o < offsets[s + 1]) start[o] = 1;
  }
}

// Insert (idempotent): slot[i] of every eligible position. A pair's home slot is its key's splitmix64 hash.
__global__ void insert_kernel(const int32_t* ids, const uint8_t* start, int64_t n, const ull* cnt, ull min_count,
                              Table tab, uint32_t* slot, ull* used, ull* fail) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    uint32_t s = kNone;
    if (i > 0 && !start[i]) {
      const uint32_t a = (uint32_t)ids[i - 1], b = (uint32_t)ids[i];
      if (cnt[a] >= min_count && cnt[b] >= min_count) {
        bool won = false;
        const uint64_t key = (((uint64_t)a << 32) | b) + 1;
        const int64_t j = claim<kMaxProbe>(tab.key, tab.mask, mix64(key) & tab.mask, key, &won);
        if (j < 0) {
          atomicAdd(fail, 1ull);
        } else {
          if (won) atomicAdd(used, 1ull);
          s = (uint32_t)j;
        }
      }
    }
    slot[i] = s;
  }
}

// Move every key of `from` into `to` (a larger, empty table); the counts are still zero.
__global__ void rehash_kernel(const uint64_t* from, int64_t from_cap, Table to, ull* fail) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < from_cap; i += stride) {
    const uint64_t k = from[i];
    if (k == kEmpty) continue;
    bool won = false;
    const int64_t j = claim<kMaxProbe>(to.key, to.mask, mix64(k) & to.mask, k, &won);
    if (j < 0 || !won) atomicAdd(fail, 1ull);
  }
}

// lastnc[i] = -1 where i is a candidate, else i (the max-scan's input).
__global__ void score_kernel(const int32_t* ids, const uint32_t* slot, int64_t n, const ull* cnt, const ull* pair_count,
                             long long min_count, float threshold, int32_t* lastnc) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const float fn = (float)n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint32_t s = slot[i];
    bool cand = false;
    if (s != kNone) {
      const long long pab = (long long)pair_count[s];
      const float score = (float)(pab - min_count) / (float)cnt[ids[i - 1]] / (float)cnt[ids[i]] * fn;
      cand = score > threshold;
    }
    lastnc[i] = cand ? -1 : (int32_t)i;
  }
}

// z[i]: the last non-candidate at or before i. join[i] = candidate with an odd run ending at i.
__global__ void join_kernel(const int32_t* z, const uint32_t* slot, int64_t n, ull* firstjoin, int32_t* keep,
                            uint32_t* jslot) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t run = i - (int64_t)z[i];  // 0: not a candidate
    const bool join = (run & 1) != 0;
    keep[i] = join ? 0 : 1;
    uint32_t js = kNone;
    if (join) {
      js = slot[i];
      if ((ull)i < __hip_atomic_load(&firstjoin[js], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMin(&firstjoin[js], (ull)i);
    }
    jslot[i] = js;
  }
}

struct Joined {
  const ull* firstjoin;
  __host__ __device__ bool operator()(const int64_t& i) const { return firstjoin[i] != kNever; }
};

// The joined pairs in order of first joined occurrence get ids base, base + 1, ...
__global__ void assign_kernel(const int64_t* order, int64_t m, Table tab, int32_t base, int32_t* left, int32_t* right,
                              int64_t* joined) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += stride) {
    const int64_t s = order[k];
    const uint64_t key = tab.key[s] - 1;
    tab.pid[s] = base + (int32_t)k;
    left[k] = (int32_t)(key >> 32);
    right[k] = (int32_t)(key & 0xFFFFFFFFu);
    joined[k] = (int64_t)tab.joined[s];
  }
}

__global__ void write_kernel(const int32_t* ids, const int32_t* keep, const int32_t* outpos, const uint32_t* slot,
                             const int32_t* pid, int64_t n, int32_t* out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    if (!keep[i]) continue;
    int32_t v = ids[i];
    if (i + 1 < n && !keep[i + 1]) v = pid[slot[i + 1]];
    out[outpos[i]] = v;
  }
}

// out[s] = pos[offsets[s]] (total at the end of the stream), s in [0, n_sent].
__global__ void offsets_kernel(const int64_t* offsets, int64_t n_sent, const int32_t* pos, int64_t n, int64_t total,
                               int64_t* out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s <= n_sent; s += stride) {
    const int64_t o = offsets[s];
    out[s] = o < n ? (int64_t)pos[o] : total;
  }
}

__global__ void unpack_kernel(const uint64_t* keys, int64_t m, int32_t* left, int32_t* right) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += stride) {
    left[k] = (int32_t)(keys[k] >> 32);
    right[k] = (int32_t)(keys[k] & 0xFFFFFFFFu);
  }
}

__global__ void gather_pairs_kernel(const int64_t* slots, int64_t m, Table tab, uint64_t* keys, int64_t* counts) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += stride) {
    keys[k] = tab.key[slots[k]] - 1;
    counts[k] = (int64_t)tab.count[slots[k]];
  }
}

__global__ void map_kernel(const int32_t* ids, int64_t n, const int32_t* vidx, int32_t* tok, int32_t* kept) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int32_t v = vidx[ids[i]];
    tok[i] = v;
    kept[i] = v >= 0 ? 1 : 0;
  }
}

}  // namespace phrase
}  // namespace w2v

using namespace w2v::phrase;
using w2v::DevBuf;

namespace {

struct TableBuf {
  DevBuf<uint64_t> key;
  DevBuf<ull> count, joined, firstjoin;
  DevBuf<int32_t> pid;
  int64_t cap() const { return (int64_t)key.size(); }
  Table view() const {
    return Table{key.get(), count.get(), joined.get(), firstjoin.get(), pid.get(), (uint64_t)cap() - 1};
  }
  // Becomes an empty table of `cap` slots (a power of two).
  int alloc(int64_t cap, hipStream_t s) {
    TableBuf t;
    const size_t n = (size_t)cap;
    int rc;
    if ((rc = t.key.alloc(n)) || (rc = t.count.alloc(n)) || (rc = t.joined.alloc(n)) || (rc = t.firstjoin.alloc(n)) ||
        (rc = t.pid.alloc(n)))
      return rc;
    W2V_HIP_TRY(hipMemsetAsync(t.key.get(), 0, n * sizeof(uint64_t), s));
    W2V_HIP_TRY(hipMemsetAsync(t.count.get(), 0, n * sizeof(ull), s));
    W2V_HIP_TRY(hipMemsetAsync(t.joined.get(), 0, n * sizeof(ull), s));
    W2V_HIP_TRY(hipMemsetAsync(t.firstjoin.get(), 0xFF, n * sizeof(ull), s));
    *this = std::move(t);
    return W2V_OK;
  }
};

}  // namespace

struct w2v_phrase {
  int device = -1;  // -1 until the first device call resolves "current"
  hipStream_t stream = nullptr;
  int64_t initial_slots = 0;
  // the current stream
  bool loaded = false;
  int64_t n_words = 0, n_ids = 0, n_sentences = 0;
  DevBuf<int32_t> ids;
  DevBuf<int64_t> offsets;  // n_sentences + 1
  DevBuf<ull> cnt, first;   // n_words
  // the phrases of all passes, in id order (host)
  int64_t base_words = 0;
  std::vector<int32_t> left, right;
  std::vector<int64_t> joined;
  // the last pass
  TableBuf tab;
  int64_t n_bigrams = 0, n_joined = 0;
  double seconds[5] = {0, 0, 0, 0, 0};
  // the mapped samples
  bool mapped = false;
  DevBuf<int32_t> m_ids;
  DevBuf<int64_t> m_offsets;
  int64_t m_n = 0;
  std::vector<int64_t> hist;

  ~w2v_phrase() {  // the buffers free themselves after this
    if (stream) {
      (void)hipSetDevice(device);
      (void)hipStreamSynchronize(stream);
      (void)hipStreamDestroy(stream);
    }
  }
};

namespace {

// The device and the stream, on the first call that needs them (the argument
// checks of every call run before this).
int ensure_init(w2v_phrase* p) {
  if (p->stream) {
    W2V_HIP_TRY(hipSetDevice(p->device));
    return W2V_OK;
  }
  if (p->device < 0) W2V_HIP_TRY(hipGetDevice(&p->device));
  W2V_HIP_TRY(hipSetDevice(p->device));
  W2V_HIP_TRY(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
  return W2V_OK;
}

// cnt[w] and first[w] of ids[0, n) over n_words ids.
int histogram(w2v_phrase* p, const int32_t* ids, int64_t n, int64_t n_words, DevBuf<ull>& cnt, DevBuf<ull>& first) {
  const size_t m = (size_t)std::max<int64_t>(n_words, 1);
  int rc;
  if ((rc = cnt.alloc(m)) || (rc = first.alloc(m))) return rc;
  W2V_HIP_TRY(hipMemsetAsync(cnt.get(), 0, m * sizeof(ull), p->stream));
  W2V_HIP_TRY(hipMemsetAsync(first.get(), 0xFF, m * sizeof(ull), p->stream));
  if (n > 0) {
    hipLaunchKernelGGL(count_kernel<true>, grid_for(n / 16), dim3(kBlock), 0, p->stream,
                       reinterpret_cast<const uint32_t*>(ids), n, cnt.get(), first.get());
    W2V_HIP_TRY(hipGetLastError());
  }
  W2V_HIP_TRY(hipStreamSynchronize(p->stream));
  return W2V_OK;
}

// A new stream in the handle: everything an earlier one left goes.
void install(w2v_phrase* p, DevBuf<int32_t>& ids, DevBuf<int64_t>& offsets, DevBuf<ull>& cnt, DevBuf<ull>& first,
             int64_t n, int64_t n_sent, int64_t n_words) {
  p->ids = std::move(ids), p->offsets = std::move(offsets), p->cnt = std::move(cnt), p->first = std::move(first);
  p->n_ids = n, p->n_sentences = n_sent, p->n_words = p->base_words = n_words;
  p->left.clear(), p->right.clear(), p->joined.clear();
  p->tab = TableBuf();
  p->n_bigrams = p->n_joined = 0;
  p->mapped = false;
  p->loaded = true;
}

struct Clock {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  double lap() {
    const auto t1 = std::chrono::steady_clock::now();
    const double s = std::chrono::duration<double>(t1 - t0).count();
    t0 = t1;
    return s;
  }
};

}  // namespace

extern "C" {

int w2v_phrase_create(int32_t device, w2v_phrase** out) {
  if (!out) return w2v::set_error(W2V_ERR_ARG, "w2v_phrase_create: null argument");
  *out = nullptr;
  if (device < -1) return w2v::set_error(W2V_ERR_ARG, "w2v_phrase_create: device must be >= -1");
  w2v_phrase* p = new w2v_phrase();
  p->device = device;
  *out = p;
  return W2V_OK;
}

void w2v_phrase_destroy(w2v_phrase* p) { delete p; }

int w2v_phrase_set_table(w2v_phrase* p, int64_t initial_slots) {
  if (!p) return w2v::set_error(W2V_ERR_ARG, "w2v_phrase_set_table: null handle");
  if (initial_slots < 0 || initial_slots > kMaxCap)
    return w2v::set_error(W2V_ERR_ARG, "w2v_phrase_set_table: initial_slots must be in [0, 2^30]");
  p->initial_slots = initial_slots == 0 ? 0 : pow2_at_least(std::max<int64_t>(initial_slots, 2));
  return W2V_OK;
}

int w2v_phrase_upload(w2v_phrase* p, const int32_t* ids, int64_t n, const int64_t* offsets, int64_t n_sent,
                      int64_t n_words) {
  if (!p || !offsets || (n > 0 && !ids)) return w2v::set_error(W2V_ERR_ARG, "w2v_phrase_upload: null argument");
  if (n < 0 || n_sent < 0 || n_words < 0) return w2v::set_error(W2V_ERR_ARG, "w2v_phrase_upload: negative size");
  if (n_words >= kMaxWords) return w2v::set_error(W2V_ERR_ARG, "w2v_phrase_upload: n_words must be < 2^31");
  if (n > kMaxTokens) return w2v::set_error(W2V_ERR_UNSUPPORTED, "w2v_phrase_upload: a stream holds < 2^31 - 64 tokens");
  if (offsets[0] != 0 || offsets[n_sent] != n)
    return w2v::set_error(W2V_ERR_ARG, "w2v_phrase_upload: sentence offsets must span [0, n_ids]");
  for (int64_t s = 0; s < n_sent; ++s)
    if (offsets[s] > offsets[s + 1]) return w2v::set_error(W2V_ERR_ARG, "w2v_phrase_upload: sentence offsets must be non-decreasing");
  for (int64_t i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= n_words) return w2v::set_error(W2V_ERR_ARG, "w2v_phrase_upload: token id outside [0, n_words)");
  w2v::Range range_("w2v_phrase_upload");
  if (int rc = ensure_init(p)) return rc;
  DevBuf<int32_t> d_ids;
  DevBuf<int64_t> d_off;
  DevBuf<ull> cnt, first;
  int rc;
  if ((rc = d_ids.alloc((size_t)std::max<int64_t>(n, 1))) || (rc = d_off.alloc((size_t)n_sent + 1))) return rc;
  if (n > 0) W2V_HIP_TRY(hipMemcpyAsync(d_ids.get(), ids, n * sizeof(int32_t), hipMemcpyHostToDevice, p->stream));
  W2V_HIP_TRY(hipMemcpyAsync(d_off.get(), offsets, (n_sent + 1) * sizeof(int64_t), hipMemcpyHostToDevice, p->stream));
  if ((rc = histogram(p, d_ids.get(), n, n_words, cnt, first))) return rc;
  install(p, d_ids, d_off, cnt, first, n, n_sent, n_words);
  return W2V_OK;
}

int w2v_phrase_adopt_ingest(w2v_phrase* p, w2v_ingest* g) {
  if (!p || !g) return w2v::set_error(W2V_ERR_ARG, "w2v_phrase_adopt_ingest: null argument");
  const w2v::IngestView v = w2v::ingest_view(g);
  if (!v.ok) return w2v::set_error(W2V_ERR_STATE, "w2v_phrase_adopt_ingest: map the ingest first");
  if (p->device >= 0 && v.device != p->device)
    return w2v::set_error(W2V_ERR_ARG, "w2v_phrase_adopt_ingest: ingest on another device");
  if (v.n_ids > kMaxTokens)
    return w2v::set_error(W2V_ERR_UNSUPPORTED, "w2v_phrase_adopt_ingest: a stream holds < 2^31 - 64 tokens");
  w2v::Range range_("w2v_phrase_adopt_ingest");
  if (int rc = ensure_init(p)) return rc;
  if (v.device != p->device) return w2v::set_error(W2V_ERR_ARG, "w2v_phrase_adopt_ingest: ingest on another device");
  DevBuf<int32_t> d_ids;
  DevBuf<int64_t> d_off;
  DevBuf<ull> cnt, first;
  int rc;
  if ((rc = d_ids.alloc((size_t)std::max<int64_t>(v.n_ids, 1))) || (rc = d_off.alloc((size_t)v.n_sentences + 1)))
    return rc;
  if (v.n_ids > 0)
    W2V_HIP_TRY(hipMemcpyAsync(d_ids.get(), v.ids, v.n_ids * sizeof(int32_t), hipMemcpyDeviceToDevice, p->stream));
  W2V_HIP_TRY(hipMemcpyAsync(d_off.get(), v.offsets, (v.n_sentences + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice,
                             p->stream));
  if ((rc = histogram(p, d_ids.get(), v.n_ids, v.n_vocab, cnt, first))) return rc;
  install(p, d_ids, d_off, cnt, first, v.n_ids, v.n_sentences, v.n_vocab);
  return W2V_OK;
}

int w2v_phrase_pass(w2v_phrase* p, int64_t min_count, float threshold) {
  if (!p) return w2v::set_error(W2V_ERR_ARG, "w2v_phrase_pass: null handle");
  if (min_count < 1) return w2v::set_error(W2V_ERR_ARG, "w2v_phrase_pass: min_count must be >= 1");
  if (!std::isfinite(threshold) || threshold < 0.0f)
    return w2v::set_error(W2V_ERR_ARG, "w2v_phrase_pass: threshold must be finite and >= 0");
  if (!p->loaded) return w2v::set_error(W2V_ERR_STATE, "w2v_phrase_pass: upload or adopt a stream first");
  w2v::Range range_("w2v_phrase_pass");
  if (int rc = ensure_init(p)) return rc;
  const int64_t n = p->n_ids, S = p->n_sentences;
  hipStream_t st = p->stream;
  int rc;
  // the table: automatic = the power of two >= n within [2^16, 2^26] (a corpus has about n / 2 distinct
  // pairs: at most half full without growing); it doubles whenever it passes half full
  int64_t cap = p->initial_slots > 0 ? p->initial_slots
                                     : std::min<int64_t>(std::max<int64_t>(pow2_at_least(n), (int64_t)1 << 16),
                                                         (int64_t)1 << 26);
  TableBuf tab;
  if ((rc = tab.alloc(cap, st))) return rc;
  double sec[5] = {0, 0, 0, 0, 0};
  if (n == 0) {
    p->tab = std::move(tab);
    p->n_bigrams = p->n_joined = 0;
    std::copy(sec, sec + 5, p->seconds);
    p->mapped = false;
    return W2V_OK;
  }
  DevBuf<uint8_t> start;
  DevBuf<uint32_t> slot, jslot;
  DevBuf<int32_t> lastnc, z, keep, outpos;
  DevBuf<ull> ctr;  // [0] used slots, [1] positions that found no slot
  if ((rc = start.alloc((size_t)n)) || (rc = slot.alloc((size_t)n)) || (rc = jslot.alloc((size_t)n)) ||
      (rc = lastnc.alloc((size_t)n)) || (rc = z.alloc((size_t)n)) || (rc = keep.alloc((size_t)n)) ||
      (rc = outpos.alloc((size_t)n)) || (rc = ctr.alloc(2)))
    return rc;
  W2V_HIP_TRY(hipMemsetAsync(start.get(), 0, (size_t)n, st));
  W2V_HIP_TRY(hipMemsetAsync(ctr.get(), 0, 2 * sizeof(ull), st));
  hipLaunchKernelGGL(starts_kernel, grid_for(S), dim3(kBlock), 0, st, p->offsets.get(), S, start.get());
  W2V_HIP_TRY(hipGetLastError());
  W2V_HIP_TRY(hipStreamSynchronize(st));
  Clock clock;
  // insert until every eligible position has its slot and the table is at most half full
  ull used = 0;
  for (;;) {
    W2V_HIP_TRY(hipMemsetAsync(ctr.get() + 1, 0, sizeof(ull), st));
    hipLaunchKernelGGL(insert_kernel, grid_for(n), dim3(kBlock), 0, st, p->ids.get(), start.get(), n, p->cnt.get(),
                       (ull)min_count, tab.view(), slot.get(), ctr.get(), ctr.get() + 1);
    W2V_HIP_TRY(hipGetLastError());
    ull c[2] = {0, 0};
    W2V_HIP_TRY(hipMemcpyAsync(c, ctr.get(), sizeof(c), hipMemcpyDeviceToHost, st));
    W2V_HIP_TRY(hipStreamSynchronize(st));
    used = c[0];
    if (c[1] == 0 && (int64_t)used * 2 <= tab.cap()) break;
    auto rehash = [&](const TableBuf& from, const TableBuf& to) {  // the keys alone: the counts are still zero
      hipLaunchKernelGGL(rehash_kernel, grid_for(from.cap()), dim3(kBlock), 0, st, from.key.get(), from.cap(), to.view(),
                         ctr.get() + 1);
    };
    if ((rc = grow(st, tab, (int64_t)used, ctr.get() + 1, rehash, "w2v_phrase_pass: more than 2^29 distinct pairs",
                   "w2v_phrase_pass: rehash lost pairs")))
      return rc;
  }
  sec[1] = clock.lap();
  hipLaunchKernelGGL(count_kernel<false>, grid_for(n / 16), dim3(kBlock), 0, st, slot.get(), n, tab.count.get(),
                     (ull*)nullptr);
  W2V_HIP_TRY(hipGetLastError());
  W2V_HIP_TRY(hipStreamSynchronize(st));
  sec[2] = clock.lap();
  // candidates and joins
  hipLaunchKernelGGL(score_kernel, grid_for(n), dim3(kBlock), 0, st, p->ids.get(), slot.get(), n, p->cnt.get(),
                     tab.count.get(), (long long)min_count, threshold, lastnc.get());
  W2V_HIP_TRY(hipGetLastError());
  {
    size_t tb = 0;
    W2V_HIP_TRY(hipcub::DeviceScan::InclusiveScan(nullptr, tb, lastnc.get(), z.get(), hipcub::Max(), (int)n, st));
    DevBuf<unsigned char> tmp;
    if ((rc = tmp.alloc(std::max<size_t>(tb, 1)))) return rc;
    W2V_HIP_TRY(hipcub::DeviceScan::InclusiveScan(tmp.get(), tb, lastnc.get(), z.get(), hipcub::Max(), (int)n, st));
    hipLaunchKernelGGL(join_kernel, grid_for(n), dim3(kBlock), 0, st, z.get(), slot.get(), n, tab.firstjoin.get(),
                       keep.get(), jslot.get());
    W2V_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(count_kernel<false>, grid_for(n / 16), dim3(kBlock), 0, st, jslot.get(), n, tab.joined.get(),
                       (ull*)nullptr);
    W2V_HIP_TRY(hipGetLastError());
    W2V_HIP_TRY(hipStreamSynchronize(st));
  }
  sec[3] = clock.lap();
  // rewrite: phrase ids by first joined position, output positions, the new stream
  DevBuf<int64_t> order;
  DevBuf<ull> sorted;
  int64_t P = 0;
  const Table tv = tab.view();
  if ((rc = select_sorted(st, tab.cap(), Joined{tv.firstjoin}, tv.firstjoin, order, sorted, &P))) return rc;
  if (p->n_words + P >= kMaxWords)
    return w2v::set_error(W2V_ERR_UNSUPPORTED, "w2v_phrase_pass: words + phrases must stay below 2^31");
  std::vector<int32_t> h_left((size_t)P), h_right((size_t)P);
  std::vector<int64_t> h_joined((size_t)P);
  if (P > 0) {
    DevBuf<int32_t> d_left, d_right;
    DevBuf<int64_t> d_joined;
    if ((rc = d_left.alloc((size_t)P)) || (rc = d_right.alloc((size_t)P)) || (rc = d_joined.alloc((size_t)P))) return rc;
    hipLaunchKernelGGL(assign_kernel, grid_for(P), dim3(kBlock), 0, st, order.get(), P, tv, (int32_t)p->n_words,
                       d_left.get(), d_right.get(), d_joined.get());
    W2V_HIP_TRY(hipGetLastError());
    W2V_HIP_TRY(hipMemcpyAsync(h_left.data(), d_left.get(), P * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    W2V_HIP_TRY(hipMemcpyAsync(h_right.data(), d_right.get(), P * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    W2V_HIP_TRY(hipMemcpyAsync(h_joined.data(), d_joined.get(), P * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    W2V_HIP_TRY(hipStreamSynchronize(st));
  }
  int64_t n_out = 0;
  DevBuf<unsigned char> scratch;
  if ((rc = exclusive_sum(st, keep.get(), outpos.get(), n, &n_out, scratch))) return rc;
  DevBuf<int32_t> new_ids;
  DevBuf<int64_t> new_off;
  if ((rc = new_ids.alloc((size_t)std::max<int64_t>(n_out, 1))) || (rc = new_off.alloc((size_t)S + 1))) return rc;
  hipLaunchKernelGGL(write_kernel, grid_for(n), dim3(kBlock), 0, st, p->ids.get(), keep.get(), outpos.get(), slot.get(),
                     tv.pid, n, new_ids.get());
  W2V_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(offsets_kernel, grid_for(S + 1), dim3(kBlock), 0, st, p->offsets.get(), S, outpos.get(), n, n_out,
                     new_off.get());
  W2V_HIP_TRY(hipGetLastError());
  W2V_HIP_TRY(hipStreamSynchronize(st));
  sec[4] = clock.lap();
  DevBuf<ull> cnt, first;
  if ((rc = histogram(p, new_ids.get(), n_out, p->n_words + P, cnt, first))) return rc;
  sec[0] = clock.lap();
  // commit
  p->ids = std::move(new_ids), p->offsets = std::move(new_off), p->cnt = std::move(cnt), p->first = std::move(first);
  p->n_ids = n_out;
  p->n_words += P;
  p->left.insert(p->left.end(), h_left.begin(), h_left.end());
  p->right.insert(p->right.end(), h_right.begin(), h_right.end());
  p->joined.insert(p->joined.end(), h_joined.begin(), h_joined.end());
  p->tab = std::move(tab);
  p->n_bigrams = (int64_t)used;
  p->n_joined = n - n_out;
  std::copy(sec, sec + 5, p->seconds);
  p->mapped = false;
  return W2V_OK;
}

int w2v_phrase_summary(w2v_phrase* p, int64_t* n_words, int64_t* n_phrases, int64_t* n_ids, int64_t* n_sentences,
                       int64_t* n_bigrams, int64_t* n_joined) {
  if (!p) return w2v::set_error(W2V_ERR_ARG, "w2v_phrase_summary: null handle");
  if (!p->loaded) return w2v::set_error(W2V_ERR_STATE, "w2v_phrase_summary: upload or adopt a stream first");
  if (n_words) *n_words = p->n_words;
  if (n_phrases) *n_phrases = p->n_words - p->base_words;
  if (n_ids) *n_ids = p->n_ids;
  if (n_sentences) *n_sentences = p->n_sentences;
  if (n_bigrams) *n_bigrams = p->n_bigrams;
  if (n_joined) *n_joined = p->n_joined;
  return W2V_OK;
}

int w2v_phrase_times(w2v_phrase* p, double* seconds, int64_t* table_slots) {
  if (!p) return w2v::set_error(W2V_ERR_ARG, "w2v_phrase_times: null handle");
  if (seconds) std::copy(p->seconds, p->seconds + 5, seconds);
  if (table_slots) *table_slots = p->tab.cap();
  return W2V_OK;
}

int w2v_phrase_phrases(w2v_phrase* p, int32_t* left, int32_t* right, int64_t* joined) {
  if (!p) return w2v::set_error(W2V_ERR_ARG, "w2v_phrase_phrases: null handle");
  if (!p->loaded) return w2v::set_error(W2V_ERR_STATE, "w2v_phrase_phrases: upload or adopt a stream first");
  if (left) std::copy(p->left.begin(), p->left.end(), left);
  if (right) std::copy(p->right.begin(), p->right.end(), right);
  if (joined) std::copy(p->joined.begin(), p->joined.end(), joined);
  return W2V_OK;
}

int w2v_phrase_bigrams(w2v_phrase* p, int32_t* left, int32_t* right, int64_t* count) {
  if (!p) return w2v::set_error(W2V_ERR_ARG, "w2v_phrase_bigrams: null handle");
  if (!p->loaded) return w2v::set_error(W2V_ERR_STATE, "w2v_phrase_bigrams: upload or adopt a stream first");
  if (p->n_bigrams == 0) return W2V_OK;
  if (int rc = ensure_init(p)) return rc;
  hipStream_t st = p->stream;
  const Table tv = p->tab.view();
  DevBuf<int64_t> order;
  DevBuf<ull> sorted;
  int64_t m = 0;
  int rc;
  if ((rc = select_sorted(st, p->tab.cap(), Used{tv.key}, reinterpret_cast<const ull*>(tv.key), order, sorted, &m)))
    return rc;
  if (m != p->n_bigrams) return w2v::set_error(W2V_ERR_STATE, "w2v_phrase_bigrams: used-slot count mismatch");
  DevBuf<uint64_t> d_keys;
  DevBuf<int64_t> d_counts;
  DevBuf<int32_t> d_left, d_right;
  if ((rc = d_keys.alloc((size_t)m)) || (rc = d_counts.alloc((size_t)m)) || (rc = d_left.alloc((size_t)m)) ||
      (rc = d_right.alloc((size_t)m)))
    return rc;
  hipLaunchKernelGGL(gather_pairs_kernel, grid_for(m), dim3(kBlock), 0, st, order.get(), m, tv, d_keys.get(),
                     d_counts.get());
  W2V_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(unpack_kernel, grid_for(m), dim3(kBlock), 0, st, d_keys.get(), m, d_left.get(), d_right.get());
  W2V_HIP_TRY(hipGetLastError());
  if (left) W2V_HIP_TRY(hipMemcpyAsync(left, d_left.get(), m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (right) W2V_HIP_TRY(hipMemcpyAsync(right, d_right.get(), m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (count) W2V_HIP_TRY(hipMemcpyAsync(count, d_counts.get(), m * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  W2V_HIP_TRY(hipStreamSynchronize(st));
  return W2V_OK;
}

int w2v_phrase_words(w2v_phrase* p, int64_t* count, int64_t* first) {
  if (!p) return w2v::set_error(W2V_ERR_ARG, "w2v_phrase_words: null handle");
  if (!p->loaded) return w2v::set_error(W2V_ERR_STATE, "w2v_phrase_words: upload or adopt a stream first");
  if (p->n_words == 0) return W2V_OK;
  if (int rc = ensure_init(p)) return rc;
  // kNever reads as -1
  if (count) W2V_HIP_TRY(hipMemcpy(count, p->cnt.get(), p->n_words * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (first) W2V_HIP_TRY(hipMemcpy(first, p->first.get(), p->n_words * sizeof(int64_t), hipMemcpyDeviceToHost));
  return W2V_OK;
}

int w2v_phrase_stream(w2v_phrase* p, int32_t* ids, int64_t* offsets) {
  if (!p) return w2v::set_error(W2V_ERR_ARG, "w2v_phrase_stream: null handle");
  if (!p->loaded) return w2v::set_error(W2V_ERR_STATE, "w2v_phrase_stream: upload or adopt a stream first");
  if (int rc = ensure_init(p)) return rc;
  if (ids && p->n_ids > 0) W2V_HIP_TRY(hipMemcpy(ids, p->ids.get(), p->n_ids * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (offsets)
    W2V_HIP_TRY(hipMemcpy(offsets, p->offsets.get(), (p->n_sentences + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
  return W2V_OK;
}

int w2v_phrase_map(w2v_phrase* p, const int32_t* vocab_index, int64_t n_words) {
  if (!p || (n_words > 0 && !vocab_index)) return w2v::set_error(W2V_ERR_ARG, "w2v_phrase_map: null argument");
  if (!p->loaded) return w2v::set_error(W2V_ERR_STATE, "w2v_phrase_map: upload or adopt a stream first");
  if (n_words != p->n_words) return w2v::set_error(W2V_ERR_ARG, "w2v_phrase_map: one vocab index per id of the stream");
  w2v::Range range_("w2v_phrase_map");
  if (int rc = ensure_init(p)) return rc;  // the counts behind the vocab_index check are on the device
  hipStream_t st = p->stream;
  const int64_t n = p->n_ids, S = p->n_sentences;
  int rc;
  std::vector<int64_t> cnt((size_t)n_words), hist;  // tokens per vocab id, from the stream's counts
  if (n_words > 0) W2V_HIP_TRY(hipMemcpy(cnt.data(), p->cnt.get(), n_words * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (!vocab_hist(vocab_index, cnt.data(), n_words, hist))
    return w2v::set_error(W2V_ERR_ARG, "w2v_phrase_map: vocab_index entries must be >= -1");
  DevBuf<int32_t> m_ids;
  DevBuf<int64_t> m_off;
  int64_t kept = 0;
  if ((rc = m_off.alloc((size_t)S + 1))) return rc;
  if (n > 0) {
    DevBuf<int32_t> d_vidx, tok, flag, kpos;
    DevBuf<int64_t> n_sel;
    DevBuf<unsigned char> tmp;
    if ((rc = d_vidx.alloc((size_t)n_words)) || (rc = tok.alloc((size_t)n)) || (rc = flag.alloc((size_t)n)) ||
        (rc = kpos.alloc((size_t)n)) || (rc = n_sel.alloc(1)))
      return rc;
    W2V_HIP_TRY(hipMemcpyAsync(d_vidx.get(), vocab_index, n_words * sizeof(int32_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(map_kernel, grid_for(n), dim3(kBlock), 0, st, p->ids.get(), n, d_vidx.get(), tok.get(),
                       flag.get());
    W2V_HIP_TRY(hipGetLastError());
    if ((rc = exclusive_sum(st, flag.get(), kpos.get(), n, &kept, tmp))) return rc;
    if ((rc = m_ids.alloc((size_t)std::max<int64_t>(kept, 1)))) return rc;
    size_t tb = 0;
    W2V_HIP_TRY(hipcub::DeviceSelect::If(nullptr, tb, tok.get(), m_ids.get(), n_sel.get(), (int)n, NotNegative(), st));
    if ((rc = tmp.alloc(std::max<size_t>(tb, 1)))) return rc;
    W2V_HIP_TRY(hipcub::DeviceSelect::If(tmp.get(), tb, tok.get(), m_ids.get(), n_sel.get(), (int)n, NotNegative(), st));
    hipLaunchKernelGGL(offsets_kernel, grid_for(S + 1), dim3(kBlock), 0, st, p->offsets.get(), S, kpos.get(), n, kept,
                       m_off.get());
    W2V_HIP_TRY(hipGetLastError());
    int64_t sel = 0;
    W2V_HIP_TRY(hipMemcpyAsync(&sel, n_sel.get(), sizeof(int64_t), hipMemcpyDeviceToHost, st));
    W2V_HIP_TRY(hipStreamSynchronize(st));
    if (sel != kept) return w2v::set_error(W2V_ERR_STATE, "w2v_phrase_map: kept-token count mismatch");
  } else {
    if ((rc = m_ids.alloc(1))) return rc;
    W2V_HIP_TRY(hipMemsetAsync(m_off.get(), 0, (S + 1) * sizeof(int64_t), st));
    W2V_HIP_TRY(hipStreamSynchronize(st));
  }
  p->m_ids = std::move(m_ids), p->m_offsets = std::move(m_off);
  p->m_n = kept;
  p->hist = std::move(hist);
  p->mapped = true;
  return W2V_OK;
}

int w2v_phrase_samples_size(w2v_phrase* p, int64_t* n_ids, int64_t* n_sentences, int64_t* train_words) {
  if (!p) return w2v::set_error(W2V_ERR_ARG, "w2v_phrase_samples_size: null handle");
  if (!p->mapped) return w2v::set_error(W2V_ERR_STATE, "w2v_phrase_map first");
  if (n_ids) *n_ids = p->m_n;
  if (n_sentences) *n_sentences = p->n_sentences;
  if (train_words) *train_words = p->n_ids;
  return W2V_OK;
}

int w2v_phrase_download(w2v_phrase* p, int32_t* ids, int64_t* offsets) {
  if (!p) return w2v::set_error(W2V_ERR_ARG, "w2v_phrase_download: null handle");
  if (!p->mapped) return w2v::set_error(W2V_ERR_STATE, "w2v_phrase_map first");
  if (int rc = ensure_init(p)) return rc;
  if (ids && p->m_n > 0) W2V_HIP_TRY(hipMemcpy(ids, p->m_ids.get(), p->m_n * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (offsets)
    W2V_HIP_TRY(hipMemcpy(offsets, p->m_offsets.get(), (p->n_sentences + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
  return W2V_OK;
}

}  // extern "C"

namespace w2v {
IngestView phrase_view(const w2v_phrase* p) {
  IngestView v{};
  if (!p || !p->mapped) return v;
  v.device = p->device;
  v.ids = p->m_ids.get();
  v.n_ids = p->m_n;
  v.offsets = p->m_offsets.get();
  v.n_sentences = p->n_sentences;
  v.train_words = p->n_ids;
  v.hist = p->hist.data();
  v.n_vocab = (int64_t)p->hist.size();
  v.ok = true;
  return v;
}
}  // namespace w2v
