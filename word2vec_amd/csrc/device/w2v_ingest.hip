// w2v_ingest.hip — corpus ingestion on the GPU (include/w2v_ingest.h): the
// vocabulary count (Word2Vec.cpp:134-141) and build_sample's id mapping
// (:212-230) of a corpus file, bit-exact with the host readers
// (csrc/host/corpus.cpp, which match line_docs, Word2Vec.cpp:19-30, and the
// CLI's text8 reader, main.cpp:63-92).
//
// Per chunk of the file (cut after a whitespace byte, after '\n' for lines):
//   * token starts: a byte that is not C-locale whitespace after one that is
//     (or at the chunk start) — flags, then a device select into positions;
//   * per token (one thread): its end, two 64-bit hashes of its bytes, and the
//     newlines between it and the next token (the line index of a token is
//     the newlines before it: a scan of those counts);
//   * pass 1, insert: find or claim the token's slot in an open-addressing
//     table keyed by the first hash (compare-and-swap on the key) and lower
//     the slot's first byte offset (atomic min, only when smaller: after the
//     first occurrences nearly every token only reads). Idempotent, so a
//     chunk that fills the table past half is re-inserted after the table
//     doubles (rehash kernel);
//   * pass 1, count: one add per token on its slot, aggregated per workgroup
//     in an LDS table first (Zipf corpora: the hot words' adds stay in LDS,
//     one global add per distinct word per workgroup);
//   * the used slots, sorted by first occurrence on the device (select +
//     radix sort), are the words in the order the host map needs;
//   * pass 2: look the token up, check the second hash and the length against
//     the slot's (a collision of the first hash between two different words
//     fails the call rather than merging them), map to the vocab index, and
//     append the in-vocab ids (a device select). Sentence offsets without
//     atomics: the exclusive scan of the kept flags gives each token's output
//     position, and the token that opens sentence s writes offsets[s] (text8:
//     raw token index 1000 s; lines: the first token of a line, which also
//     writes the offsets of the empty lines before it).
// The table's probe loops, the count kernel, the ordering of the used slots and
// the growth step are w2v_table.hpp's, shared with w2v_phrase.hip; the columns,
// the key, insert_kernel and the payload-moving rehash_kernel are this unit's.
// The per-word token histogram the training handle needs (flush scales,
// w2v_dev_adopt_corpus) is the vocab words' counts from pass 1.
// The work is byte- and hash-table-bound, far from the HBM roofline: the
// point is taking the counting and mapping of a multi-GB corpus off the host.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "w2v_dev_internal.hpp"
#include "w2v_ingest.h"
#include "w2v_table.hpp"

namespace w2v {
namespace ingest {

using namespace w2v::table;

constexpr int64_t kText8Sentence = 1000;  // main.cpp:66
constexpr int kMaxProbe = 4096;           // a longer chain counts as a full table (the table grows)
constexpr int64_t kResidentMax = (int64_t)64 << 30;  // default: bytes of corpus kept in HBM between the passes

__device__ __forceinline__ bool is_space(unsigned char c) {  // C-locale isspace, as operator>>
  return c == ' ' || c == '\t' || c == '\n' || c == '\v' || c == '\f' || c == '\r';
}

// Token starts, compacted without a byte-flag array: a workgroup takes a
// 4 KiB tile (16 bytes per thread), counts its starts (pass a), the tile
// counts are scanned, and the workgroup writes its starts in order (pass b).
constexpr int kTileBytes = 4096;
constexpr int kPerThread = kTileBytes / 256;

__device__ __forceinline__ int starts_in(const unsigned char* b, int64_t n, int64_t i0, uint32_t* mask) {
  int c = 0;
  uint32_t m = 0;
  *mask = 0;
  if (i0 >= n) return 0;
  bool prev_space = i0 == 0 ? true : is_space(b[i0 - 1]);
  for (int k = 0; k < kPerThread; ++k) {
    const int64_t i = i0 + k;
    if (i >= n) break;
    const bool sp = is_space(b[i]);
    if (!sp && prev_space) {
      ++c;
      m |= 1u << k;
    }
    prev_space = sp;
  }
  *mask = m;
  return c;
}

__global__ __launch_bounds__(256) void tile_count_kernel(const unsigned char* b, int64_t n, int64_t* tile_count) {
  __shared__ int sum;
  if (threadIdx.x == 0) sum = 0;
  __syncthreads();
  uint32_t m;
  const int c = starts_in(b, n, (int64_t)blockIdx.x * kTileBytes + (int64_t)threadIdx.x * kPerThread, &m);
  if (c) atomicAdd(&sum, c);
  __syncthreads();
  if (threadIdx.x == 0) tile_count[blockIdx.x] = sum;
}

__global__ __launch_bounds__(256) void tile_write_kernel(const unsigned char* b, int64_t n, const int64_t* tile_pos,
                                                         int64_t* starts) {
  __shared__ int sh[256];
  uint32_t m;
  const int64_t i0 = (int64_t)blockIdx.x * kTileBytes + (int64_t)threadIdx.x * kPerThread;
  const int c = starts_in(b, n, i0, &m);
  sh[threadIdx.x] = c;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {  // inclusive scan of the per-thread counts
    const int v = threadIdx.x >= (unsigned)off ? sh[threadIdx.x - off] : 0;
    __syncthreads();
    sh[threadIdx.x] += v;
    __syncthreads();
  }
  int64_t pos = tile_pos[blockIdx.x] + sh[threadIdx.x] - c;
  while (m) {
    const int k = __builtin_ctz(m);
    m &= m - 1;
    starts[pos++] = i0 + k;
  }
}

// One token: its length, two hashes, and the newlines before the next token.
struct Tok {
  uint32_t len;
  uint32_t nl_after;
  uint64_t h1, h2;
};

__device__ __forceinline__ Tok read_token(const unsigned char* b, int64_t n, int64_t s) {
  Tok t;
  uint64_t f = 1469598103934665603ull;  // FNV-1a
  uint64_t m = 0x9E3779B97F4A7C15ull;   // multiplicative rolling hash, another prime
  int64_t e = s;
  while (e < n && !is_space(b[e])) {
    const unsigned char c = b[e];
    f = (f ^ c) * 1099511628211ull;
    m = (m + c + 1) * 0xC2B2AE3D27D4EB4Full;
    ++e;
  }
  t.len = (uint32_t)(e - s);
  t.h1 = mix64(f ^ (uint64_t)t.len);
  if (t.h1 == kEmpty) t.h1 = 1;
  t.h2 = mix64(m + 0x165667B19E3779F9ull * (uint64_t)t.len);
  uint32_t nl = 0;
  while (e < n && is_space(b[e])) {
    nl += b[e] == '\n';
    ++e;
  }
  t.nl_after = nl;
  return t;
}

struct Table {
  uint64_t* key;  // first hash, 0 = empty
  uint64_t* h2;
  unsigned long long* first;  // smallest byte offset seen
  unsigned long long* count;
  uint32_t* len;
  uint64_t mask;
};

// Pass 1, insert (idempotent). base_off: the chunk's byte offset in the file.
// The key is the first hash, already mixed: its home slot is h1 & mask.
__global__ void insert_kernel(const unsigned char* b, int64_t n, const int64_t* starts, int64_t nt, int64_t base_off,
                              Table tab, uint32_t* slot, uint32_t* nl_after, unsigned long long* used,
                              unsigned long long* fail) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nt; t += stride) {
    const int64_t s = starts[t];
    const Tok k = read_token(b, n, s);
    nl_after[t] = k.nl_after;
    bool won = false;
    const int64_t i = claim<kMaxProbe>(tab.key, tab.mask, k.h1 & tab.mask, k.h1, &won);
    if (i < 0) {
      atomicAdd(fail, 1ull);
      slot[t] = kNone;
      continue;
    }
    if (won) {
      tab.h2[i] = k.h2;
      tab.len[i] = k.len;
      atomicAdd(used, 1ull);
    }
    const unsigned long long off = (unsigned long long)(base_off + s);
    if (off < __hip_atomic_load(&tab.first[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&tab.first[i], off);
    slot[t] = (uint32_t)i;
  }
}

// Move every used slot of `from` into `to` (a larger, empty table).
__global__ void rehash_kernel(Table from, int64_t from_cap, Table to, unsigned long long* fail) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < from_cap; i += stride) {
    const uint64_t h1 = from.key[i];
    if (h1 == kEmpty) continue;
    bool won = false;
    const int64_t j = claim<kMaxProbe>(to.key, to.mask, h1 & to.mask, h1, &won);
    if (j < 0 || !won) {
      atomicAdd(fail, 1ull);
      continue;
    }
    to.h2[j] = from.h2[i];
    to.len[j] = from.len[i];
    to.first[j] = from.first[i];
    to.count[j] = from.count[i];
  }
}

__global__ void gather_words_kernel(const int64_t* order, int64_t m, Table tab, int64_t* first, int32_t* len,
                                    int64_t* count) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += stride) {
    const int64_t s = order[k];
    first[k] = (int64_t)tab.first[s];
    len[k] = (int32_t)tab.len[s];
    count[k] = (int64_t)tab.count[s];
  }
}

__global__ void scatter_ids_kernel(const int64_t* order, const int32_t* vidx, int64_t m, int32_t* slot_id) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += stride) slot_id[order[k]] = vidx[k];
}

// Pass 2: token -> vocab index (or -1) and its kept flag. Verifies the second hash and length.
__global__ void map_kernel(const unsigned char* b, int64_t n, const int64_t* starts, int64_t nt, Table tab,
                           const int32_t* slot_id, int32_t* tok_id, int32_t* kept, uint32_t* nl_after,
                           unsigned long long* mismatch) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nt; t += stride) {
    const Tok k = read_token(b, n, starts[t]);
    nl_after[t] = k.nl_after;
    const int64_t i = find(tab.key, tab.mask, k.h1 & tab.mask, k.h1);
    int32_t id = -1;
    if (i < 0) {
      atomicAdd(mismatch, 1ull);  // pass 2 saw a word pass 1 did not (different bytes)
    } else {
      if (tab.h2[i] != k.h2 || tab.len[i] != k.len) atomicAdd(mismatch, 1ull);
      id = slot_id[i];
    }
    tok_id[t] = id;
    kept[t] = id >= 0 ? 1 : 0;
  }
}

// offsets[s] = kept tokens before sentence s, written by the token that opens s.
// text8: raw token 1000 s. lines: the first token of line L writes offsets[l]
// for l in (previous token's line, L] (the empty lines before it too).
__global__ void boundary_kernel(const int32_t* kpos, const int64_t* line_of, int64_t nt, int64_t raw_base,
                                int64_t kept_base, int64_t prev_line, int text8, int64_t* offsets) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nt; t += stride) {
    const int64_t pos = kept_base + kpos[t];
    if (text8) {
      const int64_t r = raw_base + t;
      if (r > 0 && r % kText8Sentence == 0) offsets[r / kText8Sentence] = pos;
    } else {
      const int64_t L = line_of[t];
      const int64_t P = t > 0 ? line_of[t - 1] : prev_line;
      for (int64_t l = P + 1; l <= L; ++l) offsets[l] = pos;
    }
  }
}

__global__ void fill_kernel(int64_t* p, int64_t lo, int64_t hi, int64_t v) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += stride) p[i] = v;
}

__global__ void add_base_kernel(int64_t* l, int64_t m, int64_t base) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < m; t += stride) l[t] += base;
}

}  // namespace ingest
}  // namespace w2v

using namespace w2v::ingest;

using w2v::DevBuf;

// The hash table's memory; the kernels take its view.
struct TableBuf {
  DevBuf<uint64_t> key, h2;
  DevBuf<unsigned long long> first, count;
  DevBuf<uint32_t> len;
  int64_t cap() const { return (int64_t)key.size(); }
  Table view() const { return Table{key.get(), h2.get(), first.get(), count.get(), len.get(), (uint64_t)cap() - 1}; }
  // Becomes an empty table of `cap` slots (a power of two).
  int alloc(int64_t cap, hipStream_t s) {
    TableBuf t;
    const size_t n = (size_t)cap;
    int rc;
    if ((rc = t.key.alloc(n)) || (rc = t.h2.alloc(n)) || (rc = t.first.alloc(n)) || (rc = t.count.alloc(n)) ||
        (rc = t.len.alloc(n)))
      return rc;
    W2V_HIP_TRY(hipMemsetAsync(t.key.get(), 0, n * sizeof(uint64_t), s));
    W2V_HIP_TRY(hipMemsetAsync(t.first.get(), 0xFF, n * sizeof(unsigned long long), s));
    W2V_HIP_TRY(hipMemsetAsync(t.count.get(), 0, n * sizeof(unsigned long long), s));
    *this = std::move(t);
    return W2V_OK;
  }
};

// The chunk work buffers, sized together (ensure_work).
struct Work {
  DevBuf<unsigned char> buf;  // one chunk (the file is not resident), and a byte more
  DevBuf<int64_t> tile;       // per-4 KiB-tile start counts, then positions
  DevBuf<int64_t> starts;
  DevBuf<uint32_t> nl_after;
  DevBuf<uint32_t> slot;
  DevBuf<int64_t> line_of;
  DevBuf<int32_t> tok_id;
  DevBuf<int32_t> kept;
  DevBuf<int32_t> kpos;
  DevBuf<int64_t> n_sel;
  DevBuf<unsigned char> temp;  // scratch of the selects and scans
};

struct w2v_ingest {
  int device = 0;
  int format = W2V_INGEST_LINES;
  int64_t chunk = (int64_t)1 << 30;
  int64_t resident_max = kResidentMax;
  hipStream_t stream = nullptr;
  TableBuf tab;
  DevBuf<unsigned long long> ctr;  // [0] used slots, [1] probe failures, [2] mismatches
  // pass 1 results
  bool counted = false;
  int64_t n_bytes = 0, raw_tokens = 0, n_sentences = 0, n_words = 0;
  DevBuf<int64_t> order;  // the used slots in order of first occurrence
  std::vector<int64_t> word_count;  // host: pass-1 counts in that order
  // pass 2 results
  bool mapped = false;
  DevBuf<int32_t> ids;
  int64_t n_ids = 0;
  DevBuf<int64_t> offsets;  // n_sentences + 1
  std::vector<int64_t> hist;   // host: tokens per vocab id
  DevBuf<unsigned char> file;  // the whole file in HBM between pass 1 and pass 2 (<= kResidentMax)
  const unsigned char* cur = nullptr;  // device bytes of the current chunk
  Work w;

  ~w2v_ingest() {  // the buffers free themselves after this
    (void)hipSetDevice(device);
    if (stream) {
      (void)hipStreamSynchronize(stream);
      (void)hipStreamDestroy(stream);
    }
  }
};

namespace {

bool host_space(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\v' || c == '\f' || c == '\r'; }

// Chunks cut after a '\n' (lines) or a whitespace byte (text8), as corpus.cpp's split().
std::vector<std::pair<int64_t, int64_t>> chunks(const char* p, int64_t n, int64_t size, bool lines) {
  std::vector<std::pair<int64_t, int64_t>> r;
  int64_t b = 0;
  while (b < n) {
    int64_t e = std::min(n, b + size);
    while (e < n && !(lines ? p[e - 1] == '\n' : host_space(p[e - 1]))) ++e;
    r.emplace_back(b, e);
    b = e;
  }
  return r;
}

// Double the table until it holds `need` words at most half full; the rehash carries the words' payload.
int grow_words(w2v_ingest* g, int64_t need) {
  unsigned long long* fail = g->ctr.get() + 1;
  auto rehash = [&](const TableBuf& from, const TableBuf& to) {
    hipLaunchKernelGGL(rehash_kernel, grid_for(from.cap()), dim3(kBlock), 0, g->stream, from.view(), from.cap(),
                       to.view(), fail);
  };
  return grow(g->stream, g->tab, need, fail, rehash, "w2v_ingest_count: more than 2^29 distinct words",
              "w2v_ingest_count: rehash lost words");
}

// hipcub's element counts are int: a chunk is at most INT32_MAX - 64 bytes
// (chunk_size_limit; the callers cut the file into such chunks), so its tokens
// (<= bytes / 2 + 1), tiles (<= bytes / 4096 + 2), the table (<= 2^30 slots,
// kMaxCap) and the words (<= 2^29) all fit the (int) casts below.
int ensure_work(w2v_ingest* g, int64_t bytes) {
  if (bytes < 0 || bytes > (int64_t)INT32_MAX - 64)
    return w2v::set_error(W2V_ERR_UNSUPPORTED, "w2v_ingest: a chunk must be < 2^31 - 64 bytes (hipcub int counts)");
  if ((int64_t)g->w.buf.size() > bytes) return W2V_OK;
  Work w;
  const size_t max_tok = (size_t)bytes / 2 + 1;  // a token and its separator take >= 2 bytes
  const size_t n_tiles = (size_t)bytes / kTileBytes + 2;
  int rc;
  if ((rc = w.buf.alloc((size_t)bytes + 1)) || (rc = w.tile.alloc(n_tiles)) || (rc = w.starts.alloc(max_tok)) ||
      (rc = w.nl_after.alloc(max_tok)) || (rc = w.slot.alloc(max_tok)) || (rc = w.line_of.alloc(max_tok)) ||
      (rc = w.tok_id.alloc(max_tok)) || (rc = w.kept.alloc(max_tok)) || (rc = w.kpos.alloc(max_tok)) ||
      (rc = w.n_sel.alloc(1)))
    return rc;
  // scratch for the selects and scans at the largest size
  size_t t1 = 0, t2 = 0, t3 = 0, t4 = 0;
  const int nk = (int)std::min<size_t>(max_tok, INT32_MAX);
  W2V_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, t1, w.tile.get(), w.tile.get(), (int)n_tiles));
  W2V_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, t2, w.nl_after.get(), w.line_of.get(), nk));
  W2V_HIP_TRY(hipcub::DeviceSelect::If(nullptr, t3, w.tok_id.get(), w.tok_id.get(), w.n_sel.get(), nk, NotNegative()));
  W2V_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, t4, w.kept.get(), w.kpos.get(), nk));
  if ((rc = w.temp.alloc(std::max({t1, t2, t3, t4})))) return rc;
  g->w = std::move(w);
  return W2V_OK;
}

// The chunk's bytes on the device (copied unless the file is resident), and
// its token starts; returns the token count in *nt.
int tokenize(w2v_ingest* g, const char* data, int64_t off, int64_t n, int64_t* nt) {
  Work& w = g->w;
  if (g->file.get()) {
    g->cur = g->file.get() + off;
  } else {
    W2V_HIP_TRY(hipMemcpyAsync(w.buf.get(), data + off, n, hipMemcpyHostToDevice, g->stream));
    g->cur = w.buf.get();
  }
  const int64_t n_tiles = (n + kTileBytes - 1) / kTileBytes;
  if (n_tiles == 0) {
    *nt = 0;
    return W2V_OK;
  }
  int64_t* tile = w.tile.get();
  W2V_HIP_TRY(hipMemsetAsync(tile + n_tiles, 0, sizeof(int64_t), g->stream));
  hipLaunchKernelGGL(tile_count_kernel, dim3((unsigned)n_tiles), dim3(256), 0, g->stream, g->cur, n, tile);
  W2V_HIP_TRY(hipGetLastError());
  size_t tb = w.temp.size();
  W2V_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(w.temp.get(), tb, tile, tile, (int)n_tiles + 1, g->stream));
  hipLaunchKernelGGL(tile_write_kernel, dim3((unsigned)n_tiles), dim3(256), 0, g->stream, g->cur, n, tile,
                     w.starts.get());
  W2V_HIP_TRY(hipGetLastError());
  W2V_HIP_TRY(hipMemcpyAsync(nt, tile + n_tiles, sizeof(int64_t), hipMemcpyDeviceToHost, g->stream));
  W2V_HIP_TRY(hipStreamSynchronize(g->stream));
  return W2V_OK;
}

// Line index of each token of the chunk (line_base + newlines before it in the
// chunk); returns the newline count after the chunk's last token in *after.
int lines_of(w2v_ingest* g, int64_t nt, int64_t line_base, int64_t* last_line, int64_t* after) {
  Work& w = g->w;
  size_t tb = w.temp.size();
  W2V_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(w.temp.get(), tb, w.nl_after.get(), w.line_of.get(), (int)nt, g->stream));
  hipLaunchKernelGGL(add_base_kernel, grid_for(nt), dim3(kBlock), 0, g->stream, w.line_of.get(), nt, line_base);
  W2V_HIP_TRY(hipGetLastError());
  uint32_t last_nl = 0;
  W2V_HIP_TRY(hipMemcpyAsync(last_line, w.line_of.get() + nt - 1, sizeof(int64_t), hipMemcpyDeviceToHost, g->stream));
  W2V_HIP_TRY(hipMemcpyAsync(&last_nl, w.nl_after.get() + nt - 1, sizeof(uint32_t), hipMemcpyDeviceToHost, g->stream));
  W2V_HIP_TRY(hipStreamSynchronize(g->stream));
  *after = last_nl;
  return W2V_OK;
}

// Newlines before the chunk's first token (its leading whitespace).
int64_t leading_newlines(const char* p, int64_t n) {
  int64_t k = 0;
  for (int64_t i = 0; i < n && host_space(p[i]); ++i) k += p[i] == '\n';
  return k;
}

int64_t chunk_size_limit(const w2v_ingest* g) { return std::min<int64_t>(g->chunk, (int64_t)INT32_MAX - 64); }

// The used slots sorted by first occurrence -> g->order.
int order_words(w2v_ingest* g, int64_t n_words) {
  DevBuf<int64_t> order;
  DevBuf<unsigned long long> firsts_sorted;
  int64_t sel = 0;
  if (int rc = select_sorted(g->stream, g->tab.cap(), Used{g->tab.key.get()}, g->tab.first.get(), order, firsts_sorted,
                             &sel))
    return rc;
  if (sel != n_words) return w2v::set_error(W2V_ERR_STATE, "w2v_ingest_count: used-slot count mismatch");
  g->order = std::move(order);
  return W2V_OK;
}

// The first m words in g->order's order: first byte offset, length and count,
// each to the host array given (nullptr: not wanted).
int gather_words(w2v_ingest* g, int64_t m, int64_t* first_offset, int32_t* length, int64_t* count) {
  DevBuf<int64_t> d_first, d_count;
  DevBuf<int32_t> d_len;
  int rc;
  if ((rc = d_first.alloc((size_t)m)) || (rc = d_len.alloc((size_t)m)) || (rc = d_count.alloc((size_t)m))) return rc;
  hipLaunchKernelGGL(gather_words_kernel, grid_for(m), dim3(kBlock), 0, g->stream, g->order.get(), m, g->tab.view(),
                     d_first.get(), d_len.get(), d_count.get());
  W2V_HIP_TRY(hipGetLastError());
  if (first_offset)
    W2V_HIP_TRY(hipMemcpyAsync(first_offset, d_first.get(), m * sizeof(int64_t), hipMemcpyDeviceToHost, g->stream));
  if (length) W2V_HIP_TRY(hipMemcpyAsync(length, d_len.get(), m * sizeof(int32_t), hipMemcpyDeviceToHost, g->stream));
  if (count) W2V_HIP_TRY(hipMemcpyAsync(count, d_count.get(), m * sizeof(int64_t), hipMemcpyDeviceToHost, g->stream));
  W2V_HIP_TRY(hipStreamSynchronize(g->stream));
  return W2V_OK;
}

}  // namespace

extern "C" {

int w2v_ingest_create(int32_t device, int32_t format, int64_t chunk_bytes, w2v_ingest** out) {
  if (!out) return w2v::set_error(W2V_ERR_ARG, "w2v_ingest_create: null argument");
  *out = nullptr;
  if (format != W2V_INGEST_LINES && format != W2V_INGEST_TEXT8) return w2v::set_error(W2V_ERR_ARG, "bad ingest format");
  if (chunk_bytes < 0) return w2v::set_error(W2V_ERR_ARG, "chunk_bytes must be >= 0");
  w2v_ingest* g = new w2v_ingest();
  g->format = format;
  if (chunk_bytes > 0) g->chunk = std::max<int64_t>(chunk_bytes, 1 << 12);
  hipError_t e = hipSuccess;
  if (device >= 0) g->device = device;
  else e = hipGetDevice(&g->device);
  if (e == hipSuccess) e = hipSetDevice(g->device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    delete g;
    return w2v::set_error(W2V_ERR_HIP, std::string("w2v_ingest_create: ") + hipGetErrorString(e));
  }
  if (int rc = g->ctr.alloc(3)) {
    delete g;
    return rc;
  }
  *out = g;
  return W2V_OK;
}

void w2v_ingest_destroy(w2v_ingest* g) { delete g; }

int w2v_ingest_set_resident(w2v_ingest* g, int64_t max_bytes) {
  if (!g) return w2v::set_error(W2V_ERR_ARG, "null ingest");
  g->resident_max = max_bytes < 0 ? kResidentMax : max_bytes;
  return W2V_OK;
}

int w2v_ingest_count(w2v_ingest* g, const char* data, int64_t n) {
  if (!g || (n > 0 && !data) || n < 0) return w2v::set_error(W2V_ERR_ARG, "w2v_ingest_count: bad argument");
  w2v::Range range_("w2v_ingest_count");
  W2V_HIP_TRY(hipSetDevice(g->device));
  g->counted = g->mapped = false;
  const bool lines = g->format == W2V_INGEST_LINES;
  const auto cs = chunks(data, n, chunk_size_limit(g), lines);
  int64_t biggest = 0;
  for (auto& c : cs) biggest = std::max(biggest, c.second - c.first);
  if (biggest > (int64_t)INT32_MAX - 64) return w2v::set_error(W2V_ERR_UNSUPPORTED, "w2v_ingest_count: a line longer than 2 GiB");
  if (int rc = ensure_work(g, std::max<int64_t>(biggest, 1))) return rc;
  // a file that fits the residency budget crosses PCIe once: pass 2 reads this copy
  g->file.reset();
  // ... and only while it leaves at least half of the device's free memory to
  // the work buffers, the table and whatever trains next on this device
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
  if (n > 0 && n <= g->resident_max && (uint64_t)n <= (uint64_t)free_b / 2) {
    DevBuf<unsigned char> file;
    if (file.alloc((size_t)n) == W2V_OK) {
      W2V_HIP_TRY(hipMemcpyAsync(file.get(), data, n, hipMemcpyHostToDevice, g->stream));
      g->file = std::move(file);
    } else {
      (void)hipGetLastError();  // no room: stream the chunks in both passes instead
    }
  }
  // the table starts at 2^16..2^24 slots and doubles whenever it is half full
  int64_t cap = (int64_t)1 << 16;
  while (cap < std::min<int64_t>(n / 64, (int64_t)1 << 24)) cap <<= 1;
  if (int rc = g->tab.alloc(cap, g->stream)) return rc;
  W2V_HIP_TRY(hipMemsetAsync(g->ctr.get(), 0, 3 * sizeof(unsigned long long), g->stream));
  int64_t raw = 0, newlines = 0;
  for (auto& c : cs) {
    const int64_t len = c.second - c.first;
    int64_t nt = 0;
    if (int rc = tokenize(g, data, c.first, len, &nt)) return rc;
    newlines += leading_newlines(data + c.first, len);
    if (nt > 0) {
      for (;;) {  // insert until no token failed to find a slot and the table is at most half full
        W2V_HIP_TRY(hipMemsetAsync(g->ctr.get() + 1, 0, sizeof(unsigned long long), g->stream));
        hipLaunchKernelGGL(insert_kernel, grid_for(nt), dim3(kBlock), 0, g->stream, g->cur, len, g->w.starts.get(), nt,
                           c.first, g->tab.view(), g->w.slot.get(), g->w.nl_after.get(), g->ctr.get(), g->ctr.get() + 1);
        W2V_HIP_TRY(hipGetLastError());
        unsigned long long cnt[2] = {0, 0};
        W2V_HIP_TRY(hipMemcpyAsync(cnt, g->ctr.get(), sizeof(cnt), hipMemcpyDeviceToHost, g->stream));
        W2V_HIP_TRY(hipStreamSynchronize(g->stream));
        if (cnt[1] == 0 && (int64_t)cnt[0] * 2 <= g->tab.cap()) break;
        if (int rc = grow_words(g, (int64_t)cnt[0] + (int64_t)cnt[1])) return rc;
      }
      hipLaunchKernelGGL(count_kernel<false>, grid_for(nt / 16), dim3(kBlock), 0, g->stream, g->w.slot.get(), nt,
                         g->tab.count.get(), (ull*)nullptr);
      W2V_HIP_TRY(hipGetLastError());
      int64_t last_line = 0, after = 0;
      if (int rc = lines_of(g, nt, 0, &last_line, &after)) return rc;
      newlines += last_line + after;
    }
    raw += nt;
  }
  unsigned long long used = 0;
  W2V_HIP_TRY(hipMemcpy(&used, g->ctr.get(), sizeof(used), hipMemcpyDeviceToHost));
  if (int rc = order_words(g, (int64_t)used)) return rc;
  g->n_words = (int64_t)used;
  g->word_count.assign((size_t)used, 0);
  if (used > 0)
    if (int rc = gather_words(g, (int64_t)used, nullptr, nullptr, g->word_count.data())) return rc;
  g->n_bytes = n;
  g->raw_tokens = raw;
  // sentences: lines (getline: a final unterminated line counts when it holds bytes) or 1000-token cuts
  if (lines) g->n_sentences = newlines + ((n > 0 && data[n - 1] != '\n') ? 1 : 0);
  else g->n_sentences = (raw + kText8Sentence - 1) / kText8Sentence;
  g->counted = true;
  return W2V_OK;
}

int w2v_ingest_summary(w2v_ingest* g, int64_t* n_words, int64_t* raw_tokens, int64_t* n_sentences) {
  if (!g) return w2v::set_error(W2V_ERR_ARG, "null ingest");
  if (!g->counted) return w2v::set_error(W2V_ERR_STATE, "w2v_ingest_count first");
  if (n_words) *n_words = g->n_words;
  if (raw_tokens) *raw_tokens = g->raw_tokens;
  if (n_sentences) *n_sentences = g->n_sentences;
  return W2V_OK;
}

int w2v_ingest_words(w2v_ingest* g, int64_t* first_offset, int32_t* length, int64_t* count) {
  if (!g) return w2v::set_error(W2V_ERR_ARG, "null ingest");
  if (!g->counted) return w2v::set_error(W2V_ERR_STATE, "w2v_ingest_count first");
  const int64_t m = g->n_words;
  if (m == 0) return W2V_OK;
  W2V_HIP_TRY(hipSetDevice(g->device));
  return gather_words(g, m, first_offset, length, count);
}

int w2v_ingest_map(w2v_ingest* g, const char* data, int64_t n, const int32_t* vocab_index, int64_t n_words) {
  if (!g || (n > 0 && !data) || (n_words > 0 && !vocab_index)) return w2v::set_error(W2V_ERR_ARG, "w2v_ingest_map: null argument");
  if (!g->counted) return w2v::set_error(W2V_ERR_STATE, "w2v_ingest_count first");
  if (n != g->n_bytes || n_words != g->n_words) return w2v::set_error(W2V_ERR_ARG, "w2v_ingest_map: not the counted corpus");
  w2v::Range range_("w2v_ingest_map");
  W2V_HIP_TRY(hipSetDevice(g->device));
  g->mapped = false;
  std::vector<int64_t> hist;  // tokens per vocab id, from pass 1's counts
  if (!vocab_hist(vocab_index, g->word_count.data(), n_words, hist))
    return w2v::set_error(W2V_ERR_ARG, "vocab_index entries must be >= -1");
  // slot -> vocab index
  DevBuf<int32_t> d_slot, d_vidx, ids;
  DevBuf<int64_t> offsets;
  const int64_t cap = g->tab.cap();
  int rc;
  if ((rc = d_slot.alloc((size_t)cap))) return rc;
  W2V_HIP_TRY(hipMemsetAsync(d_slot.get(), 0xFF, cap * sizeof(int32_t), g->stream));
  if (n_words > 0) {
    if ((rc = d_vidx.alloc((size_t)n_words))) return rc;
    W2V_HIP_TRY(hipMemcpyAsync(d_vidx.get(), vocab_index, n_words * sizeof(int32_t), hipMemcpyHostToDevice, g->stream));
    hipLaunchKernelGGL(scatter_ids_kernel, grid_for(n_words), dim3(kBlock), 0, g->stream, g->order.get(), d_vidx.get(),
                       n_words, d_slot.get());
    W2V_HIP_TRY(hipGetLastError());
  }
  if ((rc = ids.alloc((size_t)std::max<int64_t>(g->raw_tokens, 1))) || (rc = offsets.alloc((size_t)g->n_sentences + 1)))
    return rc;
  W2V_HIP_TRY(hipMemsetAsync(offsets.get(), 0, (g->n_sentences + 1) * sizeof(int64_t), g->stream));
  unsigned long long* mismatch = g->ctr.get() + 2;
  W2V_HIP_TRY(hipMemsetAsync(mismatch, 0, sizeof(unsigned long long), g->stream));
  const bool lines = g->format == W2V_INGEST_LINES;
  const auto cs = chunks(data, n, chunk_size_limit(g), lines);
  Work& w = g->w;
  int64_t raw = 0, kept = 0, line_base = 0, prev_line = -1;
  for (auto& c : cs) {
    const int64_t len = c.second - c.first;
    int64_t nt = 0;
    if ((rc = tokenize(g, data, c.first, len, &nt))) return rc;
    line_base += leading_newlines(data + c.first, len);
    if (nt > 0) {
      hipLaunchKernelGGL(map_kernel, grid_for(nt), dim3(kBlock), 0, g->stream, g->cur, len, w.starts.get(), nt,
                         g->tab.view(), d_slot.get(), w.tok_id.get(), w.kept.get(), w.nl_after.get(), mismatch);
      W2V_HIP_TRY(hipGetLastError());
      int64_t last_line = 0, after = 0;
      if ((rc = lines_of(g, nt, line_base, &last_line, &after))) return rc;
      int64_t sel = 0;  // the chunk's in-vocab tokens (w.temp holds the scan's scratch at the largest size: ensure_work)
      if ((rc = exclusive_sum(g->stream, w.kept.get(), w.kpos.get(), nt, &sel, w.temp))) return rc;
      hipLaunchKernelGGL(boundary_kernel, grid_for(nt), dim3(kBlock), 0, g->stream, w.kpos.get(), w.line_of.get(), nt,
                         raw, kept, prev_line, lines ? 0 : 1, offsets.get());
      W2V_HIP_TRY(hipGetLastError());
      // append the chunk's in-vocab ids
      size_t tb = w.temp.size();
      W2V_HIP_TRY(hipcub::DeviceSelect::If(w.temp.get(), tb, w.tok_id.get(), ids.get() + kept, w.n_sel.get(), (int)nt,
                                           NotNegative(), g->stream));
      kept += sel;
      prev_line = last_line;
      line_base = last_line + after;
    }
    raw += nt;
  }
  if (raw != g->raw_tokens) return w2v::set_error(W2V_ERR_STATE, "w2v_ingest_map: token count differs from pass 1");
  // the sentences after the last token's (lines: trailing empty lines) and the end
  const int64_t tail = lines ? prev_line + 1 : g->n_sentences;
  hipLaunchKernelGGL(fill_kernel, grid_for(g->n_sentences + 1 - tail), dim3(kBlock), 0, g->stream, offsets.get(), tail,
                     g->n_sentences + 1, kept);
  W2V_HIP_TRY(hipGetLastError());
  unsigned long long mism = 0;
  W2V_HIP_TRY(hipMemcpyAsync(&mism, mismatch, sizeof(mism), hipMemcpyDeviceToHost, g->stream));
  W2V_HIP_TRY(hipStreamSynchronize(g->stream));
  if (mism > 0)
    return w2v::set_error(W2V_ERR_UNSUPPORTED, "w2v_ingest_map: " + std::to_string(mism) +
                                                   " tokens matched a word by the first hash but not the second "
                                                   "(a collision) or were not counted: the bytes differ from pass 1");
  g->ids = std::move(ids), g->offsets = std::move(offsets);
  g->hist = std::move(hist);
  g->n_ids = kept;
  g->mapped = true;
  return W2V_OK;
}

int w2v_ingest_samples_size(w2v_ingest* g, int64_t* n_ids, int64_t* n_sentences, int64_t* train_words) {
  if (!g) return w2v::set_error(W2V_ERR_ARG, "null ingest");
  if (!g->mapped) return w2v::set_error(W2V_ERR_STATE, "w2v_ingest_map first");
  if (n_ids) *n_ids = g->n_ids;
  if (n_sentences) *n_sentences = g->n_sentences;
  if (train_words) *train_words = g->raw_tokens;
  return W2V_OK;
}

int w2v_ingest_download(w2v_ingest* g, int32_t* ids, int64_t* offsets) {
  if (!g) return w2v::set_error(W2V_ERR_ARG, "null ingest");
  if (!g->mapped) return w2v::set_error(W2V_ERR_STATE, "w2v_ingest_map first");
  W2V_HIP_TRY(hipSetDevice(g->device));
  if (ids && g->n_ids > 0) W2V_HIP_TRY(hipMemcpy(ids, g->ids.get(), g->n_ids * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (offsets) W2V_HIP_TRY(hipMemcpy(offsets, g->offsets.get(), (g->n_sentences + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
  return W2V_OK;
}

}  // extern "C"

namespace w2v {
IngestView ingest_view(const w2v_ingest* g) {
  IngestView v{};
  if (!g || !g->mapped) return v;
  v.device = g->device;
  v.ids = g->ids.get();
  v.n_ids = g->n_ids;
  v.offsets = g->offsets.get();
  v.n_sentences = g->n_sentences;
  v.train_words = g->raw_tokens;
  v.hist = g->hist.data();
  v.n_vocab = (int64_t)g->hist.size();
  v.ok = true;
  return v;
}
}  // namespace w2v
