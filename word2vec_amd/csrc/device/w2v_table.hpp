// w2v_table.hpp — the open-addressing device hash table and the stream
// compaction around it that corpus ingestion (w2v_ingest.hip) and phrase
// detection (w2v_phrase.hip) share. A unit owns its table's columns, its key
// and home slot, its probe limit, its insert and its payload-moving rehash;
// the probe loops, the LDS-aggregated count, the ordering of the used slots
// and the growth step are here, once. Not part of the public boundary.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <vector>

#include "w2v_dev_internal.hpp"

namespace w2v {
namespace table {

using ull = unsigned long long;

constexpr uint64_t kEmpty = 0;           // a key column's free slot
constexpr uint32_t kNone = 0xFFFFFFFFu;  // slot[t] of an element that holds no key (not counted)
constexpr int kBlock = 256;
constexpr int kLdsSlots = 4096;  // per-workgroup count aggregation
constexpr int64_t kMaxCap = (int64_t)1 << 30;

__device__ __forceinline__ uint64_t mix64(uint64_t z) {  // splitmix64 finaliser
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// Claim (CAS) or find `key` from its home slot; -1 after min(kMaxProbe, mask + 1)
// slots: a longer chain counts as a full table (the table grows).
template <int kMaxProbe>
__device__ __forceinline__ int64_t claim(uint64_t* keys, uint64_t mask, uint64_t home, uint64_t key, bool* won) {
  uint64_t i = home;
  *won = false;
  for (uint64_t probe = 0; probe < (uint64_t)kMaxProbe && probe <= mask; ++probe, i = (i + 1) & mask) {
    uint64_t cur = __hip_atomic_load(&keys[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kEmpty) {
      uint64_t expected = kEmpty;
      if (__hip_atomic_compare_exchange_strong(&keys[i], &expected, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT)) {
        *won = true;
        return (int64_t)i;
      }
      cur = expected;
    }
    if (cur == key) return (int64_t)i;
  }
  return -1;
}

// The slot of `key` in a table no kernel is writing; -1 when it is not there.
__device__ __forceinline__ int64_t find(const uint64_t* keys, uint64_t mask, uint64_t home, uint64_t key) {
  uint64_t i = home;
  for (uint64_t probe = 0; probe <= mask; ++probe, i = (i + 1) & mask) {
    const uint64_t cur = keys[i];
    if (cur == kEmpty) break;
    if (cur == key) return (int64_t)i;
  }
  return -1;
}

// count[slot[t]] += 1 for every slot[t] != kNone: per workgroup the adds go to
// an LDS table first (Zipf data: the hot slots' adds stay in LDS, one global
// add per distinct slot per workgroup); a slot that finds no LDS entry within
// 8 probes adds to HBM directly. With kFirst, first[slot[t]] is lowered to t
// as well.
template <bool kFirst>
__global__ __launch_bounds__(kBlock) void count_kernel(const uint32_t* slot, int64_t n, ull* count, ull* first) {
  __shared__ uint32_t lkey[kLdsSlots];
  __shared__ uint32_t lcnt[kLdsSlots];
  for (int h = threadIdx.x; h < kLdsSlots; h += kBlock) {
    lkey[h] = kNone;
    lcnt[h] = 0;
  }
  __syncthreads();
  const int64_t per = (n + gridDim.x - 1) / gridDim.x;
  const int64_t lo = (int64_t)blockIdx.x * per, hi = min(n, lo + per);
  for (int64_t t = lo + threadIdx.x; t < hi; t += kBlock) {
    const uint32_t s = slot[t];
    if (s == kNone) continue;
    if (kFirst)
      if ((ull)t < __hip_atomic_load(&first[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&first[s], (ull)t);
    uint32_t h = (s * 2654435761u) >> 20;  // 12 bits
    bool done = false;
    for (int probe = 0; probe < 8 && !done; ++probe, h = (h + 1) & (kLdsSlots - 1)) {
      uint32_t k = lkey[h];
      if (k == kNone) {
        const uint32_t old = atomicCAS(&lkey[h], kNone, s);
        k = old == kNone ? s : old;  // claimed it, or another thread did
      }
      if (k == s) {
        atomicAdd(&lcnt[h], 1u);
        done = true;
      }
    }
    if (!done) atomicAdd(&count[s], 1ull);
  }
  __syncthreads();
  for (int h = threadIdx.x; h < kLdsSlots; h += kBlock)
    if (lcnt[h]) atomicAdd(&count[lkey[h]], (ull)lcnt[h]);
}

template <class T>
__global__ void gather_kernel(const int64_t* slots, int64_t m, const T* src, T* out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += stride) out[k] = src[slots[k]];
}

struct Used {
  const uint64_t* key;
  __host__ __device__ bool operator()(const int64_t& i) const { return key[i] != kEmpty; }
};
struct NotNegative {
  __host__ __device__ bool operator()(const int32_t& v) const { return v >= 0; }
};

inline dim3 grid_for(int64_t n) {
  return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(8192, (n + kBlock - 1) / kBlock)));
}

inline int64_t pow2_at_least(int64_t v) {
  int64_t c = 1;
  while (c < v) c <<= 1;
  return c;
}

// The slots in [0, cap) that satisfy `pred`, sorted ascending by sort_key[slot]:
// *m_out of them into order (and their keys into sorted_keys). hipcub's element
// counts are int: cap <= kMaxCap.
template <class Pred>
int select_sorted(hipStream_t st, int64_t cap, Pred pred, const ull* sort_key, DevBuf<int64_t>& order,
                  DevBuf<ull>& sorted_keys, int64_t* m_out) {
  DevBuf<int64_t> slots, n_sel;
  DevBuf<ull> keys;
  DevBuf<unsigned char> tmp;
  int rc;
  if ((rc = slots.alloc((size_t)cap)) || (rc = n_sel.alloc(1))) return rc;
  hipcub::CountingInputIterator<int64_t> it(0);
  size_t t1 = 0;
  W2V_HIP_TRY(hipcub::DeviceSelect::If(nullptr, t1, it, slots.get(), n_sel.get(), (int)cap, pred, st));
  if ((rc = tmp.alloc(std::max<size_t>(t1, 1)))) return rc;
  W2V_HIP_TRY(hipcub::DeviceSelect::If(tmp.get(), t1, it, slots.get(), n_sel.get(), (int)cap, pred, st));
  int64_t m = 0;
  W2V_HIP_TRY(hipMemcpyAsync(&m, n_sel.get(), sizeof(int64_t), hipMemcpyDeviceToHost, st));
  W2V_HIP_TRY(hipStreamSynchronize(st));
  *m_out = m;
  const size_t mm = (size_t)std::max<int64_t>(m, 1);
  if ((rc = keys.alloc(mm)) || (rc = sorted_keys.alloc(mm)) || (rc = order.alloc(mm))) return rc;
  if (m == 0) return W2V_OK;
  hipLaunchKernelGGL(gather_kernel<ull>, grid_for(m), dim3(kBlock), 0, st, slots.get(), m, sort_key, keys.get());
  W2V_HIP_TRY(hipGetLastError());
  size_t t2 = 0;
  W2V_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, t2, keys.get(), sorted_keys.get(), slots.get(), order.get(),
                                                 (int)m, 0, 64, st));
  if ((rc = tmp.alloc(std::max<size_t>(t2, 1)))) return rc;
  W2V_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp.get(), t2, keys.get(), sorted_keys.get(), slots.get(), order.get(),
                                                 (int)m, 0, 64, st));
  W2V_HIP_TRY(hipStreamSynchronize(st));
  return W2V_OK;
}

// The growth step of an insert loop: `tab` (a unit's TableBuf: cap(), alloc(cap, stream))
// is replaced by an empty one, doubled until it holds `need` keys at most half
// full, into which `rehash(from, to)` launches the unit's kernel that moves the
// used slots with their payload and counts in *fail the keys that found no slot.
template <class TableBuf, class Rehash>
int grow(hipStream_t st, TableBuf& tab, int64_t need, ull* fail, Rehash rehash, const char* too_many, const char* lost) {
  int64_t cap = tab.cap() * 2;
  while (cap < 2 * need) cap <<= 1;
  if (cap > kMaxCap) return set_error(W2V_ERR_UNSUPPORTED, too_many);
  TableBuf nt;
  if (int rc = nt.alloc(cap, st)) return rc;
  W2V_HIP_TRY(hipMemsetAsync(fail, 0, sizeof(ull), st));
  rehash(tab, nt);
  W2V_HIP_TRY(hipGetLastError());
  ull f = 0;
  W2V_HIP_TRY(hipMemcpyAsync(&f, fail, sizeof(f), hipMemcpyDeviceToHost, st));
  W2V_HIP_TRY(hipStreamSynchronize(st));
  if (f) return set_error(W2V_ERR_STATE, lost);
  tab = std::move(nt);
  return W2V_OK;
}

// ExclusiveSum of flags[0, n) (n > 0) into pos, and the total. `scratch` grows
// when it is too small: a caller in a loop sizes it once, ahead.
inline int exclusive_sum(hipStream_t st, const int32_t* flags, int32_t* pos, int64_t n, int64_t* total,
                         DevBuf<unsigned char>& scratch) {
  size_t tb = 0;
  W2V_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, flags, pos, (int)n, st));
  if (scratch.size() < std::max<size_t>(tb, 1))
    if (int rc = scratch.alloc(std::max<size_t>(tb, 1))) return rc;
  W2V_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(scratch.get(), tb, flags, pos, (int)n, st));
  int32_t last_pos = 0, last_flag = 0;
  W2V_HIP_TRY(hipMemcpyAsync(&last_pos, pos + n - 1, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  W2V_HIP_TRY(hipMemcpyAsync(&last_flag, flags + n - 1, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  W2V_HIP_TRY(hipStreamSynchronize(st));
  *total = (int64_t)last_pos + last_flag;
  return W2V_OK;
}

// The tokens per vocab id of a map call: hist[vocab_index[k]] += count[k] over
// the n_words ids with vocab_index[k] >= 0 (every occurrence of an in-vocab id
// is kept). False when an entry is below -1.
inline bool vocab_hist(const int32_t* vocab_index, const int64_t* count, int64_t n_words, std::vector<int64_t>& hist) {
  int32_t vmax = -1;
  for (int64_t k = 0; k < n_words; ++k) {
    if (vocab_index[k] < -1) return false;
    vmax = std::max(vmax, vocab_index[k]);
  }
  hist.assign((size_t)vmax + 1, 0);
  for (int64_t k = 0; k < n_words; ++k)
    if (vocab_index[k] >= 0) hist[(size_t)vocab_index[k]] += count[(size_t)k];
  return true;
}

}  // namespace table
}  // namespace w2v
