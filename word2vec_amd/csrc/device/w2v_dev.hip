// w2v_dev.hip — implementation of the C-ABI in include/w2v_dev.h: HBM
// residency of the model / vocab products / corpus, and the launches of the
// gfx950 kernels in w2v_kernels.hpp. No exceptions cross the boundary.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "w2v_dev.h"
#include "w2v_dev_internal.hpp"
#include "w2v_kernels.hpp"
#include "w2v_launch.hpp"
#include "w2v_policy.hpp"
#include "w2v_score.hpp"
#include "w2v_shared.hpp"

namespace w2v {

// Expand the monotone unigram table from its V+1 first-index boundaries.
__global__ void expand_table_kernel(const int64_t* bounds, int64_t V, uint32_t* table, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    int64_t lo = 0, hi = V - 1;  // largest w with bounds[w] <= i
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (bounds[mid] <= i) lo = mid;
      else hi = mid - 1;
    }
    table[i] = (uint32_t)lo;
  }
}


}  // namespace w2v

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

}  // namespace

using w2v::Knobs;  // the experiment knobs (w2v_policy.hpp)

static Knobs read_knobs() {
  Knobs k;
  auto get = [&](const char* name) -> const char* {
    const char* v = std::getenv(name);
    if (v && *v) k.desc += (k.desc.empty() ? "" : " ") + std::string(name) + "=" + v;
    return (v && *v) ? v : nullptr;
  };
  if (const char* v = get("W2V_SEG_LEN")) k.seg_len = std::max<int64_t>(0, std::atoll(v));
  if (const char* v = get("W2V_DEBUG_WPB")) k.wpb = std::max(1, std::atoi(v));
  if (const char* v = get("W2V_DEBUG_LDS_PER_WAVE")) k.lds_per_wave = std::max<int64_t>(0, std::atoll(v));
  if (const char* v = get("W2V_DEBUG_MAX_BLOCKS")) k.max_blocks = std::max<int64_t>(0, std::atoll(v));
  if (const char* v = get("W2V_SN_OCC")) k.sn_occ = std::max(0, std::atoi(v));
  if (const char* v = get("W2V_SN_COHERENT_ROWS")) k.sn_coherent_rows = std::max<int64_t>(0, std::atoll(v));
  if (const char* v = get("W2V_SN_ATOMIC_ROWS")) k.sn_atomic_rows = std::max<int64_t>(0, std::atoll(v));
  if (const char* v = get("W2V_SCALE_RESIDENT")) k.scale_resident = std::atoi(v) != 0;
  if (const char* v = get("W2V_PRIV_TAIL_AVG")) k.priv_tail_avg = std::max(0.0, std::atof(v));
  if (const char* v = get("W2V_SN_PER_CU")) k.sn_per_cu = std::max(0, std::atoi(v));
  if (const char* v = get("W2V_CTX_AVG")) k.ctx_avg = std::max(0.0, std::atof(v));
  if (const char* v = get("W2V_PRIV_HS_TAIL_AVG")) k.priv_hs_tail_avg = std::max(0.0, std::atof(v));
  if (const char* v = get("W2V_HS_HOT_AVG")) k.hs_hot_avg = std::max(0.0, std::atof(v));
  if (const char* v = get("W2V_WIDE_HS")) k.wide_hs = std::atoi(v) != 0;
  if (const char* v = get("W2V_DEEP_HS")) k.deep_hs = std::atoi(v) != 0;
  return k;
}

// A resident corpus (token ids + sentence offsets). Handles on one device may
// train on one copy (w2v_dev_share_corpus: replicas of configs[3]'s 40 GB of
// ids); each holds it through a shared_ptr and the last one to let go frees
// it, so an owner that is destroyed or re-uploads its corpus never frees
// buffers a borrower's kernels still read.
struct CorpusBuf {
  w2v::DevBuf<int32_t> ids;
  w2v::DevBuf<int64_t> soff;
};

struct w2v_dev {
  w2v_dev_config cfg{};
  Knobs knobs;
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int64_t V = 0;
  int64_t pitch = 0;
  int32_t d4 = 0;
  int nv = 1;                 // floats per lane per row (instantiated width >= ceil(d / 64))
  w2v::PolicySettings set;   // the update policy's setters (w2v_dev_set_hot_rows ... w2v_dev_set_private_rate)
  bool need_C = false, need_S = false;
  // The model the kernels read, and its memory when the handle allocated it:
  // the buffers stay empty when w2v_dev_bind_model supplied the caller's.
  float* W = nullptr;
  float* C = nullptr;
  float* S = nullptr;
  w2v::DevBuf<float> W_own, C_own, S_own;
  w2v::DevBuf<float> keep;
  w2v::DevBuf<uint32_t> table;
  w2v::DevBuf<uint8_t> codes;
  w2v::DevBuf<int32_t> points;
  w2v::DevBuf<int64_t> coff;
  int64_t n_codes = 0;
  std::shared_ptr<CorpusBuf> corpus;  // shared with the handles training on it
  int64_t n_tok = 0, n_sent = 0, train_words = 0;
  int64_t max_len = 0;        // longest sentence (tokens)
  w2v::DevBuf<int64_t> order;
  int64_t n_order = 0;        // entries of `order` set by w2v_dev_set_order
  w2v::DevBuf<uint32_t> replay;
  w2v::DevBuf<int64_t> replay_off;
  int64_t n_replay_off = 0;
  w2v::DevBuf<unsigned long long> counters;  // [0] words, [1..5] stats
  w2v::DevBuf<unsigned int> work;
  w2v::DevBuf<float> scratch_f;      // x | grad | rows for apply_rows
  w2v::DevBuf<uint8_t> scratch_codes;
  w2v::DevBuf<int32_t> wide_scratch; // CBOW windows past kMaxWideWindow: per-wave id slices (cbow_center_huge)
  w2v::DevBuf<float> xfer_f;         // row-sparse transfers: packed rows | row ids
  float fixed_alpha = 0.0f;
  int32_t rng = W2V_RNG_PHILOX;
  uint64_t seed = 0;
  int32_t sched = W2V_SCHED_PARALLEL;
  int32_t update = W2V_UPDATE_PER_PAIR;
  int n_cu = 256;
  bool model_ready = false, vocab_ready = false, corpus_ready = false;
  // Host copies of the vocab and corpus uploads, for the update policy's
  // frequency-derived settings (stats_of: flush scales, automatic hot rows):
  std::vector<float> keep_h;        // sample probabilities
  std::vector<int32_t> leaf_node;   // HS: per word, the deepest internal node of its path (-1: none)
  std::vector<int32_t> node_parent; // HS: parent of each internal node, -1 for the root
  std::vector<int64_t> tok_count;   // corpus token count per word
  uint64_t data_version = 0;        // bumped by every upload that changes the statistics
  uint64_t stats_version = ~0ull;   // the data_version `stats` was derived from
  w2v::RowStats stats;              // derived (stats_of); its table_frac is set by the table's upload
  int32_t replicas = 1;             // replicas of the exchange group this handle joined (w2v::set_replicas)
  w2v::LaunchPlan last_plan;        // what the last launch's policy decided (w2v_dev_launch_plan)
  // the device copy of last_plan.hot_sc and the scales it holds
  std::vector<float> hot_sc_h;
  w2v::DevBuf<float> hot_sc_d;
  // w2v_dev_score: the scored arrays, their work items and the partials (reused across calls)
  int32_t score_item = 0;  // centers per work item (0: automatic)
  w2v::DevBuf<int32_t> score_ids;
  w2v::DevBuf<int64_t> score_soff, score_item_off, score_part_targets, score_targets;
  w2v::DevBuf<double> score_part_ll, score_ll;
  w2v::DevBuf<uint32_t> score_part_nonfinite;
  w2v::DevBuf<unsigned long long> score_ctr;

  ~w2v_dev() {  // the buffers free themselves after this
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    if (own_stream && stream) (void)hipStreamDestroy(stream);
  }
  // Let go of the handle's own model memory (W / C / S then view nothing).
  void drop_model() {
    W_own.reset(), C_own.reset(), S_own.reset();
    W = C = S = nullptr;
  }
};

namespace w2v {
int set_error(int code, const std::string& msg) { return fail(code, msg); }
DevInfo dev_info(const w2v_dev* h) { return DevInfo{h->device, h->stream, h->V, h->cfg.word_dim}; }
void set_replicas(w2v_dev* h, int32_t n) { h->replicas = n < 1 ? 1 : n; }
}  // namespace w2v

// Per-word and per-node shares of the corpus (cached until the next upload).
static const w2v::RowStats& stats_of(w2v_dev* h) {
  if (h->stats_version != h->data_version) {
    h->stats_version = h->data_version;
    w2v::row_stats(h->stats, h->V, h->tok_count, h->keep_h, h->leaf_node, h->node_parent);
  }
  return h->stats;
}

namespace w2v {
// Per kept center (Word2Vec.cpp:319-353 SG, :273-317 CBOW): skip-gram updates
// the center's W row once, the C row of every context (win1 = window + 1 on
// average over the shrunk windows) and of neg table draws per context, and
// the Huffman nodes of every context's path; CBOW the C rows of the contexts,
// the W row of the center and of neg draws, and the center's path. Times the
// kept fraction of the tokens.
bool row_update_rates(w2v_dev* h, int k, std::vector<double>& out) {
  const w2v::RowStats& st = stats_of(h);
  const int64_t V = h->V;
  out.clear();
  if (!st.stats_ok || h->tok_count.empty()) return false;
  double N = 0.0;
  for (int64_t c : h->tok_count) N += (double)c;
  const double q = N > 0.0 ? st.kept_tokens / N : 0.0;
  const double win1 = (double)h->cfg.window + 1.0, neg = (double)h->cfg.negative;
  const bool cbow = h->cfg.cbow != 0;
  if (k == 2) {
    if (!st.has_nodes(V)) return false;
    out.resize((size_t)(V - 1));
    for (int64_t j = 0; j < V - 1; ++j) out[(size_t)j] = q * st.node_rate(j, cbow, win1);
    return true;
  }
  out.resize((size_t)V);
  for (int64_t r = 0; r < V; ++r) {
    const double f = st.f[(size_t)r], fk = st.fk[(size_t)r];
    double m;
    if (k == 0) m = cbow ? (neg > 0 ? fk + neg * st.u(r) : 0.0) : fk;
    else m = cbow ? win1 * f : win1 * (f + neg * st.u(r));
    out[(size_t)r] = q * m;
  }
  return true;
}
}  // namespace w2v

namespace {

using KernelFn = w2v::KernelFn;

// Instantiated row widths (floats per lane): the smallest one covering d
// (w2v_rows.hpp kFullVecs relies on it: the vectors below the next smaller
// width are inside d in every lane).
const w2v::NvKernels& kernels_for_need(int need) {
  for (const w2v::NvKernels& k : w2v::kNvKernels)
    if (k.nv >= need) return k;
  return *(std::end(w2v::kNvKernels) - 1);
}
int pick_nv(int d) { return kernels_for_need((d + w2v::kWave - 1) / w2v::kWave).nv; }

KernelFn kernel_for(const w2v_dev* h) {
  const bool wd = 2 * h->cfg.window + 1 > w2v::kWave;  // CBOW's lane-per-position context set no longer fits
  return kernels_for_need(h->nv).pick_train(h->cfg.cbow != 0, h->cfg.hs != 0, h->cfg.negative > 0,
                                            h->rng == W2V_RNG_REPLAY, wd);
}
KernelFn kernel_deep_for(const w2v_dev* h) { return kernels_for_need(h->nv).pick_train_deep(h->cfg.cbow != 0); }
w2v::ApplyFn apply_for(const w2v_dev* h) { return kernels_for_need(h->nv).pick_apply(); }

int set_device(w2v_dev* h) {
  W2V_HIP_TRY(hipSetDevice(h->device));
  return W2V_OK;
}

// Make `c` the handle's corpus (the three entrances: upload, adopt, share).
// The handle lets go of its old one here, after the last step that can fail;
// the last handle to let go of a corpus frees it.
int install_corpus(w2v_dev* h, std::shared_ptr<CorpusBuf> c, int64_t n_tok, int64_t n_sent, int64_t max_len,
                   int64_t train_words, std::vector<int64_t> hist) {
  w2v::DevBuf<int64_t> order;
  if (int rc = order.alloc((size_t)(n_sent > 0 ? n_sent : 1))) return rc;
  h->corpus = std::move(c);
  h->order = std::move(order);
  h->n_tok = n_tok;
  h->n_sent = n_sent;
  h->n_order = 0;
  h->max_len = max_len;
  h->train_words = train_words;
  h->tok_count = std::move(hist);  // also the flush-scale statistics (priv_scales)
  ++h->data_version;
  h->corpus_ready = true;
  return W2V_OK;
}

// h->stream, the counters and the device's size, for w2v_dev_create.
int init_device(w2v_dev* h) {
  W2V_HIP_TRY(hipSetDevice(h->device));
  W2V_HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  h->own_stream = true;
  if (int rc = h->counters.alloc(8)) return rc;
  W2V_HIP_TRY(hipMemset(h->counters.get(), 0, 8 * sizeof(unsigned long long)));
  if (int rc = h->work.alloc(1)) return rc;
  int ncu = 0;
  W2V_HIP_TRY(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, h->device));
  h->n_cu = ncu > 0 ? ncu : 256;
  return W2V_OK;
}

}  // namespace

extern "C" {

const char* w2v_dev_version(void) { return "word2vec_amd-dev 0.1 (gfx950)"; }
const char* w2v_dev_last_error(void) { return g_err.c_str(); }

const char* w2v_dev_knobs(w2v_dev* h) { return h ? h->knobs.desc.c_str() : ""; }

// The per-pair kernels' range (the reference takes any, Word2Vec.cpp:254, 285,
// 335): a row is <= 32 floats per lane; a context's negatives are drawn and
// deduplicated 64 at a time (ns_word_many: every chunk is compared with every
// earlier one) with the draw index in the Philox counter (philox_table_pos:
// k < 2^20); a CBOW window past 127 is walked from the sentence
// (cbow_center_huge: each position against the earlier ones) with a per-wave
// scratch of huge_stride ints. Both walks are quadratic, so window and
// negative stop at 4096, where their cost was measured (include/w2v_dev.h;
// at 65535 a center would take ~2^28 steps).
constexpr int32_t kMaxDim = 2048, kMaxNegative = 4096, kMaxWindowHost = 4096;
constexpr int32_t kSnMaxDim = 1024, kSnMaxWindow = 8, kSnMaxNegative = 15;

int w2v_dev_limits(int32_t* max_dim, int32_t* max_window, int32_t* max_negative, int32_t* shared_max_window,
                   int32_t* shared_max_negative) {
  if (max_dim) *max_dim = kMaxDim;
  if (max_window) *max_window = kMaxWindowHost;
  if (max_negative) *max_negative = kMaxNegative;
  if (shared_max_window) *shared_max_window = kSnMaxWindow;
  if (shared_max_negative) *shared_max_negative = kSnMaxNegative;
  return W2V_OK;
}

int w2v_dev_shared_limits(int32_t* max_dim, int32_t* max_window, int32_t* max_negative) {
  if (max_dim) *max_dim = kSnMaxDim;
  if (max_window) *max_window = kSnMaxWindow;
  if (max_negative) *max_negative = kSnMaxNegative;
  return W2V_OK;
}

int w2v_dev_create(const w2v_dev_config* cfg, w2v_dev** out) {
  if (!cfg || !out) return fail(W2V_ERR_ARG, "w2v_dev_create: null argument");
  *out = nullptr;
  if (cfg->word_dim <= 0) return fail(W2V_ERR_ARG, "word_dim must be > 0");
  if (cfg->word_dim > kMaxDim) return fail(W2V_ERR_UNSUPPORTED, "word_dim > " + std::to_string(kMaxDim) + " unsupported");
  if (cfg->window < 0 || cfg->window > kMaxWindowHost)
    return fail(W2V_ERR_UNSUPPORTED, "window must be in [0, " + std::to_string(kMaxWindowHost) + "]");
  if (cfg->negative < 0 || cfg->negative > kMaxNegative)
    return fail(W2V_ERR_UNSUPPORTED, "negative must be in [0, " + std::to_string(kMaxNegative) + "]");
  if (!cfg->hs && cfg->negative == 0)
    return fail(W2V_ERR_ARG, "neither hs nor negative sampling enabled");
  if (cfg->negative > 0 && cfg->table_size <= 0) return fail(W2V_ERR_ARG, "table_size must be > 0");
  if (cfg->iter <= 0) return fail(W2V_ERR_ARG, "iter must be > 0");
  w2v_dev* h = new w2v_dev();
  h->cfg = *cfg;
  h->knobs = read_knobs();
  h->last_plan.private_rate = h->last_plan.tau_rows = h->last_plan.hs_hot_avg = 0.0;  // no launch yet
  if (cfg->device >= 0) {
    h->device = cfg->device;
  } else {
    hipError_t e = hipGetDevice(&h->device);
    if (e != hipSuccess) {
      delete h;
      return fail(W2V_ERR_HIP, std::string("hipGetDevice: ") + hipGetErrorString(e));
    }
  }
  if (int rc = init_device(h)) {
    delete h;
    return rc;
  }
  h->d4 = (cfg->word_dim + 3) & ~3;
  h->nv = pick_nv(cfg->word_dim);
  h->pitch = (int64_t)h->nv * w2v::kWave;  // the kernels' row width (w2v_rows.hpp)
  h->need_C = cfg->negative > 0 || cfg->cbow;
  h->need_S = cfg->hs != 0;
  *out = h;
  return W2V_OK;
}

void w2v_dev_destroy(w2v_dev* h) { delete h; }

int w2v_dev_set_stream(w2v_dev* h, void* s) {
  if (!h) return fail(W2V_ERR_ARG, "null handle");
  if (set_device(h)) return W2V_ERR_HIP;
  W2V_HIP_TRY(hipStreamSynchronize(h->stream));
  hipStream_t next = (hipStream_t)s;
  if (!s) W2V_HIP_TRY(hipStreamCreateWithFlags(&next, hipStreamNonBlocking));
  const hipStream_t old = h->own_stream ? h->stream : nullptr;
  h->stream = next;  // the handle holds a live stream whatever the old one's destroy says
  h->own_stream = !s;
  if (old) W2V_HIP_TRY(hipStreamDestroy(old));
  return W2V_OK;
}

int w2v_dev_set_rng(w2v_dev* h, int32_t mode, uint64_t seed) {
  if (!h) return fail(W2V_ERR_ARG, "null handle");
  if (mode != W2V_RNG_PHILOX && mode != W2V_RNG_REPLAY) return fail(W2V_ERR_ARG, "bad rng mode");
  h->rng = mode;
  h->seed = seed;
  return W2V_OK;
}

int w2v_dev_set_schedule(w2v_dev* h, int32_t s) {
  if (!h) return fail(W2V_ERR_ARG, "null handle");
  if (s != W2V_SCHED_PARALLEL && s != W2V_SCHED_SEQUENTIAL) return fail(W2V_ERR_ARG, "bad schedule");
  h->sched = s;
  return W2V_OK;
}

int w2v_dev_upload_vocab(w2v_dev* h, int64_t V, const float* keep, const int64_t* bounds,
                         const uint8_t* codes, const int32_t* points, const int64_t* coff) {
  w2v::Range range_("w2v_dev_upload_vocab");
  if (!h || !keep) return fail(W2V_ERR_ARG, "w2v_dev_upload_vocab: null argument");
  if (V < 1 || V > (int64_t)INT32_MAX) return fail(W2V_ERR_ARG, "vocab_size out of range");
  if (h->cfg.hs && V < 2) return fail(W2V_ERR_ARG, "hs needs vocab_size >= 2");
  if (h->cfg.negative > 0 && !bounds && !h->table.get())
    return fail(W2V_ERR_ARG, "negative sampling needs table_bounds (or w2v_dev_upload_table first)");
  if (h->cfg.hs && (!codes || !points || !coff)) return fail(W2V_ERR_ARG, "hs needs codes/points/code_offsets");
  // validate everything before touching the handle, so a rejected call leaves it as it was
  const int64_t n = h->cfg.table_size;
  if (h->cfg.negative > 0 && bounds) {
    if (bounds[0] != 0 || bounds[V] != n) return fail(W2V_ERR_ARG, "table_bounds must start at 0 and end at table_size");
    for (int64_t w = 0; w < V; ++w)
      if (bounds[w] > bounds[w + 1]) return fail(W2V_ERR_ARG, "table_bounds must be non-decreasing");
  }
  if (h->cfg.hs) {
    if (coff[0] != 0) return fail(W2V_ERR_ARG, "code_offsets[0] must be 0");
    for (int64_t w = 0; w < V; ++w)
      if (coff[w] > coff[w + 1] || coff[w + 1] - coff[w] > 4096)
        return fail(W2V_ERR_ARG, "code_offsets must be non-decreasing with paths <= 4096");
    for (int64_t t = 0; t < coff[V]; ++t)
      if (points[t] < 0 || points[t] > V - 2 || codes[t] > 1)
        return fail(W2V_ERR_ARG, "Huffman point/code out of range");
  }
  if (set_device(h)) return W2V_ERR_HIP;
  // device buffers first (a HIP failure leaves the handle's old vocab in place)
  w2v::DevBuf<float> dkeep;
  w2v::DevBuf<uint32_t> dtable;
  w2v::DevBuf<uint8_t> dcodes;
  w2v::DevBuf<int32_t> dpoints;
  w2v::DevBuf<int64_t> dcoff;
  int rc = dkeep.alloc((size_t)V);
  if (rc) return rc;
  W2V_HIP_TRY(hipMemcpy(dkeep.get(), keep, V * sizeof(float), hipMemcpyHostToDevice));
  if (h->cfg.negative > 0 && bounds) {
    w2v::DevBuf<int64_t> db;
    if ((rc = dtable.alloc((size_t)n)) || (rc = db.alloc((size_t)V + 1))) return rc;
    W2V_HIP_TRY(hipMemcpy(db.get(), bounds, (V + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(w2v::expand_table_kernel, dim3(4096), dim3(256), 0, h->stream, db.get(), V, dtable.get(), n);
    W2V_HIP_TRY(hipGetLastError());
    W2V_HIP_TRY(hipStreamSynchronize(h->stream));
  }
  const int64_t nc = h->cfg.hs ? coff[V] : 0;
  if (h->cfg.hs) {
    const size_t n1 = (size_t)(nc > 0 ? nc : 1);
    if ((rc = dcodes.alloc(n1)) || (rc = dpoints.alloc(n1)) || (rc = dcoff.alloc((size_t)V + 1))) return rc;
    if (nc > 0) W2V_HIP_TRY(hipMemcpy(dcodes.get(), codes, nc, hipMemcpyHostToDevice));
    if (nc > 0) W2V_HIP_TRY(hipMemcpy(dpoints.get(), points, nc * sizeof(int32_t), hipMemcpyHostToDevice));
    W2V_HIP_TRY(hipMemcpy(dcoff.get(), coff, (V + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  }
  if (h->V != V) {
    h->drop_model();
    h->pitch = (int64_t)h->nv * w2v::kWave;
    h->model_ready = false;
    h->tok_count.clear();  // the corpus statistics refer to the old ids
  }
  h->V = V;
  ++h->data_version;
  h->keep = std::move(dkeep);
  h->keep_h.assign(keep, keep + V);
  if (dtable.get()) {
    h->table = std::move(dtable);
    h->stats.table_frac.assign((size_t)V, 0.0);
    for (size_t r = 0; r < h->stats.table_frac.size(); ++r) h->stats.table_frac[r] = (double)(bounds[r + 1] - bounds[r]) / (double)n;
  }
  if (h->cfg.hs) {
    h->codes = std::move(dcodes), h->points = std::move(dpoints), h->coff = std::move(dcoff);
    h->n_codes = nc;
    // the tree's shape, for the per-node statistics: paths run root -> leaf
    h->leaf_node.assign((size_t)V, -1);
    h->node_parent.assign((size_t)(V - 1), -1);
    for (int64_t w = 0; w < V; ++w) {
      int32_t prev = -1;
      for (int64_t t = coff[w]; t < coff[w + 1]; ++t) {
        h->node_parent[(size_t)points[t]] = prev;
        prev = points[t];
      }
      h->leaf_node[(size_t)w] = prev;
    }
  }
  h->vocab_ready = true;
  return W2V_OK;
}

int w2v_dev_upload_table(w2v_dev* h, const uint32_t* table, int64_t n) {
  if (!h || !table) return fail(W2V_ERR_ARG, "w2v_dev_upload_table: null argument");
  if (n != h->cfg.table_size) return fail(W2V_ERR_ARG, "table length != table_size");
  if (set_device(h)) return W2V_ERR_HIP;
  w2v::DevBuf<uint32_t> t;
  if (int rc = t.alloc((size_t)n)) return rc;
  W2V_HIP_TRY(hipMemcpy(t.get(), table, n * sizeof(uint32_t), hipMemcpyHostToDevice));
  h->table = std::move(t);
  h->stats.table_frac.assign((size_t)std::max<int64_t>(h->V, 0), 0.0);
  for (int64_t i = 0; i < n; ++i)
    if ((int64_t)table[i] < h->V) h->stats.table_frac[table[i]] += 1.0 / (double)n;
  ++h->data_version;
  return W2V_OK;
}

// A zeroed matrix of n floats owned by the handle, unless it views one already.
static int ensure_matrix(w2v::DevBuf<float>& own, float*& view, size_t n) {
  if (view) return W2V_OK;
  w2v::DevBuf<float> m;
  if (int rc = m.alloc(n)) return rc;
  W2V_HIP_TRY(hipMemset(m.get(), 0, n * sizeof(float)));
  own = std::move(m);
  view = own.get();
  return W2V_OK;
}

static int ensure_model(w2v_dev* h) {
  if (h->V < 1) return fail(W2V_ERR_STATE, "upload the vocab before the model");
  const size_t rows = (size_t)h->V * h->pitch;
  int rc = ensure_matrix(h->W_own, h->W, rows);
  if (!rc && h->need_C) rc = ensure_matrix(h->C_own, h->C, rows);
  if (!rc && h->need_S) rc = ensure_matrix(h->S_own, h->S, (size_t)(h->V > 1 ? h->V - 1 : 1) * h->pitch);
  return rc;
}

int w2v_dev_upload_model(w2v_dev* h, const float* W, const float* C, const float* S) {
  w2v::Range range_("w2v_dev_upload_model");
  if (!h) return fail(W2V_ERR_ARG, "null handle");
  if (set_device(h)) return W2V_ERR_HIP;
  int rc = ensure_model(h);
  if (rc) return rc;
  const size_t d = (size_t)h->cfg.word_dim, dp = (size_t)h->pitch * sizeof(float);
  if (W) W2V_HIP_TRY(hipMemcpy2D(h->W, dp, W, d * sizeof(float), d * sizeof(float), h->V, hipMemcpyHostToDevice));
  if (C) {
    if (!h->C) return fail(W2V_ERR_ARG, "C is not used by this configuration");
    W2V_HIP_TRY(hipMemcpy2D(h->C, dp, C, d * sizeof(float), d * sizeof(float), h->V, hipMemcpyHostToDevice));
  }
  if (S) {
    if (!h->S) return fail(W2V_ERR_ARG, "synapses1 is not used by this configuration");
    if (h->V > 1)
      W2V_HIP_TRY(hipMemcpy2D(h->S, dp, S, d * sizeof(float), d * sizeof(float), h->V - 1, hipMemcpyHostToDevice));
  }
  h->model_ready = true;
  return W2V_OK;
}

int w2v_dev_download_model(w2v_dev* h, float* W, float* C, float* S) {
  w2v::Range range_("w2v_dev_download_model");
  if (!h) return fail(W2V_ERR_ARG, "null handle");
  if (!h->W) return fail(W2V_ERR_STATE, "no model on the device");
  if (set_device(h)) return W2V_ERR_HIP;
  W2V_HIP_TRY(hipStreamSynchronize(h->stream));
  const size_t d = (size_t)h->cfg.word_dim, dp = (size_t)h->pitch * sizeof(float);
  if (W) W2V_HIP_TRY(hipMemcpy2D(W, d * sizeof(float), h->W, dp, d * sizeof(float), h->V, hipMemcpyDeviceToHost));
  if (C && h->C) W2V_HIP_TRY(hipMemcpy2D(C, d * sizeof(float), h->C, dp, d * sizeof(float), h->V, hipMemcpyDeviceToHost));
  if (S && h->S && h->V > 1)
    W2V_HIP_TRY(hipMemcpy2D(S, d * sizeof(float), h->S, dp, d * sizeof(float), h->V - 1, hipMemcpyDeviceToHost));
  return W2V_OK;
}

namespace w2v {
// max |A - B| and max |A| over the first d columns of two pitch-padded
// matrices (non-negative floats compare as their bits: one 32-bit atomicMax
// per block each).
__global__ void max_diff_kernel(const float* A, const float* B, int64_t rows, int64_t pitch, int d,
                                unsigned int* out) {
  __shared__ unsigned int part[2][4];
  float dm = 0.f, am = 0.f;
  const int64_t n = rows * (int64_t)d;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = k / d, c = k - r * d;
    const float a = A[r * pitch + c], b = B[r * pitch + c];
    dm = fmaxf(dm, fabsf(a - b));
    am = fmaxf(am, fabsf(a));
    if (!(a == a) || !(b == b)) dm = __int_as_float(0x7F800000);  // NaN counts as infinitely different
  }
  for (int o = 32; o > 0; o >>= 1) {
    dm = fmaxf(dm, __shfl_xor(dm, o));
    am = fmaxf(am, __shfl_xor(am, o));
  }
  if ((threadIdx.x & 63) == 0) {
    part[0][threadIdx.x >> 6] = __float_as_uint(dm);
    part[1][threadIdx.x >> 6] = __float_as_uint(am);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned int x = 0, y = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) {
      x = max(x, part[0][w]);
      y = max(y, part[1][w]);
    }
    atomicMax(out, x);
    atomicMax(out + 1, y);
  }
}
// rows[k] of M (pitch-padded) <-> packed[k] (dim floats), one wave per row.
__global__ void scatter_rows_kernel(float* M, int64_t pitch, int d, const int32_t* rows, int64_t n, const float* packed) {
  const int64_t k = blockIdx.x;
  if (k >= n) return;
  float* dst = M + (int64_t)rows[k] * pitch;
  const float* src = packed + k * d;
  for (int e = threadIdx.x; e < d; e += blockDim.x) dst[e] = src[e];
}
__global__ void gather_rows_kernel(const float* M, int64_t pitch, int d, const int32_t* rows, int64_t n, float* packed) {
  const int64_t k = blockIdx.x;
  if (k >= n) return;
  const float* src = M + (int64_t)rows[k] * pitch;
  float* dst = packed + k * d;
  for (int e = threadIdx.x; e < d; e += blockDim.x) dst[e] = src[e];
}
}  // namespace w2v

int w2v_dev_model_max_diff(w2v_dev* a, w2v_dev* b, float* out) {
  if (!a || !b || !out) return fail(W2V_ERR_ARG, "null argument");
  if (!a->W || !b->W) return fail(W2V_ERR_STATE, "no model on the device");
  if (a->V != b->V || a->pitch != b->pitch || a->cfg.word_dim != b->cfg.word_dim || !a->C != !b->C ||
      !a->S != !b->S)
    return fail(W2V_ERR_ARG, "the two handles hold models of different shapes");
  if (set_device(b)) return W2V_ERR_HIP;
  W2V_HIP_TRY(hipStreamSynchronize(b->stream));
  if (set_device(a)) return W2V_ERR_HIP;
  W2V_HIP_TRY(hipStreamSynchronize(a->stream));
  const float* MA[3] = {a->W, a->C, a->S};
  const float* MB[3] = {b->W, b->C, b->S};
  const int64_t rows[3] = {a->V, a->V, a->V - 1};
  w2v::DevBuf<unsigned int> acc;
  w2v::DevBuf<float> stage;  // b's matrix on a's device when they differ
  if (int rc = acc.alloc(6)) return rc;
  W2V_HIP_TRY(hipMemset(acc.get(), 0, 6 * sizeof(unsigned int)));
  for (int k = 0; k < 3; ++k) {
    if (!MA[k] || rows[k] <= 0) continue;
    const size_t bytes = (size_t)rows[k] * (size_t)a->pitch * sizeof(float);
    const float* B = MB[k];
    if (a->device != b->device) {
      if (!stage.get())
        if (int rc = stage.alloc((size_t)a->V * (size_t)a->pitch)) return rc;
      W2V_HIP_TRY(hipMemcpyPeer(stage.get(), a->device, B, b->device, bytes));
      B = stage.get();
    }
    hipLaunchKernelGGL(w2v::max_diff_kernel, dim3(2048), dim3(256), 0, a->stream, MA[k], B, rows[k], a->pitch,
                       a->cfg.word_dim, acc.get() + 2 * k);
    W2V_HIP_TRY(hipGetLastError());
    W2V_HIP_TRY(hipStreamSynchronize(a->stream));
  }
  unsigned int host[6] = {0, 0, 0, 0, 0, 0};
  W2V_HIP_TRY(hipMemcpy(host, acc.get(), sizeof(host), hipMemcpyDeviceToHost));
  for (int k = 0; k < 3; ++k) {  // acc holds (max |A - B|, max |A|) per matrix
    std::memcpy(&out[k], &host[2 * k], sizeof(float));
    std::memcpy(&out[3 + k], &host[2 * k + 1], sizeof(float));
  }
  return W2V_OK;
}

// Row-sparse transfer between host rows and one resident matrix: the per-call
// methods (train_sentence_*) move only the rows a sentence's update can touch.
static int transfer_rows(w2v_dev* h, int32_t which, const int32_t* rows, int64_t n, float* data, bool up) {
  if (!h || (n > 0 && (!rows || !data))) return fail(W2V_ERR_ARG, "row transfer: null argument");
  if (n < 0 || n > (int64_t)INT32_MAX) return fail(W2V_ERR_ARG, "row transfer: bad row count");
  if (which < 0 || which > 2) return fail(W2V_ERR_ARG, "row transfer: which must be 0 (W), 1 (C) or 2 (synapses1)");
  if (set_device(h)) return W2V_ERR_HIP;
  if (int rc = ensure_model(h)) return rc;
  float* M = which == 0 ? h->W : which == 1 ? h->C : h->S;
  const int64_t nrows = which == 2 ? h->V - 1 : h->V;
  if (!M) return fail(W2V_ERR_ARG, "row transfer: this configuration has no such matrix");
  for (int64_t k = 0; k < n; ++k)
    if (rows[k] < 0 || rows[k] >= nrows) return fail(W2V_ERR_ARG, "row transfer: row index out of range");
  if (n == 0) return W2V_OK;
  const int d = h->cfg.word_dim;
  const int64_t need = n * d + n + 1;  // packed rows, then the row ids (int32 in float slots)
  if ((int64_t)h->xfer_f.size() < need)
    if (int rc = h->xfer_f.alloc((size_t)need)) return rc;
  float* packed = h->xfer_f.get();
  int32_t* drows = reinterpret_cast<int32_t*>(packed + n * d);
  W2V_HIP_TRY(hipMemcpyAsync(drows, rows, n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  if (up) {
    W2V_HIP_TRY(hipMemcpyAsync(packed, data, (size_t)n * d * sizeof(float), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(w2v::scatter_rows_kernel, dim3((unsigned)n), dim3(256), 0, h->stream, M, h->pitch, d, drows, n,
                       packed);
    W2V_HIP_TRY(hipGetLastError());
  } else {
    hipLaunchKernelGGL(w2v::gather_rows_kernel, dim3((unsigned)n), dim3(256), 0, h->stream, M, h->pitch, d, drows, n,
                       packed);
    W2V_HIP_TRY(hipGetLastError());
    W2V_HIP_TRY(hipMemcpyAsync(data, packed, (size_t)n * d * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  }
  W2V_HIP_TRY(hipStreamSynchronize(h->stream));
  h->model_ready = true;
  return W2V_OK;
}

int w2v_dev_upload_rows(w2v_dev* h, int32_t which, const int32_t* rows, int64_t n, const float* data) {
  return transfer_rows(h, which, rows, n, const_cast<float*>(data), true);
}

int w2v_dev_download_rows(w2v_dev* h, int32_t which, const int32_t* rows, int64_t n, float* data) {
  return transfer_rows(h, which, rows, n, data, false);
}

int w2v_dev_bind_model(w2v_dev* h, float* dW, float* dC, float* dS, int64_t pitch) {
  if (!h || !dW) return fail(W2V_ERR_ARG, "w2v_dev_bind_model: null argument");
  if (h->V < 1) return fail(W2V_ERR_STATE, "upload the vocab before binding the model");
  if (pitch < (int64_t)h->nv * w2v::kWave || pitch % 4 != 0)
    return fail(W2V_ERR_ARG, std::string("pitch must be a multiple of 4 and >= w2v_dev_row_pitch (the kernels' row "
                                         "width, ") + std::to_string((int64_t)h->nv * w2v::kWave) + " floats here)");
  if (h->need_C && !dC) return fail(W2V_ERR_ARG, "this configuration needs C");
  if (h->need_S && !dS) return fail(W2V_ERR_ARG, "this configuration needs synapses1");
  for (const float* p : {dW, dC, dS})
    if (p && (reinterpret_cast<uintptr_t>(p) & 15u)) return fail(W2V_ERR_ARG, "matrix base must be 16-B aligned");
  h->drop_model();
  h->W = dW;
  h->C = h->need_C ? dC : nullptr;
  h->S = h->need_S ? dS : nullptr;
  h->pitch = pitch;
  h->model_ready = true;
  return W2V_OK;
}

int w2v_dev_row_pitch(w2v_dev* h, int64_t* pitch) {
  if (!h || !pitch) return fail(W2V_ERR_ARG, "null argument");
  *pitch = (int64_t)h->nv * w2v::kWave;
  return W2V_OK;
}

int w2v_dev_model_layout(w2v_dev* h, float** dW, float** dC, float** dS, int64_t* pitch) {
  if (!h) return fail(W2V_ERR_ARG, "null handle");
  if (set_device(h)) return W2V_ERR_HIP;
  int rc = ensure_model(h);
  if (rc) return rc;
  if (dW) *dW = h->W;
  if (dC) *dC = h->C;
  if (dS) *dS = h->S;
  if (pitch) *pitch = h->pitch;
  return W2V_OK;
}

int w2v_dev_upload_corpus(w2v_dev* h, const int32_t* ids, int64_t n_tok, const int64_t* soff,
                          int64_t n_sent, int64_t train_words) {
  w2v::Range range_("w2v_dev_upload_corpus");
  if (!h || !soff || (n_tok > 0 && !ids)) return fail(W2V_ERR_ARG, "w2v_dev_upload_corpus: null argument");
  if (n_sent < 0 || n_tok < 0 || n_sent > (int64_t)UINT32_MAX - 1)
    return fail(W2V_ERR_ARG, "corpus sizes out of range");
  if (soff[0] != 0 || soff[n_sent] != n_tok) return fail(W2V_ERR_ARG, "sentence offsets must span [0, n_tokens]");
  int64_t max_len = 0;
  for (int64_t s = 0; s < n_sent; ++s) {
    if (soff[s] > soff[s + 1] || soff[s + 1] - soff[s] > (int64_t)INT32_MAX)
      return fail(W2V_ERR_ARG, "sentence offsets must be non-decreasing");
    max_len = std::max<int64_t>(max_len, soff[s + 1] - soff[s]);
  }
  if (h->V < 1) return fail(W2V_ERR_STATE, "upload the vocab before the corpus");
  std::vector<int64_t> hist((size_t)h->V, 0);
  for (int64_t t = 0; t < n_tok; ++t) {
    if (ids[t] < 0 || ids[t] >= h->V) return fail(W2V_ERR_ARG, "token id out of vocab range");
    ++hist[(size_t)ids[t]];
  }
  if (train_words <= 0 && n_tok > 0) return fail(W2V_ERR_ARG, "train_words must be > 0");
  if (set_device(h)) return W2V_ERR_HIP;
  auto c = std::make_shared<CorpusBuf>();
  int rc;
  if ((rc = c->ids.alloc((size_t)(n_tok > 0 ? n_tok : 1))) || (rc = c->soff.alloc((size_t)n_sent + 1))) return rc;
  if (n_tok > 0) W2V_HIP_TRY(hipMemcpy(c->ids.get(), ids, n_tok * sizeof(int32_t), hipMemcpyHostToDevice));
  W2V_HIP_TRY(hipMemcpy(c->soff.get(), soff, (n_sent + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  return install_corpus(h, std::move(c), n_tok, n_sent, max_len, train_words, std::move(hist));
}

// Device samples (a mapped ingest's or a mapped phrase handle's) into the handle.
static int adopt_view(w2v_dev* h, const w2v::IngestView& v, const char* what, const char* source) {
  if (!v.ok) return fail(W2V_ERR_STATE, std::string(what) + ": map the " + source + " first");
  if (v.device != h->device) return fail(W2V_ERR_ARG, std::string(what) + ": " + source + " on another device");
  if (h->V < 1) return fail(W2V_ERR_STATE, "upload the vocab before the corpus");
  if (v.n_vocab > h->V) return fail(W2V_ERR_ARG, "ingest vocab index beyond the handle's vocab");
  if (v.n_sentences > (int64_t)UINT32_MAX - 1) return fail(W2V_ERR_ARG, "corpus sizes out of range");
  if (v.train_words <= 0 && v.n_ids > 0) return fail(W2V_ERR_ARG, "train_words must be > 0");
  if (set_device(h)) return W2V_ERR_HIP;
  std::vector<int64_t> soff((size_t)v.n_sentences + 1);
  W2V_HIP_TRY(hipMemcpy(soff.data(), v.offsets, soff.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (soff[0] != 0 || soff.back() != v.n_ids) return fail(W2V_ERR_STATE, "ingest offsets do not span its ids");
  int64_t max_len = 0;
  for (int64_t s = 0; s < v.n_sentences; ++s) {
    if (soff[s + 1] - soff[s] > (int64_t)INT32_MAX) return fail(W2V_ERR_UNSUPPORTED, "a sentence over 2^31 tokens");
    max_len = std::max<int64_t>(max_len, soff[s + 1] - soff[s]);
  }
  std::vector<int64_t> hist((size_t)h->V, 0);
  for (int64_t w = 0; w < v.n_vocab; ++w) hist[(size_t)w] = v.hist[w];
  auto c = std::make_shared<CorpusBuf>();
  int rc;
  if ((rc = c->ids.alloc((size_t)(v.n_ids > 0 ? v.n_ids : 1))) || (rc = c->soff.alloc(soff.size()))) return rc;
  if (v.n_ids > 0) W2V_HIP_TRY(hipMemcpy(c->ids.get(), v.ids, v.n_ids * sizeof(int32_t), hipMemcpyDeviceToDevice));
  W2V_HIP_TRY(hipMemcpy(c->soff.get(), v.offsets, soff.size() * sizeof(int64_t), hipMemcpyDeviceToDevice));
  return install_corpus(h, std::move(c), v.n_ids, v.n_sentences, max_len, v.train_words, std::move(hist));
}

int w2v_dev_adopt_corpus(w2v_dev* h, w2v_ingest* g) {
  w2v::Range range_("w2v_dev_adopt_corpus");
  if (!h || !g) return fail(W2V_ERR_ARG, "w2v_dev_adopt_corpus: null argument");
  return adopt_view(h, w2v::ingest_view(g), "w2v_dev_adopt_corpus", "ingest");
}

int w2v_dev_adopt_phrases(w2v_dev* h, w2v_phrase* p) {
  w2v::Range range_("w2v_dev_adopt_phrases");
  if (!h || !p) return fail(W2V_ERR_ARG, "w2v_dev_adopt_phrases: null argument");
  return adopt_view(h, w2v::phrase_view(p), "w2v_dev_adopt_phrases", "phrase handle");
}

int w2v_dev_share_corpus(w2v_dev* h, w2v_dev* src) {
  w2v::Range range_("w2v_dev_share_corpus");
  if (!h || !src || h == src) return fail(W2V_ERR_ARG, "w2v_dev_share_corpus: two distinct handles");
  if (!src->corpus_ready) return fail(W2V_ERR_STATE, "w2v_dev_share_corpus: the source has no corpus");
  if (src->device != h->device) return fail(W2V_ERR_ARG, "w2v_dev_share_corpus: the source is on another device");
  if (h->V != src->V) return fail(W2V_ERR_ARG, "w2v_dev_share_corpus: the vocabularies differ");
  if (set_device(h)) return W2V_ERR_HIP;
  W2V_HIP_TRY(hipStreamSynchronize(h->stream));
  if (h->corpus == src->corpus) return W2V_OK;
  return install_corpus(h, src->corpus, src->n_tok, src->n_sent, src->max_len, src->train_words, src->tok_count);
}

int w2v_dev_upload_replay(w2v_dev* h, const uint32_t* stream, int64_t n, const int64_t* off,
                          int64_t n_off) {
  if (!h || !off || (n > 0 && !stream)) return fail(W2V_ERR_ARG, "w2v_dev_upload_replay: null argument");
  for (int64_t k = 0; k < n_off; ++k)
    if (off[k] < 0 || off[k] > n) return fail(W2V_ERR_ARG, "replay offset out of range");
  if (set_device(h)) return W2V_ERR_HIP;
  w2v::DevBuf<uint32_t> r;
  w2v::DevBuf<int64_t> ro;
  int rc;
  if ((rc = r.alloc((size_t)(n > 0 ? n : 1))) || (rc = ro.alloc((size_t)(n_off > 0 ? n_off : 1)))) return rc;
  if (n > 0) W2V_HIP_TRY(hipMemcpy(r.get(), stream, n * sizeof(uint32_t), hipMemcpyHostToDevice));
  if (n_off > 0) W2V_HIP_TRY(hipMemcpy(ro.get(), off, n_off * sizeof(int64_t), hipMemcpyHostToDevice));
  h->replay = std::move(r), h->replay_off = std::move(ro);
  h->n_replay_off = n_off;
  return W2V_OK;
}

int w2v_dev_set_progress(w2v_dev* h, int64_t cw) {
  if (!h) return fail(W2V_ERR_ARG, "null handle");
  if (set_device(h)) return W2V_ERR_HIP;
  unsigned long long v = (unsigned long long)cw;
  W2V_HIP_TRY(hipMemcpyAsync(h->counters.get(), &v, sizeof(v), hipMemcpyHostToDevice, h->stream));
  W2V_HIP_TRY(hipStreamSynchronize(h->stream));
  return W2V_OK;
}

namespace w2v {
__global__ void set_counter_kernel(unsigned long long* p, unsigned long long v) { *p = v; }
}  // namespace w2v

int w2v_dev_set_progress_async(w2v_dev* h, int64_t cw) {
  if (!h) return fail(W2V_ERR_ARG, "null handle");
  if (cw < 0) return fail(W2V_ERR_ARG, "current_words must be >= 0");
  if (set_device(h)) return W2V_ERR_HIP;
  hipLaunchKernelGGL(w2v::set_counter_kernel, dim3(1), dim3(1), 0, h->stream, h->counters.get(), (unsigned long long)cw);
  W2V_HIP_TRY(hipGetLastError());
  return W2V_OK;
}

int w2v_dev_set_train_words(w2v_dev* h, int64_t train_words) {
  if (!h) return fail(W2V_ERR_ARG, "null handle");
  if (train_words <= 0) return fail(W2V_ERR_ARG, "train_words must be > 0");
  if (!h->corpus_ready) return fail(W2V_ERR_STATE, "upload the corpus first");
  h->train_words = train_words;
  return W2V_OK;
}

int w2v_dev_get_progress(w2v_dev* h, int64_t* cw) {
  if (!h || !cw) return fail(W2V_ERR_ARG, "null argument");
  if (set_device(h)) return W2V_ERR_HIP;
  unsigned long long v = 0;
  W2V_HIP_TRY(hipStreamSynchronize(h->stream));
  W2V_HIP_TRY(hipMemcpy(&v, h->counters.get(), sizeof(v), hipMemcpyDeviceToHost));
  *cw = (int64_t)v;
  return W2V_OK;
}

static int launch_train(w2v_dev* h, int32_t epoch, const int64_t* order_dev, int64_t count);

// The shared-negatives minibatch covers skip-gram NS only: a 16 x 16 MFMA tile
// holds <= 16 unique context rows (2 * window <= 16) and the center + <= 15
// negatives; its draws are Philox (the reference has no such path to replay).
static int check_shared_negatives(const w2v_dev* h, bool at_launch) {
  if (h->cfg.cbow || h->cfg.hs || h->cfg.negative <= 0)
    return fail(W2V_ERR_UNSUPPORTED, "shared negatives: skip-gram with negative sampling only (no hs, no cbow)");
  if (h->cfg.negative > kSnMaxNegative) return fail(W2V_ERR_UNSUPPORTED, "shared negatives: negative must be <= 15");
  if (h->cfg.window > kSnMaxWindow) return fail(W2V_ERR_UNSUPPORTED, "shared negatives: window must be <= 8");
  if (h->cfg.word_dim > kSnMaxDim) return fail(W2V_ERR_UNSUPPORTED, "shared negatives: word_dim must be <= 1024");
  if (at_launch && h->rng != W2V_RNG_PHILOX) return fail(W2V_ERR_UNSUPPORTED, "shared negatives: Philox draws only");
  return W2V_OK;
}

int w2v_dev_train_epoch_async(w2v_dev* h, int32_t epoch, const int64_t* order_dev) {
  if (!h) return fail(W2V_ERR_ARG, "null handle");
  return launch_train(h, epoch, order_dev, h->n_sent);
}

int w2v_dev_set_order(w2v_dev* h, const int64_t* order, int64_t n) {
  if (!h || (n > 0 && !order)) return fail(W2V_ERR_ARG, "w2v_dev_set_order: null argument");
  if (!h->corpus_ready) return fail(W2V_ERR_STATE, "upload the corpus first");
  if (n < 0 || n > h->n_sent) return fail(W2V_ERR_ARG, "order length must be in [0, n_sentences]");
  for (int64_t k = 0; k < n; ++k)
    if (order[k] < 0 || order[k] >= h->n_sent) return fail(W2V_ERR_ARG, "order entry out of range");
  if (set_device(h)) return W2V_ERR_HIP;
  W2V_HIP_TRY(hipStreamSynchronize(h->stream));  // a slice enqueued before may still read the old order
  if (n > 0) W2V_HIP_TRY(hipMemcpy(h->order.get(), order, n * sizeof(int64_t), hipMemcpyHostToDevice));
  h->n_order = n;
  return W2V_OK;
}

int w2v_dev_train_slice_async(w2v_dev* h, int32_t epoch, int64_t first, int64_t count) {
  if (!h) return fail(W2V_ERR_ARG, "null handle");
  if (first < 0 || count < 0 || first + count > h->n_order)
    return fail(W2V_ERR_ARG, "slice outside the order set with w2v_dev_set_order");
  return launch_train(h, epoch, h->order.get() + first, count);
}

int w2v_dev_train_sentences_async(w2v_dev* h, int32_t epoch, const int64_t* order_dev, int64_t count) {
  if (!h) return fail(W2V_ERR_ARG, "null handle");
  if (!order_dev && count != h->n_sent) return fail(W2V_ERR_ARG, "a slice needs an order array");
  if (count < 0) return fail(W2V_ERR_ARG, "count < 0");
  return launch_train(h, epoch, order_dev, count);
}

// What the policy reads of the handle for a launch of `count` sentences.
static w2v::PolicyInput policy_input(w2v_dev* h, int64_t count, int sn_waves) {
  w2v::PolicyInput in{h->set, h->knobs, stats_of(h)};
  in.window = h->cfg.window; in.negative = h->cfg.negative; in.hs = h->cfg.hs != 0; in.cbow = h->cfg.cbow != 0;
  in.V = h->V; in.pitch = h->pitch; in.nv = h->nv; in.n_cu = h->n_cu;
  in.sched = h->sched; in.update = h->update; in.rng = h->rng; in.replicas = h->replicas;
  in.n_sent = h->n_sent; in.max_len = h->max_len; in.count = count; in.sn_waves = sn_waves;
  return in;
}

// The device buffers a plan asks for: the atomic hot Huffman nodes' scales and
// the per-wave id slices of a CBOW window past kMaxWideWindow.
static int launch_buffers(w2v_dev* h, const w2v::LaunchPlan& p, w2v::TrainArgs& a) {
  if (!p.hot_sc.empty()) {  // the atomic hot Huffman nodes' scales
    const int64_t nodes = (int64_t)p.hot_sc.size();
    if (p.hot_sc != h->hot_sc_h || !h->hot_sc_d.get()) {
      W2V_HIP_TRY(hipStreamSynchronize(h->stream));  // an earlier launch may still read the old scales
      h->hot_sc_h.clear();  // until the copy below has landed
      if (nodes > (int64_t)h->hot_sc_d.size())
        if (int rc = h->hot_sc_d.alloc((size_t)nodes)) return rc;
      W2V_HIP_TRY(hipMemcpy(h->hot_sc_d.get(), p.hot_sc.data(), (size_t)nodes * sizeof(float), hipMemcpyHostToDevice));
      h->hot_sc_h = p.hot_sc;
    }
    a.hot_sc = h->hot_sc_d.get();
  }
  if (p.wide_scratch > 0) {  // cbow_center_huge: one id slice per wave
    if (p.wide_scratch > (int64_t)h->wide_scratch.size()) {
      W2V_HIP_TRY(hipStreamSynchronize(h->stream));  // an earlier launch may still use the old slices
      if (int rc = h->wide_scratch.alloc((size_t)p.wide_scratch)) return rc;
    }
    a.wide_ids = h->wide_scratch.get();
    a.wide_stride = p.wide_stride;
  }
  return W2V_OK;
}

static int launch_train(w2v_dev* h, int32_t epoch, const int64_t* order_dev, int64_t count) {
  w2v::Range range_("w2v launch");
  if (!h->vocab_ready || !h->corpus_ready) return fail(W2V_ERR_STATE, "upload vocab and corpus first");
  if (!h->model_ready) return fail(W2V_ERR_STATE, "upload the model first");
  if (h->cfg.negative > 0 && !h->table.get()) return fail(W2V_ERR_STATE, "no unigram table on the device");
  if (h->rng == W2V_RNG_REPLAY) {
    if (!h->replay.get()) return fail(W2V_ERR_STATE, "replay mode without a replay stream");
    if ((int64_t)(epoch + 1) * h->n_sent > h->n_replay_off)
      return fail(W2V_ERR_ARG, "replay offsets do not cover this epoch");
  }
  if (epoch < 0) return fail(W2V_ERR_ARG, "epoch must be >= 0");
  KernelFn sn_fn = nullptr;
  int sn_waves = 0;
  if (h->update == W2V_UPDATE_SHARED_NEGATIVES) {
    if (int rc = check_shared_negatives(h, true)) return rc;
    const int occ = h->knobs.sn_occ;  // register budget (waves per SIMD); experiment knob
    if ((double)h->V * (double)h->pitch * sizeof(float) >= 4294967296.0)
      return fail(W2V_ERR_UNSUPPORTED, "shared negatives: W / C must be < 4 GiB each (32-bit buffer offsets)");
    if (!(sn_fn = w2v::pick_shared_neg(h->pitch, occ, &sn_waves)))
      return fail(W2V_ERR_UNSUPPORTED, "shared negatives: row pitch must be 64 * {1..8,10,12,14,16} floats");
  }
  if (count == 0) return W2V_OK;
  if (set_device(h)) return W2V_ERR_HIP;
  w2v::TrainArgs a{};
  a.W = h->W; a.C = h->C; a.S = h->S;
  a.pitch = h->pitch; a.dim = h->cfg.word_dim;
  a.window = h->cfg.window; a.negative = h->cfg.negative; a.cbow_mean = h->cfg.cbow_mean;
  a.iter = h->cfg.iter; a.init_alpha = h->cfg.init_alpha; a.min_alpha = h->cfg.min_alpha;
  a.train_words = (double)h->train_words;
  a.ids = h->corpus->ids.get(); a.soff = h->corpus->soff.get(); a.order = order_dev; a.n_sent = count; a.n_corpus = h->n_sent;
  a.keep = h->keep.get(); a.table = h->table.get(); a.table_size = h->cfg.table_size;
  a.codes = h->codes.get(); a.points = h->points.get(); a.coff = h->coff.get();
  a.replay = h->replay.get();
  a.replay_off = h->replay_off.get() ? h->replay_off.get() + (int64_t)epoch * h->n_sent : nullptr;
  a.words = h->counters.get();
  a.work = h->work.get();
  a.stats = h->counters.get() + 1;
  a.key0 = (uint32_t)h->seed; a.key1 = (uint32_t)(h->seed >> 32);
  a.epoch = (uint32_t)epoch;
  a.fixed_alpha = h->fixed_alpha;
  a.strict = h->sched == W2V_SCHED_SEQUENTIAL ? 1 : 0;
  W2V_HIP_TRY(hipMemsetAsync(h->work.get(), 0, sizeof(unsigned int), h->stream));  // runs while the host plans
  // the policy (w2v_policy.cpp) decides the rest
  const KernelFn occ_fn = sn_fn ? sn_fn : kernel_for(h), deep_fn = sn_fn ? sn_fn : kernel_deep_for(h);
  hipError_t occ_err = hipSuccess;
  auto occupancy = [&](w2v::OccKernel k, int threads, int64_t lds) {
    int per_cu = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &per_cu, k == w2v::kOccTrainDeep ? deep_fn : occ_fn, threads, (size_t)lds);
    if (e != hipSuccess) occ_err = e;
    return per_cu;
  };
  w2v::LaunchPlan p = w2v::plan_launch(policy_input(h, count, sn_waves), occupancy);
  if (occ_err != hipSuccess)
    return fail(W2V_ERR_HIP, std::string("hipOccupancyMaxActiveBlocksPerMultiprocessor: ") + hipGetErrorString(occ_err));
  // what this launch did not decide keeps the value of the last launch that did (the accessors' contract)
  if (p.private_rate < 0.0) p.private_rate = h->last_plan.private_rate;
  if (p.tau_rows < 0.0) p.tau_rows = h->last_plan.tau_rows;
  if (p.hs_hot_avg < 0.0) p.hs_hot_avg = h->last_plan.hs_hot_avg;
  a.hot_wc = p.hot_wc; a.hot_s = p.hot_s; a.hot_atomic = p.hot_atomic;
  a.priv_lo = p.priv_lo; a.priv_n = p.priv_n; a.ctx_n = p.ctx_n; a.priv_avg = p.priv_avg;
  a.flush_every = p.flush_every; a.ctx_flush_every = p.ctx_flush_every;
  a.nseg = p.nseg; a.seg_len = p.seg_len;
  std::memcpy(a.priv_sc, p.priv_sc, sizeof(a.priv_sc));
  std::memcpy(a.ctx_sc, p.ctx_sc, sizeof(a.ctx_sc));
  if (!p.shared) {
    if (p.priv_n > 0) a.priv_M = h->cfg.hs ? h->S : (h->cfg.cbow ? h->W : h->C);
    if (p.ctx_n > 0) a.ctx_M = h->C;
  }
  if (int rc = launch_buffers(h, p, a)) return rc;
  const KernelFn fn = p.deep ? deep_fn : occ_fn;
  const dim3 grid((unsigned)p.grid), block((unsigned)p.threads);
  const size_t lds_bytes = (size_t)p.lds_bytes;
  h->last_plan = std::move(p);
  hipLaunchKernelGGL(fn, grid, block, lds_bytes, h->stream, a);
  W2V_HIP_TRY(hipGetLastError());
  return W2V_OK;
}

int w2v_dev_train_epoch(w2v_dev* h, int32_t epoch, const int64_t* order, w2v_dev_stats* st) {
  w2v::Range range_("w2v_dev_train_epoch");
  if (!h) return fail(W2V_ERR_ARG, "null handle");
  w2v_dev_stats before{};
  {
    int rc = w2v_dev_read_stats(h, &before);
    if (rc) return rc;
  }
  const int64_t* od = nullptr;
  if (order) {
    for (int64_t k = 0; k < h->n_sent; ++k)
      if (order[k] < 0 || order[k] >= h->n_sent) return fail(W2V_ERR_ARG, "order entry out of range");
    if (set_device(h)) return W2V_ERR_HIP;
    W2V_HIP_TRY(hipMemcpyAsync(h->order.get(), order, h->n_sent * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    od = h->order.get();
    h->n_order = h->n_sent;
  }
  int rc = w2v_dev_train_epoch_async(h, epoch, od);
  if (rc) return rc;
  W2V_HIP_TRY(hipStreamSynchronize(h->stream));
  w2v_dev_stats after{};
  rc = w2v_dev_read_stats(h, &after);
  if (rc) return rc;
  if (st) {
    st->words += after.words - before.words;
    st->centers += after.centers - before.centers;
    st->contexts += after.contexts - before.contexts;
    st->targets += after.targets - before.targets;
    st->draws += after.draws - before.draws;
    st->sentences += after.sentences - before.sentences;
    st->nonfinite += after.nonfinite - before.nonfinite;
  }
  if (after.nonfinite > before.nonfinite)
    return fail(W2V_ERR_DIVERGED, "training diverged: " + std::to_string(after.nonfinite - before.nonfinite) +
                                      " non-finite sigma arguments (row . input) in this epoch; "
                                      "lower init_alpha or use a less aggressive update policy");
  return W2V_OK;
}

int w2v_dev_synchronize(w2v_dev* h) {
  w2v::Range range_("w2v_dev_synchronize");
  if (!h) return fail(W2V_ERR_ARG, "null handle");
  if (set_device(h)) return W2V_ERR_HIP;
  W2V_HIP_TRY(hipStreamSynchronize(h->stream));
  return W2V_OK;
}

int w2v_dev_read_stats(w2v_dev* h, w2v_dev_stats* st) {
  if (!h || !st) return fail(W2V_ERR_ARG, "null argument");
  if (set_device(h)) return W2V_ERR_HIP;
  unsigned long long c[8];
  W2V_HIP_TRY(hipStreamSynchronize(h->stream));
  W2V_HIP_TRY(hipMemcpy(c, h->counters.get(), sizeof(c), hipMemcpyDeviceToHost));
  st->words = (int64_t)c[0];
  st->centers = (int64_t)c[1];
  st->contexts = (int64_t)c[2];
  st->targets = (int64_t)c[3];
  st->draws = (int64_t)c[4];
  st->sentences = (int64_t)c[5];
  st->nonfinite = (int64_t)c[6];
  return W2V_OK;
}

int w2v_dev_reset_stats(w2v_dev* h) {
  if (!h) return fail(W2V_ERR_ARG, "null handle");
  if (set_device(h)) return W2V_ERR_HIP;
  W2V_HIP_TRY(hipMemsetAsync(h->counters.get() + 1, 0, 7 * sizeof(unsigned long long), h->stream));
  W2V_HIP_TRY(hipStreamSynchronize(h->stream));
  return W2V_OK;
}

int w2v_dev_set_max_waves(w2v_dev* h, int64_t n) {
  if (!h) return fail(W2V_ERR_ARG, "null handle");
  if (n < 0) return fail(W2V_ERR_ARG, "max_waves must be >= 0");
  h->set.max_waves = n;
  return W2V_OK;
}

int w2v_dev_set_private_rows(w2v_dev* h, int32_t n) {
  if (!h) return fail(W2V_ERR_ARG, "null handle");
  if (n < -1) return fail(W2V_ERR_ARG, "private_rows must be >= -1");
  h->set.private_rows = n;
  return W2V_OK;
}

int w2v_dev_set_context_private(w2v_dev* h, int32_t rows, int32_t flush_centers) {
  if (!h) return fail(W2V_ERR_ARG, "null handle");
  if (rows < -1) return fail(W2V_ERR_ARG, "context rows must be >= -1");
  if (flush_centers < 0) return fail(W2V_ERR_ARG, "flush_centers must be >= 0");
  h->set.context_rows = rows;
  h->set.context_flush = flush_centers;
  return W2V_OK;
}

int w2v_dev_set_private_sync(w2v_dev* h, int32_t flush_centers, float average_over) {
  if (!h) return fail(W2V_ERR_ARG, "null handle");
  if (flush_centers < 0) return fail(W2V_ERR_ARG, "flush_centers must be >= 0");
  if (!(average_over >= 0.0f)) return fail(W2V_ERR_ARG, "average_over must be >= 0");
  h->set.flush_centers = flush_centers;
  h->set.private_average = average_over;
  return W2V_OK;
}

int w2v_dev_set_update(w2v_dev* h, int32_t mode) {
  if (!h) return fail(W2V_ERR_ARG, "null handle");
  if (mode != W2V_UPDATE_PER_PAIR && mode != W2V_UPDATE_SHARED_NEGATIVES) return fail(W2V_ERR_ARG, "bad update mode");
  if (mode == W2V_UPDATE_SHARED_NEGATIVES)
    if (int rc = check_shared_negatives(h, false)) return rc;
  h->update = mode;
  return W2V_OK;
}

int w2v_dev_set_hot_rows(w2v_dev* h, int64_t hot_rows) {
  if (!h) return fail(W2V_ERR_ARG, "null handle");
  if (hot_rows < W2V_HOT_AUTO) return fail(W2V_ERR_ARG, "hot_rows must be >= -2 (W2V_HOT_AUTO)");
  h->set.hot_rows = hot_rows;
  return W2V_OK;
}

int w2v_dev_set_private_rate(w2v_dev* h, float mu) {
  if (!h) return fail(W2V_ERR_ARG, "null handle");
  if (!(mu >= 0.0f) && mu != -1.0f) return fail(W2V_ERR_ARG, "private_rate must be >= 0 (or -1: automatic)");
  h->set.private_rate = mu;
  return W2V_OK;
}

int w2v_dev_set_hot_auto(w2v_dev* h, float tau_rows, float tau_nodes) {
  if (!h) return fail(W2V_ERR_ARG, "null handle");
  if (!(tau_rows >= 0.0f) || !(tau_nodes > 0.0f))
    return fail(W2V_ERR_ARG, "the automatic hot-row thresholds must be >= 0 (rows; 0 = by vocab) and > 0 (nodes)");
  h->set.hot_tau_rows = tau_rows;
  h->set.hot_tau_nodes = tau_nodes;
  return W2V_OK;
}

int w2v_dev_policy(w2v_dev* h, int64_t* hot_rows, int64_t* hot_nodes, int32_t* private_rows, int32_t* context_rows) {
  if (!h) return fail(W2V_ERR_ARG, "null handle");
  if (hot_rows) *hot_rows = h->last_plan.hot_rows;
  if (hot_nodes) *hot_nodes = h->last_plan.hot_nodes;
  if (private_rows) *private_rows = h->last_plan.priv_n;
  if (context_rows) *context_rows = h->last_plan.ctx_n;
  return W2V_OK;
}

int w2v_dev_hot_tau(w2v_dev* h, float* tau_rows, float* tau_nodes) {
  if (!h) return fail(W2V_ERR_ARG, "null handle");
  if (tau_rows) *tau_rows = (float)h->last_plan.tau_rows;
  if (tau_nodes) *tau_nodes = (float)h->set.hot_tau_nodes;
  return W2V_OK;
}

int w2v_dev_private_rate_used(w2v_dev* h, float* mu) {
  if (!h) return fail(W2V_ERR_ARG, "null handle");
  if (mu) *mu = (float)h->last_plan.private_rate;
  return W2V_OK;
}

int w2v_dev_wave_cap_used(w2v_dev* h, int64_t* waves) {
  if (!h) return fail(W2V_ERR_ARG, "null handle");
  if (waves) *waves = h->last_plan.wave_cap;
  return W2V_OK;
}

int w2v_dev_deep_used(w2v_dev* h, int32_t* deep) {
  if (!h || !deep) return fail(W2V_ERR_ARG, "null argument");
  *deep = h->last_plan.deep ? 1 : 0;
  return W2V_OK;
}

int w2v_dev_launch_plan(w2v_dev* h, w2v_launch_plan* out, float* hot_sc, int64_t hot_sc_cap) {
  if (!h || !out) return fail(W2V_ERR_ARG, "null argument");
  *out = h->last_plan;  // the plan's public part
  out->n_hot_sc = (int64_t)h->last_plan.hot_sc.size();
  if (hot_sc) std::copy_n(h->last_plan.hot_sc.begin(), std::min(hot_sc_cap, out->n_hot_sc), hot_sc);
  return W2V_OK;
}

int w2v_dev_set_replica_count(w2v_dev* h, int32_t n) {
  if (!h) return fail(W2V_ERR_ARG, "null handle");
  if (n < 1) return fail(W2V_ERR_ARG, "replica count must be >= 1");
  w2v::set_replicas(h, n);
  return W2V_OK;
}

int w2v_dev_replica_count(w2v_dev* h, int32_t* n) {
  if (!h || !n) return fail(W2V_ERR_ARG, "null argument");
  *n = h->replicas;
  return W2V_OK;
}

int w2v_dev_row_update_rates(w2v_dev* h, int32_t which, double* out, int64_t n) {
  if (!h || !out) return fail(W2V_ERR_ARG, "null argument");
  if (which < 0 || which > 2) return fail(W2V_ERR_ARG, "which must be 0 (W), 1 (C) or 2 (synapses1)");
  std::vector<double> rate;
  if (!w2v::row_update_rates(h, which, rate)) return fail(W2V_ERR_STATE, "no vocab / corpus statistics uploaded");
  if (n != (int64_t)rate.size()) return fail(W2V_ERR_ARG, "n must be the matrix's row count");
  std::copy(rate.begin(), rate.end(), out);
  return W2V_OK;
}

int w2v_dev_flush_policy(w2v_dev* h, int32_t* flush_centers, int32_t* context_flush) {
  if (!h) return fail(W2V_ERR_ARG, "null handle");
  if (flush_centers) *flush_centers = h->last_plan.priv_n > 0 ? h->last_plan.flush_every : 0;
  if (context_flush) *context_flush = h->last_plan.ctx_n > 0 ? h->last_plan.ctx_flush_every : 0;
  return W2V_OK;
}

int w2v_dev_set_fixed_alpha(w2v_dev* h, float alpha) {
  if (!h) return fail(W2V_ERR_ARG, "null handle");
  h->fixed_alpha = alpha > 0 ? alpha : 0.0f;
  return W2V_OK;
}

int w2v_dev_apply_rows(w2v_dev* h, float* rows, const uint8_t* codes, int32_t n, const float* x, float* grad,
                       float alpha, int32_t hs_form) {
  if (!h || !x || !grad || (n > 0 && (!rows || !codes))) return fail(W2V_ERR_ARG, "null argument");
  if (n < 0) return fail(W2V_ERR_ARG, "n < 0");
  if (set_device(h)) return W2V_ERR_HIP;
  const int64_t need = (int64_t)(n + 2) * h->pitch;
  if ((int64_t)h->scratch_f.size() < need) {
    w2v::DevBuf<float> f;
    w2v::DevBuf<uint8_t> c;
    int rc;
    if ((rc = f.alloc((size_t)need)) || (rc = c.alloc((size_t)(n > 64 ? n : 64)))) return rc;
    h->scratch_f = std::move(f), h->scratch_codes = std::move(c);
  }
  const size_t d = (size_t)h->cfg.word_dim, dp = (size_t)h->pitch * sizeof(float);
  float* dx = h->scratch_f.get();
  float* dg = dx + h->pitch;
  float* dr = dx + 2 * h->pitch;
  W2V_HIP_TRY(hipMemsetAsync(dx, 0, need * sizeof(float), h->stream));
  W2V_HIP_TRY(hipMemcpyAsync(dx, x, d * sizeof(float), hipMemcpyHostToDevice, h->stream));
  W2V_HIP_TRY(hipMemcpyAsync(dg, grad, d * sizeof(float), hipMemcpyHostToDevice, h->stream));
  if (n > 0) {
    W2V_HIP_TRY(hipMemcpy2DAsync(dr, dp, rows, d * sizeof(float), d * sizeof(float), n, hipMemcpyHostToDevice, h->stream));
    W2V_HIP_TRY(hipMemcpyAsync(h->scratch_codes.get(), codes, n, hipMemcpyHostToDevice, h->stream));
  }
  w2v::ApplyFn fn = apply_for(h);
  hipLaunchKernelGGL(fn, dim3(1), dim3(64), 0, h->stream, dr, h->pitch, h->cfg.word_dim, dx, dg, h->scratch_codes.get(),
                     n, alpha, hs_form);
  W2V_HIP_TRY(hipGetLastError());
  W2V_HIP_TRY(hipMemcpyAsync(grad, dg, d * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (n > 0)
    W2V_HIP_TRY(hipMemcpy2DAsync(rows, d * sizeof(float), dr, dp, d * sizeof(float), n, hipMemcpyDeviceToHost, h->stream));
  W2V_HIP_TRY(hipStreamSynchronize(h->stream));
  return W2V_OK;
}

int w2v_dev_score_limits(int32_t* max_dim, int32_t* max_window, int32_t* max_negative) {
  if (max_dim) *max_dim = w2v::kScoreMaxDim;
  if (max_window) *max_window = w2v::kScoreMaxWindow;
  if (max_negative) *max_negative = w2v::kScoreMaxNegative;
  return W2V_OK;
}

int w2v_dev_set_score_item(w2v_dev* h, int32_t centers) {
  if (centers < 0 || centers % w2v::kWave != 0)
    return fail(W2V_ERR_ARG, "w2v_dev_set_score_item: centers must be 0 (automatic) or a multiple of 64");
  if (!h) return fail(W2V_ERR_ARG, "w2v_dev_set_score_item: null handle");
  h->score_item = centers;
  return W2V_OK;
}

int w2v_dev_score(w2v_dev* h, const int32_t* ids, int64_t n_tok, const int64_t* soff, int64_t n_sent, uint64_t key,
                  double* out_ll, int64_t* out_targets, w2v_score_summary* summary) {
  w2v::Range range_("w2v_dev_score");
  if (!h) return fail(W2V_ERR_ARG, "w2v_dev_score: null handle");
  const w2v_dev_config& cfg = h->cfg;
  if (cfg.word_dim > w2v::kScoreMaxDim)
    return fail(W2V_ERR_UNSUPPORTED, "w2v_dev_score: word_dim > " + std::to_string(w2v::kScoreMaxDim) + " unsupported");
  if (cfg.window > w2v::kScoreMaxWindow)
    return fail(W2V_ERR_UNSUPPORTED, "w2v_dev_score: window > " + std::to_string(w2v::kScoreMaxWindow) +
                                         " unsupported (a window's distinct ids are held in registers)");
  if (cfg.negative > w2v::kScoreMaxNegative)
    return fail(W2V_ERR_UNSUPPORTED, "w2v_dev_score: negative > " + std::to_string(w2v::kScoreMaxNegative) +
                                         " unsupported (a context's draws are one wave pass)");
  if (cfg.hs && cfg.negative > 0)
    return fail(W2V_ERR_UNSUPPORTED, "w2v_dev_score: hs together with negative > 0 has no single objective");
  if (!h->vocab_ready) return fail(W2V_ERR_STATE, "w2v_dev_score: upload the vocab first");
  if (!h->model_ready) return fail(W2V_ERR_STATE, "w2v_dev_score: upload the model first");
  if (!cfg.hs && !h->table.get()) return fail(W2V_ERR_STATE, "w2v_dev_score: no unigram table on the device");
  const bool resident = !ids && !soff;
  if (resident) {
    if (!h->corpus_ready) return fail(W2V_ERR_STATE, "w2v_dev_score: no resident corpus to score (ids == NULL)");
    n_tok = h->n_tok;
    n_sent = h->n_sent;
  } else {
    if (!soff || (n_tok > 0 && !ids)) return fail(W2V_ERR_ARG, "w2v_dev_score: null argument");
    if (n_sent < 0 || n_tok < 0 || n_sent > (int64_t)UINT32_MAX - 1)
      return fail(W2V_ERR_ARG, "w2v_dev_score: sizes out of range");
    if (soff[0] != 0 || soff[n_sent] != n_tok)
      return fail(W2V_ERR_ARG, "w2v_dev_score: sentence offsets must span [0, n_tokens]");
    for (int64_t s = 0; s < n_sent; ++s)
      if (soff[s] > soff[s + 1] || soff[s + 1] - soff[s] > (int64_t)INT32_MAX)
        return fail(W2V_ERR_ARG, "w2v_dev_score: sentence offsets must be non-decreasing");
    for (int64_t t = 0; t < n_tok; ++t)
      if (ids[t] < 0 || ids[t] >= h->V) return fail(W2V_ERR_ARG, "w2v_dev_score: token id out of vocab range");
  }
  if (set_device(h)) return W2V_ERR_HIP;
  W2V_HIP_TRY(hipStreamSynchronize(h->stream));  // the training enqueued so far has written the model
  // the work items: up to `item` consecutive centers of one sentence
  std::vector<int64_t> off_h;
  if (resident) {
    off_h.resize((size_t)n_sent + 1);
    W2V_HIP_TRY(hipMemcpy(off_h.data(), h->corpus->soff.get(), off_h.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    soff = off_h.data();
  }
  const int64_t item = h->score_item > 0 ? h->score_item : w2v::kScoreAutoItem;
  std::vector<int64_t> item_off((size_t)n_sent + 1, 0);
  for (int64_t s = 0; s < n_sent; ++s) item_off[(size_t)s + 1] = item_off[(size_t)s] + (soff[s + 1] - soff[s] + item - 1) / item;
  const int64_t n_items = item_off[(size_t)n_sent];
  int rc;
  // no empty buffers: nothing to score still gets one element each
  const size_t items1 = (size_t)std::max<int64_t>(n_items, 1), sents1 = (size_t)std::max<int64_t>(n_sent, 1),
               toks1 = (size_t)std::max<int64_t>(n_tok, 1);
  if ((rc = h->score_item_off.reserve((size_t)n_sent + 1)) || (rc = h->score_part_ll.reserve(items1)) ||
      (rc = h->score_part_targets.reserve(items1)) || (rc = h->score_part_nonfinite.reserve(items1)) ||
      (rc = h->score_ll.reserve(sents1)) || (rc = h->score_targets.reserve(sents1)) ||
      (rc = h->score_ctr.reserve((size_t)w2v::kScoreCounters)))
    return rc;
  if (!resident) {
    if ((rc = h->score_ids.reserve(toks1)) || (rc = h->score_soff.reserve((size_t)n_sent + 1))) return rc;
    if (n_tok > 0) W2V_HIP_TRY(hipMemcpy(h->score_ids.get(), ids, n_tok * sizeof(int32_t), hipMemcpyHostToDevice));
    W2V_HIP_TRY(hipMemcpy(h->score_soff.get(), soff, (n_sent + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  }
  W2V_HIP_TRY(hipMemcpy(h->score_item_off.get(), item_off.data(), item_off.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  w2v::ScoreArgs a{};
  a.W = h->W; a.C = h->C; a.S = h->S; a.pitch = h->pitch;
  a.window = cfg.window; a.negative = cfg.negative; a.cbow_mean = cfg.cbow_mean; a.item = (int32_t)item;
  a.ids = resident ? h->corpus->ids.get() : h->score_ids.get();
  a.soff = resident ? h->corpus->soff.get() : h->score_soff.get();
  a.item_off = h->score_item_off.get(); a.n_sent = n_sent; a.n_items = n_items;
  a.table = h->table.get(); a.table_size = cfg.table_size;
  a.codes = h->codes.get(); a.points = h->points.get(); a.coff = h->coff.get();
  a.key0 = (uint32_t)key; a.key1 = (uint32_t)(key >> 32);
  a.part_ll = h->score_part_ll.get(); a.part_targets = h->score_part_targets.get();
  a.part_nonfinite = h->score_part_nonfinite.get(); a.ctr = h->score_ctr.get();
  a.ll = h->score_ll.get(); a.targets = h->score_targets.get();
  if ((rc = w2v::score_launch(a, h->nv, cfg.cbow != 0, cfg.hs != 0, h->set.max_waves, h->n_cu, h->stream))) return rc;
  W2V_HIP_TRY(hipStreamSynchronize(h->stream));
  std::vector<double> ll_h;
  if (!out_ll && summary) {  // the summary's ll is the sentences' sum, in sentence order
    ll_h.resize((size_t)n_sent);
    out_ll = ll_h.data();
  }
  if (out_ll && n_sent > 0) W2V_HIP_TRY(hipMemcpy(out_ll, a.ll, n_sent * sizeof(double), hipMemcpyDeviceToHost));
  if (out_targets && n_sent > 0)
    W2V_HIP_TRY(hipMemcpy(out_targets, a.targets, n_sent * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (summary) {
    unsigned long long c[w2v::kScoreCounters];
    W2V_HIP_TRY(hipMemcpy(c, a.ctr, sizeof(c), hipMemcpyDeviceToHost));
    std::vector<int64_t> tg_h;
    const int64_t* tg = out_targets;
    if (!tg && n_sent > 0) {
      tg_h.resize((size_t)n_sent);
      W2V_HIP_TRY(hipMemcpy(tg_h.data(), a.targets, n_sent * sizeof(int64_t), hipMemcpyDeviceToHost));
      tg = tg_h.data();
    }
    w2v_score_summary r{};
    r.sentences = n_sent;
    r.words = n_tok;
    r.centers = (int64_t)c[w2v::kScoreCenters];
    r.contexts = (int64_t)c[w2v::kScoreContexts];
    r.draws = (int64_t)c[w2v::kScoreDraws];
    r.nonfinite = (int64_t)c[w2v::kScoreNonFinite];
    for (int64_t s = 0; s < n_sent; ++s) {
      r.targets += tg[s];
      r.ll += out_ll[s];
    }
    *summary = r;
  }
  return W2V_OK;
}

}  // extern "C"
