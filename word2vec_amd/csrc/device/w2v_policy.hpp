// w2v_policy.hpp — the update policy of a training launch: from the corpus
// statistics, the configuration and the chip's size to everything launch_train
// (w2v_dev.hip) puts into TrainArgs and the launch. Plain C++: no HIP, no
// handle; a CPU program can run it (check/policy_selftest.cpp).
#pragma once
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "w2v_dev.h"
#include "w2v_limits.hpp"

namespace w2v {

// Experiment knobs (environment variables, read ONCE at w2v_dev_create and
// reported by w2v_dev_knobs / bench.py's JSON): a stray variable must not
// change a training run silently. -1 / 0 = not set.
struct Knobs {
  int64_t seg_len = -1;          // W2V_SEG_LEN: tokens per work item (0 = whole sentences)
  int wpb = 0;                   // W2V_DEBUG_WPB: waves per workgroup
  int64_t lds_per_wave = 0;      // W2V_DEBUG_LDS_PER_WAVE: LDS budget per wave (bytes)
  int64_t max_blocks = 0;        // W2V_DEBUG_MAX_BLOCKS: grid cap
  int sn_occ = 0;                // W2V_SN_OCC: shared-negatives kernel's waves per SIMD
  int64_t sn_coherent_rows = -1; // W2V_SN_COHERENT_ROWS
  int64_t sn_atomic_rows = -1;   // W2V_SN_ATOMIC_ROWS
  int scale_resident = 0;        // W2V_SCALE_RESIDENT=1: flush scales from the chip's resident workgroups, not the launch's grid
  double priv_tail_avg = -1;     // W2V_PRIV_TAIL_AVG: private_average of the NS output rows past the 64th (0 = plain sum)
  int sn_per_cu = 0;             // W2V_SN_PER_CU: shared-negatives workgroups per CU (cap)
  double ctx_avg = -1;           // W2V_CTX_AVG: private_average of the CBOW context rows (0 = plain sum)
  double priv_hs_tail_avg = -1;  // W2V_PRIV_HS_TAIL_AVG: private_average of the HS nodes past the 64th
  double hs_hot_avg = -1;        // W2V_HS_HOT_AVG: concurrent updates the atomic hot HS nodes' deltas are scaled to (0 = none)
  int wide_hs = -1;              // W2V_WIDE_HS: 0 = never the large-vocabulary HS rule, 1 = at any V (experiments)
  int deep_hs = -1;              // W2V_DEEP_HS: 1 forces the deep-pipeline HS kernel, 0 never (auto: capped HS launches)
  std::string desc;             // "NAME=value ..." of the variables that were set
};

// Statistics of the vocab and corpus the policy's frequency-derived settings
// use: per word f = token share, fk = kept-center share; per internal Huffman
// node the same summed over the words below it.
struct RowStats {
  bool stats_ok = false;
  double kept_tokens = 0.0;         // expected kept centers of one epoch over the corpus (sum count * min(1, keep))
  std::vector<double> f, fk, node_f, node_fk;
  double path_len_f = 0.0, path_len_fk = 0.0;  // HS: mean Huffman code length over the tokens / the kept centers
  std::vector<double> table_frac;   // unigram-table share of each word (set by the table's upload, not by row_stats)

  bool has_nodes(int64_t V) const { return (int64_t)node_f.size() == V - 1; }
  double u(int64_t r) const { return r < (int64_t)table_frac.size() ? table_frac[(size_t)r] : 0.0; }
  // Expected updates per kept center (the table above priv_scales in
  // w2v_policy.cpp); win1 = window + 1, neg = negative.
  // NS output row: SG (window + 1) (f + neg u); CBOW and shared negatives fk + neg u.
  double out_rate(int64_t r, bool center_side, double win1, double neg) const {
    return center_side ? fk[(size_t)r] + neg * u(r) : win1 * (f[(size_t)r] + neg * u(r));
  }
  // CBOW context row.
  double ctx_rate(int64_t r, double win1) const { return win1 * f[(size_t)r]; }
  // Huffman node: SG every context's path, CBOW the center's.
  double node_rate(int64_t j, bool cbow, double win1) const {
    return cbow ? node_fk[(size_t)j] : win1 * node_f[(size_t)j];
  }
};

// Per-word and per-node shares of the corpus, from the uploaded host vectors
// (tok_count: corpus tokens per word; keep: sample probabilities; leaf_node:
// per word the deepest internal node of its path, -1: none; node_parent: parent
// of each internal node, -1 for the root). s.table_frac is left as it is.
void row_stats(RowStats& s, int64_t V, const std::vector<int64_t>& tok_count, const std::vector<float>& keep,
               const std::vector<int32_t>& leaf_node, const std::vector<int32_t>& node_parent);

// Which kernel's residency the policy asks for.
enum OccKernel { kOccTrain, kOccTrainDeep, kOccSharedNeg };
// Workgroups of `threads` threads and `lds_bytes` of dynamic LDS one CU holds.
using Occupancy = std::function<int(OccKernel kernel, int threads, int64_t lds_bytes)>;

// The setters' values (include/w2v_dev.h).
struct PolicySettings {
  int64_t hot_rows = W2V_HOT_AUTO;  // rows updated with atomics: -2 = auto, -1 = all, 0 = none
  int32_t private_rows = -1;  // hottest output rows privatised in LDS: -1 = auto, 0 = off
  int32_t flush_centers = 0;  // workgroup centers between flushes of the privatised rows (0 = auto)
  float private_average = 8.0f;  // concurrency the privatised rows' summed deltas are scaled to (0 = plain sum)
  int32_t context_rows = -1;  // CBOW: hottest context rows privatised in LDS too: -1 = auto, 0 = off
  int32_t context_flush = 0;  // workgroup centers between flushes of the context rows (0 = auto)
  int64_t max_waves = 0;      // cap on concurrently scheduled wavefronts (0 = as many as fit)
  double hot_tau_rows = 0.0;  // automatic hot rows: expected concurrent updates threshold, W / C rows (0 = the default)
  double hot_tau_nodes = 1.0; //   ... and Huffman nodes
  double private_rate = -1.0; // > 0: privatise only rows updated >= this many times per center (private_by_rate);
                              // 0: no rate limit; < 0 (default): automatic (private_rate_for)
};

struct PolicyInput : PolicySettings {
  const Knobs& knobs;
  const RowStats& stats;
  // w2v_dev_config
  int32_t window = 0, negative = 0;
  bool hs = false, cbow = false;
  // the handle's state
  int64_t V = 0, pitch = 0;
  int nv = 1, n_cu = 256;
  int32_t sched = W2V_SCHED_PARALLEL, update = W2V_UPDATE_PER_PAIR, rng = W2V_RNG_PHILOX, replicas = 1;
  int64_t n_sent = 0, max_len = 0;
  int64_t count = 0;     // sentences of this launch
  int sn_waves = 0;      // the shared-negatives kernel's waves per workgroup
};

// Everything decided for one launch: the public read-back's fields
// (w2v_launch_plan, include/w2v_dev.h; those named as in TrainArgs are copied
// there unchanged) and what only the launch code needs.
struct LaunchPlan : w2v_launch_plan {
  // private_rate, tau_rows, hs_hot_avg < 0: this launch did not decide them
  LaunchPlan() : w2v_launch_plan{} {
    grid = 1, threads = kWave, wpb = 1;
    private_rate = tau_rows = hs_hot_avg = -1.0;
  }
  int64_t max_waves = 0;      // the cap on waves in flight the launch runs under (0: none)
  int64_t hot_rows = 0;       // as w2v_dev_policy reports them
  std::vector<float> hot_sc;  // per atomic hot Huffman node [hot_s, V - 1): the scale of its deltas (empty: none)
  int64_t wide_stride = 0;    // CBOW windows past kMaxWideWindow: ints of a wave's id slice
};

// Work-item size of the parallel Philox schedule (tokens of a sentence per
// item) and the most items a sentence is cut into.
constexpr int64_t kSegLen = 128;
constexpr int64_t kMaxSeg = 64;

LaunchPlan plan_per_pair(const PolicyInput& in, const Occupancy& occupancy);
LaunchPlan plan_shared_negatives(const PolicyInput& in, const Occupancy& occupancy);
inline LaunchPlan plan_launch(const PolicyInput& in, const Occupancy& occupancy) {
  return in.update == W2V_UPDATE_SHARED_NEGATIVES ? plan_shared_negatives(in, occupancy) : plan_per_pair(in, occupancy);
}

}  // namespace w2v
