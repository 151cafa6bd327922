// w2v_score.hpp — what w2v_dev.hip (the C-ABI) needs of the scoring unit
// (w2v_score.hip): the kernels' arguments and their launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace w2v {

// The scoring kernels' range (w2v_dev_score_limits): a CBOW window's distinct
// ids fit in registers up to kMaxWideWindow; one context's draws fit one wave pass.
constexpr int32_t kScoreMaxDim = 2048, kScoreMaxWindow = 127, kScoreMaxNegative = 63;
// Automatic work item (centers): w2v_dev_set_score_item(h, 0).
constexpr int32_t kScoreAutoItem = 256;

// Slots of ScoreArgs::ctr.
enum { kScoreHead = 0, kScoreCenters, kScoreContexts, kScoreDraws, kScoreNonFinite, kScoreCounters = 8 };

struct ScoreArgs {
  const float* W;
  const float* C;
  const float* S;  // synapses1
  int64_t pitch;   // row pitch in floats
  int32_t window;
  int32_t negative;
  int32_t cbow_mean;
  int32_t item;             // centers per work item (a multiple of 64)
  const int32_t* ids;
  const int64_t* soff;      // n_sent + 1
  const int64_t* item_off;  // n_sent + 1: sentence s owns the items [item_off[s], item_off[s + 1])
  int64_t n_sent;
  int64_t n_items;
  const uint32_t* table;
  int64_t table_size;
  const uint8_t* codes;
  const int32_t* points;
  const int64_t* coff;
  uint32_t key0, key1;
  double* part_ll;           // per item: its terms' sum
  int64_t* part_targets;     // per item: its terms
  uint32_t* part_nonfinite;  // per item: its non-finite dot products
  unsigned long long* ctr;   // kScoreCounters counters, zeroed by the launch
  double* ll;                // per sentence (the second pass)
  int64_t* targets;
};

// Zero a.ctr, score every item (as many waves as fit, at most max_waves when
// > 0), then add each sentence's partials in item order. Enqueued on `stream`;
// returns a W2V_* code (w2v_dev_last_error holds the message).
int score_launch(const ScoreArgs& a, int nv, bool cbow, bool hs, int64_t max_waves, int n_cu, hipStream_t stream);

}  // namespace w2v
