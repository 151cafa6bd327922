// policy_selftest.cpp — runs the launch policy (device/w2v_policy.cpp) on the
// CPU with a stub for the occupancy query, over the modes, vocabulary sizes,
// launch sizes and row widths, with and without corpus statistics, and checks
// what the kernels assume of a plan (w2v_kernels.hpp, w2v_shared.hpp). Built
// under AddressSanitizer / UndefinedBehaviorSanitizer (make -C word2vec_amd/csrc
// asan; tests/test_host_sanitizers.py).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "w2v_policy.hpp"

namespace {

int failures = 0, plans = 0;
std::string where;
void expect(bool ok, const char* what) {
  if (!ok) {
    if (failures < 50) std::fprintf(stderr, "FAIL: %s [%s]\n", what, where.c_str());
    ++failures;
  }
}

// Zipf counts, the reference's subsampling and unigram table shares, and the
// Huffman tree of the counts (word2vec's two-cursor construction: internal node
// j is created after its children, the root is V - 2).
struct Vocab {
  int64_t V;
  std::vector<int64_t> counts;
  std::vector<float> keep;
  std::vector<double> table_frac;
  std::vector<int32_t> leaf_node, node_parent;
};

Vocab make_vocab(int64_t V) {
  Vocab v;
  v.V = V;
  double total = 0.0, pow_total = 0.0;
  for (int64_t r = 0; r < V; ++r) {
    v.counts.push_back(std::max<int64_t>(1, (int64_t)(1e7 / (double)(r + 1))));
    total += (double)v.counts.back();
    pow_total += std::pow((double)v.counts.back(), 0.75);
  }
  for (int64_t r = 0; r < V; ++r) {
    const double f = (double)v.counts[(size_t)r] / total;
    v.keep.push_back((float)(std::sqrt(1e-4 / f) + 1e-4 / f));
    v.table_frac.push_back(std::pow((double)v.counts[(size_t)r], 0.75) / pow_total);
  }
  if (V < 2) return v;
  std::vector<int64_t> cnt((size_t)(2 * V - 1), (int64_t)1e15);
  std::vector<int64_t> parent((size_t)(2 * V - 1), -1);
  for (int64_t r = 0; r < V; ++r) cnt[(size_t)r] = v.counts[(size_t)r];
  int64_t pos1 = V - 1, pos2 = V;
  for (int64_t a = 0; a < V - 1; ++a) {
    int64_t m[2];
    for (int k = 0; k < 2; ++k) {
      if (pos1 >= 0 && cnt[(size_t)pos1] < cnt[(size_t)pos2]) m[k] = pos1--;
      else m[k] = pos2++;
    }
    cnt[(size_t)(V + a)] = cnt[(size_t)m[0]] + cnt[(size_t)m[1]];
    parent[(size_t)m[0]] = parent[(size_t)m[1]] = V + a;
  }
  v.leaf_node.assign((size_t)V, -1);
  v.node_parent.assign((size_t)(V - 1), -1);
  for (int64_t r = 0; r < V; ++r) v.leaf_node[(size_t)r] = (int32_t)(parent[(size_t)r] - V);
  for (int64_t j = 0; j < V - 2; ++j) v.node_parent[(size_t)j] = (int32_t)(parent[(size_t)(V + j)] - V);
  return v;
}

// One CU: 160 KiB of LDS, 32 wave slots.
int occupancy(w2v::OccKernel, int threads, int64_t lds_bytes) {
  const int64_t by_lds = lds_bytes > 0 ? 160 * 1024 / lds_bytes : 32;
  return (int)std::min<int64_t>(by_lds, 32 / std::max(1, threads / w2v::kWave));
}

bool scale_ok(float s) { return s > 0.0f && s <= 1.0f; }

void check(const w2v::PolicyInput& in, const w2v::LaunchPlan& p) {
  ++plans;
  const int64_t rows = in.hs && !p.shared ? in.V - 1 : in.V;
  expect(p.priv_n >= 0 && p.priv_n <= w2v::kPrivMax, "priv_n <= kPrivMax");
  expect(p.ctx_n >= 0 && p.ctx_n <= w2v::kCtxMax && p.ctx_n <= in.V, "ctx_n <= kCtxMax");
  expect(p.priv_lo >= 0 && (int64_t)p.priv_lo + p.priv_n <= std::max<int64_t>(rows, 0), "private rows inside the matrix");
  expect(p.hot_s >= 0 && p.hot_s <= std::max<int64_t>(in.V - 1, 0), "0 <= hot_s <= V - 1");
  expect(p.hot_wc >= 0 && p.hot_wc <= in.V, "0 <= hot_wc <= V");
  expect(p.hot_atomic >= 0 && p.hot_atomic <= in.V, "0 <= hot_atomic <= V");
  expect(p.lds_bytes >= 0 && p.lds_bytes <= 160 * 1024, "lds_bytes <= 160 KiB");
  expect(p.grid >= 1, "grid >= 1");
  const int limit = p.shared ? in.sn_waves : w2v::max_block(in.nv) / w2v::kWave;
  expect(p.wpb >= 1 && (p.wpb & (p.wpb - 1)) == 0 && p.wpb <= limit && p.threads == p.wpb * w2v::kWave,
         "wpb a power of two within the block limit");
  if (p.deep) expect(p.threads <= w2v::kDeepBlock, "deep kernel's block limit");
  for (float s : p.priv_sc) expect(scale_ok(s), "priv_sc in (0, 1]");
  for (float s : p.ctx_sc) expect(scale_ok(s), "ctx_sc in (0, 1]");
  for (float s : p.hot_sc) expect(scale_ok(s), "hot_sc in (0, 1]");
  expect(p.hot_sc.empty() || (int64_t)p.hot_sc.size() == (in.V - 1) - p.hot_s, "one scale per atomic hot node");
  expect(p.nseg >= 0 && p.nseg <= w2v::kMaxSeg, "nseg <= kMaxSeg");
  expect(in.count * std::max(1, p.nseg) <= (int64_t)UINT32_MAX - (1 << 24), "items fit the 32-bit dequeue head");
  expect(p.seg_len >= 0 && p.seg_len % w2v::kWave == 0, "seg_len a multiple of 64");
  if (p.nseg > 1) expect((int64_t)p.nseg * p.seg_len >= in.max_len, "segments cover the longest sentence");
  expect(p.flush_every >= 1 && p.ctx_flush_every >= 1, "flush intervals >= 1");
  if (in.cbow && in.window > w2v::kMaxWideWindow)
    expect(p.wide_scratch == p.grid * p.wpb * w2v::huge_stride(in.window), "an id slice per wave");
}

}  // namespace

int main() {
  struct Mode { const char* name; bool cbow, hs, shared; };
  const Mode modes[] = {{"sg_ns", false, false, false}, {"sg_hs", false, true, false}, {"cbow_ns", true, false, false},
                        {"cbow_hs", true, true, false}, {"shared", false, false, true}};
  const int64_t counts[] = {1, 100, 10000, 10000000}, max_lens[] = {1, 40, 1000, 100000};
  const w2v::Knobs knobs;
  w2v::Knobs hot_avg;
  hot_avg.hs_hot_avg = 8.0;
  for (int64_t V : {1, 2, 3, 1807, 60000, 600000}) {
    const Vocab v = make_vocab(V);
    // with statistics; without; with statistics but no tree
    w2v::RowStats st[3];
    w2v::row_stats(st[0], V, v.counts, v.keep, v.leaf_node, v.node_parent);
    st[0].table_frac = v.table_frac;
    w2v::row_stats(st[1], V, {}, {}, {}, {});
    w2v::row_stats(st[2], V, v.counts, v.keep, {}, {});
    st[2].table_frac = v.table_frac;
    expect(st[0].stats_ok && !st[1].stats_ok && st[2].stats_ok && st[2].node_f.empty(), "statistics variants");
    for (const Mode& m : modes)
      for (int nv : {1, 5, 8, 32})
        for (int ci = 0; ci < 4; ++ci)
          for (int si = 0; si < 3; ++si)
            for (int64_t cap : {0, 2048}) {
              if (m.shared && nv == 32) continue;  // no shared-negatives kernel at that pitch
              if (m.hs && V < 2) continue;         // no Huffman tree of one word
              w2v::PolicyInput in{w2v::PolicySettings{}, m.hs && si == 0 && cap == 0 ? hot_avg : knobs, st[si]};
              in.window = m.shared ? 5 : (nv == 8 ? 150 : 5);
              in.negative = m.hs ? 0 : 5;
              in.hs = m.hs; in.cbow = m.cbow;
              in.V = V; in.nv = nv; in.pitch = (int64_t)nv * w2v::kWave; in.n_cu = 256;
              in.update = m.shared ? W2V_UPDATE_SHARED_NEGATIVES : W2V_UPDATE_PER_PAIR;
              in.count = counts[ci]; in.n_sent = std::max<int64_t>(counts[ci], 10000); in.max_len = max_lens[ci];
              in.sn_waves = 2; in.max_waves = cap;
              where = std::string(m.name) + " V " + std::to_string(V) + " nv " + std::to_string(nv) + " count " +
                      std::to_string(in.count) + " stats " + std::to_string(si) + " cap " + std::to_string(cap);
              check(in, w2v::plan_launch(in, occupancy));
              if (ci == 1) {  // the sequential schedule
                in.sched = W2V_SCHED_SEQUENTIAL;
                where += " sequential";
                check(in, w2v::plan_launch(in, occupancy));
              }
            }
  }
  std::printf("policy selftest: %d plan(s), %d failure(s)\n", plans, failures);
  return failures ? 1 : 0;
}
