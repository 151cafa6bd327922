// w2v_policy.cpp — the update policy of a training launch (w2v_policy.hpp).
// Double-precision arithmetic, compiled with -ffp-contract=off: the flush
// scales are compared bit for bit against recorded plans
// (tests/test_gpu_policy.py), so the order of every expression matters.
#include "w2v_policy.hpp"

#include <algorithm>
#include <cmath>
#include <utility>

namespace w2v {

void row_stats(RowStats& s, int64_t V, const std::vector<int64_t>& tok_count, const std::vector<float>& keep,
               const std::vector<int32_t>& leaf_node, const std::vector<int32_t>& node_parent) {
  s.stats_ok = V > 0 && (int64_t)tok_count.size() == V && (int64_t)keep.size() == V;
  s.f.assign((size_t)std::max<int64_t>(V, 0), 0.0);
  s.fk.assign(s.f.size(), 0.0);
  s.node_f.clear();
  s.node_fk.clear();
  if (!s.stats_ok) return;
  double N = 0.0, K = 0.0;
  for (int64_t w = 0; w < V; ++w) {
    N += (double)tok_count[(size_t)w];
    K += (double)tok_count[(size_t)w] * std::min(1.0, (double)keep[(size_t)w]);
  }
  if (!(N > 0.0 && K > 0.0)) {
    s.stats_ok = false;
    return;
  }
  s.kept_tokens = K;
  for (int64_t w = 0; w < V; ++w) {
    s.f[(size_t)w] = (double)tok_count[(size_t)w] / N;
    s.fk[(size_t)w] = (double)tok_count[(size_t)w] * std::min(1.0, (double)keep[(size_t)w]) / K;
  }
  if ((int64_t)leaf_node.size() == V && (int64_t)node_parent.size() == V - 1) {
    s.node_f.assign((size_t)(V - 1), 0.0);
    s.node_fk.assign((size_t)(V - 1), 0.0);
    for (int64_t w = 0; w < V; ++w)
      if (leaf_node[(size_t)w] >= 0) {
        s.node_f[(size_t)leaf_node[(size_t)w]] += s.f[(size_t)w];
        s.node_fk[(size_t)leaf_node[(size_t)w]] += s.fk[(size_t)w];
      }
    for (int64_t j = 0; j < V - 1; ++j)  // a node is created after its children: ids ascend towards the root
      if (node_parent[(size_t)j] >= 0) {
        s.node_f[(size_t)node_parent[(size_t)j]] += s.node_f[(size_t)j];
        s.node_fk[(size_t)node_parent[(size_t)j]] += s.node_fk[(size_t)j];
      }
    std::vector<int32_t> depth((size_t)(V - 1), 0);  // the root (V - 2) has depth 0
    for (int64_t j = V - 3; j >= 0; --j)
      if (node_parent[(size_t)j] > j) depth[(size_t)j] = depth[(size_t)node_parent[(size_t)j]] + 1;
    s.path_len_f = s.path_len_fk = 0.0;
    for (int64_t w = 0; w < V; ++w)
      if (leaf_node[(size_t)w] >= 0) {
        const double len = 1.0 + depth[(size_t)leaf_node[(size_t)w]];
        s.path_len_f += s.f[(size_t)w] * len;
        s.path_len_fk += s.fk[(size_t)w] * len;
      }
  }
}

namespace {

double win1_of(const PolicyInput& in) { return (double)in.window + 1.0; }
bool parallel(const PolicyInput& in) { return in.sched == W2V_SCHED_PARALLEL; }

// Waves the chip holds of the per-pair kernel: 8 per SIMD for rows of <= 2
// floats per lane, else 4 (kMinWaves<NV> for every width up to 16).
int64_t chip_waves(const PolicyInput& in) { return (int64_t)in.n_cu * 4 * (in.nv <= 2 ? 8 : 4); }

// Flush scales of the privatised rows (flush_private / sn_flush_private): a
// row that n of the launch's G workgroups update within one flush interval of
// k workgroup centers gets its summed delta scaled by 1 / max(1, n / S), S =
// priv_avg. n is the EXPECTED count, G (1 - exp(-k m)), with m the row's
// expected updates per center from the corpus and vocab statistics — a fixed
// function of the row's frequency rank, so the scale does not depend on the
// schedule (the previous estimator, each workgroup's running fraction of
// flushes that found the row dirty, was noisy early in a launch). Per kept
// center, with f(w) = token share, fk(w) = kept-center share, u(w) = unigram
// table share, and window + 1 the expected number of context positions
// (Word2Vec.cpp:335-337: b = window - U[0, window-1]):
//   SG-NS output (C) rows  (window + 1) (f(r) + neg u(r))   positives are contexts (:346-349)
//   CBOW-NS output (W)     fk(r) + neg u(r)                  positive is the center (:310)
//   shared negatives (C)   fk(r) + neg u(r)                  center + the window's shared draws
//   SG-HS nodes            (window + 1) sum_{w below} f(w)   every context's path (:342-345)
//   CBOW-HS nodes          sum_{w below} fk(w)               the center's path (:304-306)
//   CBOW context (C) rows  (window + 1) f(r)                 window positions (:288-300)
// NS output rows 64..127 of the private range (private_rows > 64, or
// automatically on skip-gram NS with V >= kWidePrivVocab) flush their deltas
// scaled to at most kPrivTailAverage concurrent contributions instead of the
// top rows' 8: with 128 private rows (profiles/r05p_*: W2V_PRIV_TAIL_AVG 24 /
// 40 / 48) configs[0]'s paired gate is -0.02 / -0.61 / -1.60 analogy and the
// text8-like corpus's -9.1 / -0.21 / +1.28 similarity (the averaged flush
// damps rows 64..127 less at 40), configs[2]'s +1.40 / -0.16 at 40. Only the
// large-vocabulary rule (kWidePrivVocab) ships 128 rows by default: at 40 the
// text8-shaped corpora sit within a point of both gates, too thin a margin.
// Smaller skip-gram NS vocabularies privatised kSgNsPrivRows = 96 in round 5
// (r05r: 96 / 112 rows, configs[0] +0.02 / -0.27 analogy, text8-like
// similarity +0.77..+2.08 / -0.54..+0.52 at 40; configs[0] 316 -> 357 / 374 M
// words/s). Round 6 (VERDICT r05 "next" 5), with the gates' low ends on the
// reference band: 128 at 40 scores configs[0] -0.18 and -0.77
// analogy (the band's low end is -1.05) and the text8-like SG-NS corpus -0.19
// / +0.08 similarity against the sequential golden (profiles/r06ac_*,
// r06ad_tests.log) at 387-396 M words/s; 112 scores -0.37 / +0.38 (r06ac_*)
// at ~374 M; 96 holds configs[0] within 0.05 of the reference in every run of
// rounds 5-6 at 356 M. Below V 500 K skip-gram NS takes 112: the largest
// count that keeps configs[0] more than half a point inside its band.
// Launches smaller than the chip keep the rate limit (private_rate_for).
constexpr double kPrivTailAverage = 40.0;
constexpr int64_t kWidePrivVocab = 500000;
constexpr int64_t kSgNsPrivRows = 112;
constexpr double kCtxAvgNs = 128.0;      // CBOW-NS context rows (plan_private_rows has the measurements)
constexpr int64_t kSnPrivRowsWide = 4;  // shared negatives above negative 5 (plan_shared_negatives)
// CBOW-HS: 96 private Huffman nodes (64 context rows beside them) on
// vocabularies >= 50 K. configs[1] (V 71 K, d200: 96 + 63 rows) 426 -> 468 M
// words/s, its gate +15.9 / +5.9, text8-like CBOW-HS (V 98 K) +19.7..+22.1 /
// +13.6..+14.3 (profiles/r05al_*). On the planted corpus's small tree the
// extra nodes cost 6 similarity points at every flush average (8: -6, 4 / 2 /
// 1: -8 / -14 / -18, 40 / 128: -13 / -18; r05al_4_*, r05am_*, r05an_*), so
// small vocabularies keep 64; with fewer than 63 context rows beside them
// (d300: 96 + 31) configs[1] gained 2 % and lost similarity (r05al_1_*, _2_*).
constexpr int64_t kCbowHsPrivNodes = 96;
constexpr int64_t kWideHsVocab = 50000;
// ... and nodes 64..95 flush at up to 4 averaged contributions: at the top
// nodes' 8 the text8-like CBOW-HS gate had seeds at -5 / -8 / -9 similarity in
// two suite runs of four (r05ax_tests.log, r05ay_1_*); at 4 / 2 six seed runs
// each +10.8..+15.0 / +12.95..+13.7, configs[1] +16.6 / +6.5 (r05ay_*).
constexpr double kCbowHsTailAverage = 4.0;
// Skip-gram HS: 128 private Huffman nodes (as many as fit: 127 at d300) at up
// to 4 averaged contributions. With round 4's 64 nodes at 8 it scored 24-27
// analogy points below the sequential oracle on configs[0]'s corpus (the
// headline-scale SG-HS gate, new in round 5: every context of every center
// walks the top of the tree, and nodes 64..127 as hot atomic rows were
// Hogwild-stale); 64 nodes at 4 / 2 / 1: -21 / -17 / -13.5; 128 at 8: -4 and
// one seed at -65; 128 at 4 / 2 / 1: +2.2..+3.2 / +7..+9 / +11, each within a
// point on similarity (profiles/r05as_*, r05at_*, r05au_*, r05av_*).
// The planted corpus: +4.5 / +1.4 against +3.1 / +0.7 before. Throughput on
// configs[0]'s corpus 214 -> 309 M words/s, on configs[2]'s 44.0 -> 52.3 M
// (0.71 -> 0.85 of 8 TB/s).
constexpr double kSgHsNodeAverage = 4.0;

void priv_scales(const PolicyInput& in, LaunchPlan& p, int64_t G) {
  const RowStats& st = in.stats;
  for (int k = 0; k < kPrivMax; ++k) p.priv_sc[k] = 1.0f;
  for (int k = 0; k < kCtxMax; ++k) p.ctx_sc[k] = 1.0f;
  if (!(p.priv_avg > 0.0f) || (p.priv_n == 0 && p.ctx_n == 0)) return;
  const double S = p.priv_avg, win1 = win1_of(in), neg = (double)in.negative;
  const bool ok = st.stats_ok;
  auto sc = [&](double m, int k, double avg) {  // without statistics: every workgroup counted (the most damping)
    if (!(avg > 0.0)) return 1.0f;
    const double n = ok ? (double)G * (1.0 - std::exp(-(double)k * m)) : (double)G;
    return (float)(1.0 / std::max(1.0, n / avg));
  };
  if (p.priv_n > 0) {
    if (!p.shared && in.hs) {
      const bool nodes = ok && st.has_nodes(in.V);
      for (int k = 0; k < p.priv_n; ++k) {
        const double m = !nodes ? 1.0 : st.node_rate(p.priv_lo + k, in.cbow, win1);
        // skip-gram HS caps the average at kSgHsNodeAverage, CBOW-HS its nodes
        // past the 64th at kCbowHsTailAverage (W2V_PRIV_HS_TAIL_AVG: experiments)
        const double Sh = in.cbow ? S : std::min(S, kSgHsNodeAverage);
        const double tail = in.knobs.priv_hs_tail_avg >= 0.0 ? in.knobs.priv_hs_tail_avg
                            : in.cbow ? std::min(S, kCbowHsTailAverage) : Sh;
        const double avg = k < 64 ? Sh : tail;
        p.priv_sc[k] = sc(m, p.flush_every, avg);
      }
    } else {
      for (int k = 0; k < p.priv_n; ++k) {
        const double m = ok ? st.out_rate(p.priv_lo + k, p.shared || in.cbow, win1, neg) : 0.0;
        const double avg = k < 64 ? S : in.knobs.priv_tail_avg >= 0.0 ? in.knobs.priv_tail_avg : kPrivTailAverage;
        p.priv_sc[k] = sc(m, p.flush_every, avg);
      }
    }
  }
  // CBOW context rows: HS averages them like its nodes (S); NS at up to
  // kCtxAvgNs contributions (plan_private_rows has the measurements).
  const double Sc = in.knobs.ctx_avg >= 0.0 ? in.knobs.ctx_avg : in.hs ? S : kCtxAvgNs;
  for (int k = 0; k < p.ctx_n; ++k) p.ctx_sc[k] = sc(ok ? st.ctx_rate(k, win1) : 0.0, p.ctx_flush_every, Sc);
}

// Privatised rows by update rate (private_rate mu > 0, private_rows = -1): only
// the output rows (Huffman nodes for HS) and CBOW context rows a center
// updates at least mu times on average go to LDS. The LDS rows' averaged
// flush damps every row it holds by up to 8 / workgroups whatever its rate,
// which a row of moderate rate does not need (atomics keep its updates) and
// which under-trains it: on a 2 M-token text8-like corpus whose planted role
// words rank inside the top 64, 64 private rows give SG-NS analogy / similarity
// 62.7 / 41.2 against the oracle's 69.5 / 65.4; 8 private rows 94.0 / 72.7
// (profiles/r02q_*). Returns {output rows, context rows}.
std::pair<int64_t, int64_t> private_by_rate(const PolicyInput& in, double mu) {
  const RowStats& st = in.stats;
  if (!st.stats_ok) return {64, kCtxMax};
  const double win1 = win1_of(in), neg = (double)in.negative;
  int64_t out = 0, ctx = 0;
  if (in.hs) {
    if (st.has_nodes(in.V))
      for (int64_t j = in.V - 2; j >= 0 && out < kPrivMax; --j) {  // nodes nearest the root first
        if (st.node_rate(j, in.cbow, win1) < mu) break;
        ++out;
      }
  } else {
    for (int64_t r = 0; r < in.V && out < kPrivMax; ++r) {
      if (st.out_rate(r, in.cbow, win1, neg) < mu) break;
      ++out;
    }
  }
  for (int64_t r = 0; r < in.V && ctx < kCtxMax && in.cbow; ++r) {
    if (st.ctx_rate(r, win1) < mu) break;
    ++ctx;
  }
  return {out, ctx};
}

// The private-row rate limit a launch of `count` sentences uses (private_rate
// < 0, the default): kSmallLaunchRate when the launch has fewer sentences than
// the chip holds waves, else none. Such a launch (a small corpus, a replica's
// round slice) puts every sentence on its own wave for the whole launch, so
// every frequent row is held by thousands of waves at once and the LDS rows'
// averaged flush damps rows that do not need it: text8_small (2 M tokens,
// 2,000 sentences for 8,192 waves) CBOW-HS at full concurrency scored -9.5 /
// -18.8 against the sequential oracle with no limit and +24.4 / +18.9 at 0.1;
// SG-NS +5.3 / -0.2 and +6.1 / +5.2; the planted corpus (3,000 sentences) holds
// every gate (+10.8 / +4.8, +1.1 / +0.3, +9.7 / +0.3, +19.8 / +2.5 over the four
// modes; profiles/r03b_small_corpus.log). A launch that fills the chip keeps
// no limit: there the limit costs 20 % of throughput.
constexpr double kSmallLaunchRate = 0.1;
double private_rate_for(const PolicyInput& in, int64_t max_waves) {
  if (in.private_rate >= 0.0) return in.private_rate;
  int64_t chip = chip_waves(in);
  if (max_waves > 0) chip = std::min(chip, max_waves);
  return in.count < chip ? kSmallLaunchRate : 0.0;
}

// Waves in flight of a parallel per-pair launch (max_waves == 0: as many as
// fit, unless the vocabulary cannot take them). A kept center updates about
// T rows (skip-gram: its W row and, per context, neg + 1 NS targets and the
// context's Huffman path; CBOW: the context rows, neg + 1 targets, the
// center's path), so `waves` concurrent centers update an average row
// waves x T / V times at once. Past kPairPressure of that the Hogwild
// staleness feeds on itself: on the r04a input (window 150, negative 80, V
// 1,807: T ~ 12 K, every row ~7 times per center) skip-gram's max |W| is 115 /
// 124 / 130 / 142 at 1 / 2 / 4 / 8 waves, 667 at 16, 1e7-1e16 at 32-64 and
// non-finite from 128 up, against the sequential reference's 72-119
// (profiles/r05a_1_*, r05b_2_*, r05d_4_divergence_gpu_probe.log) — and the
// reference's own OpenMP loop reaches 1.6e5 on 8 threads
// (profiles/r05_divergence_oracle.log). The cap applies only where it is below
// the waves the launch would run (the chip's, and at most one per sentence of
// the launch): at 64 it leaves every benchmarked and gated workload as it was
// (largest: the planted corpus's SG-HS, 3,000 sentences x 66 nodes / 3.4 K
// rows = 58; configs[0] 4, configs[1] 1.2, configs[2] 0.4) and holds the
// r04a input's skip-gram at 9 waves.
constexpr double kPairPressure = 64.0;

// Hierarchical softmax on a large vocabulary (V >= kWidePrivVocab, round 6):
// no LDS-private Huffman nodes or context rows, and the waves in flight
// capped so that the root — every update's first node — has at most
// kHsRootPressure updates in flight (waves x its expected updates per kept
// center: skip-gram window + 1, one per context; CBOW 1): plain Hogwild at
// the reference's own granularity, the atomic hot nodes exact. The round-5
// policy (127 private nodes flushed as a damped mean) scored 13-19 analogy
// points BELOW the sequential reference at configs[2]'s scale (SG-HS
// -18.2 / -0.2, CBOW-HS -5.3..-13.3 / -1.1..-1.2; profiles/r05ba_*, r05be_*,
// r06a_*, r06b_*), and no damping of the nodes closes it (the hot nodes'
// deltas scaled to 64 / 16 / 4 / 1 concurrent contributions: -5.4 / +36.5 /
// +40.8 / +4.4, r06a_2_*). Without private nodes (r06a_2_*, r06b_*, r06c_*):
// SG-HS -14.9 at all 8 K waves, -5.2 / -4.2 / -0.54 at 2048 / 512 / 256;
// CBOW-HS -12.5 / -9.9 at 1024 / 256 with private context rows, +1.54 / +0.73
// at 1536 / 256 without. 256 (skip-gram) and 1536 (CBOW) waves are both
// 1536 root updates in flight. Text8-sized vocabularies keep the private
// nodes: there the same rule costs SG-HS 3 analogy points (c1hs, 256 waves:
// -2.97) and configs[1]'s CBOW-HS its throughput.
//
// Between text8's vocabulary and configs[2]'s neither policy is inside the
// reference's band (round 6, a mid-vocabulary probe golden, `mhs`: SG-HS d200,
// V 264 K; profiles/r06u_1_*, r06w_1_*, r06x_tests.log): the private-node
// policy scores +19.2 above the sequential reference (+18.8 above its 16-thread
// run), the rule -1.0..-1.2 at 256 waves and -0.6..-1.25 at 64-65 (a cap that
// scales with V, 1.5e-3 root updates in flight per word) against a band whose
// low edge is the sequential run - 1. Fewer waves do approach the reference at
// every size measured (V 71 K: -3.2 / -0.6 / -0.2 at 256 / 64 / 32 waves), at
// a cost of 10-200x the throughput there, so the rule keeps its validated
// place: V >= kWidePrivVocab, 1536 root updates in flight.
constexpr double kHsRootPressure = 1536.0;
bool wide_hs_rule(const PolicyInput& in) {
  const bool on = in.knobs.wide_hs == 1 || (in.knobs.wide_hs != 0 && in.V >= kWidePrivVocab);  // knob: 1 forces, 0 never
  return in.hs && on && parallel(in) && in.update == W2V_UPDATE_PER_PAIR;
}

int64_t effective_max_waves(const PolicyInput& in) {
  const RowStats& st = in.stats;
  if (in.max_waves > 0) return in.max_waves;
  if (!parallel(in) || in.update != W2V_UPDATE_PER_PAIR) return 0;
  if (!st.stats_ok || in.V < 2) return 0;
  const double win1 = win1_of(in), neg = (double)in.negative;
  const double ns = neg > 0.0 ? neg + 1.0 : 0.0;
  const double T = in.cbow ? win1 + ns + (in.hs ? st.path_len_fk : 0.0)
                           : 1.0 + win1 * (ns + (in.hs ? st.path_len_f : 0.0));
  if (!(T > 0.0)) return 0;
  double cap = std::floor(kPairPressure * (double)in.V / T);
  if (wide_hs_rule(in) && st.has_nodes(in.V)) {
    const double m = st.node_rate(in.V - 2, in.cbow, win1);  // the root
    if (m > 0.0) cap = std::min(cap, std::floor(kHsRootPressure / m));
  }
  // The waves the launch would run: min(chip, count) with count in sentences
  // is exact also when plan_segments cuts sentences into segments (nseg > 1),
  // because it does so only when the sentences alone fill the grid (count >=
  // the grid's waves), and then min(chip, count x nseg) = chip = min(chip,
  // count).
  return cap < (double)std::min(chip_waves(in), in.count) ? std::max<int64_t>(1, (int64_t)cap) : 0;
}

// Automatic hot rows (hot_rows == W2V_HOT_AUTO): the rows (and Huffman nodes)
// whose expected number of updates in flight across the chip, waves x their
// expected updates per center, is at least hot_tau. A row that several
// wavefronts update at once loses updates under plain read-modify-write and
// is read stale across the non-coherent XCD L2s, so those rows take
// memory-side atomics. Measured on the text8-like CBOW-HS workload (DESIGN.md
// §4.1): a fixed 1000 rows cut through the planted words' Huffman nodes
// (analogy 19.8 vs the oracle's 21.4); 2000 / 4000 / 16000 rows: 36.7 /
// 43.3 / 43.0; this rule at threshold 0.5 / 1 / 2: 42.9 / 43.7 / 44.4. At
// threshold 4 for the W / C rows the planted SG-HS run collapses (analogy
// 6 vs 89: its center rows, V = 3.4K under 8K waves, fell to plain
// read-modify-write; profiles/r02c_*). Returns {W / C rows, nodes}.
// The W / C threshold when hot_tau_rows is 0 (the default) is 1 for every
// vocabulary. Round 3 used 2 for a large vocabulary (rows' average updates in
// flight waves x (window + 1) / V <= 0.1: configs[2], 1738 -> 867 atomic rows,
// +1.1 %); round 4's paired gate at configs[2]'s own scale (d300, V 717K,
// the sequential oracle's golden, tests/test_gpu_quality.py, 2 seeds) put
// threshold 2 at -1.0 / -1.2 similarity in two leases and threshold 1 at
// +0.03 (profiles/r04b_policy_probe_c3.log), for 1.1 % of throughput
// (96.3 vs 97.4 M words/s, alternating on one box: r04c_ab_tau.log). Higher
// thresholds lost more (round 3: analogy 99.9 / 99.5 / 93.0 / 94.9 at 1 / 2
// / 4 / 16, profiles/r03w_*); at 4 the planted SG-HS run (V = 3.4K) collapsed
// (its center rows fell to plain read-modify-write: analogy 6 vs 89,
// profiles/r02c_*). The shared-negatives kernel keeps 1 too (its floor of
// 1000 atomic rows decides there).
constexpr double kHotTau = 1.0;
// Returns {W / C rows [0, rows), the `nodes` internal nodes nearest the root}
// for `waves` updaters in flight; sets p.tau_rows when the automatic rule ran.
std::pair<int64_t, int64_t> hot_for(const PolicyInput& in, LaunchPlan& p, double waves) {
  const RowStats& st = in.stats;
  const int64_t V = in.V, nV = std::max<int64_t>(V - 1, 0);
  if (in.hot_rows != W2V_HOT_AUTO) {
    if (in.hot_rows < 0) return {V, nV};
    return {std::min<int64_t>(in.hot_rows, V), std::min<int64_t>(in.hot_rows, nV)};
  }
  if (!st.stats_ok) return {std::min<int64_t>(V, 1000), std::min<int64_t>(nV, 1000)};
  const double win1 = win1_of(in), tau = in.hot_tau_rows > 0.0 ? in.hot_tau_rows : kHotTau;
  p.tau_rows = tau;
  const bool cbow = in.cbow, ns = in.negative > 0;
  int64_t rows = 0;
  for (int64_t r = 0; r < V; ++r) {  // largest rate over the row's roles in W and C
    // Positive-label updates only: an NS output row's negative-sample updates
    // (label 0, sigma(f) small for most draws) are small. Counting them put
    // 13K rows (c3) in the atomic class where these give 2.3K, for the same
    // paired scores and 2.5 % less throughput (profiles/r02b_*, r02c_*).
    double m;
    if (p.shared) m = std::max(win1 * st.fk[(size_t)r], st.fk[(size_t)r]);   // W: window inputs; C: the center
    else if (cbow) m = std::max(win1 * st.f[(size_t)r], ns ? st.fk[(size_t)r] : 0.0);  // C: contexts; W: center
    else m = std::max(st.fk[(size_t)r], ns ? win1 * st.f[(size_t)r] : 0.0);            // W: center; C: contexts
    if (waves * m >= tau) rows = r + 1;
  }
  int64_t nodes = 0;
  if (in.hs && st.has_nodes(V))
    for (int64_t j = 0; j < V - 1; ++j)
      if (waves * st.node_rate(j, cbow, win1) >= in.hot_tau_nodes) ++nodes;
  return {std::min<int64_t>(V, std::max<int64_t>(rows, 64)), nodes};
}

// Shared-negatives workgroups in flight per (vocab row / row held by a center); plan_shared_negatives.
constexpr double kSnPressure = 0.06;

// Flush interval of the HS privatised rows (auto: flush_centers == 0), in
// centers of a workgroup: the fewest of 64, 128, ..., 1024 that still gives
// every workgroup at least kHsFlushes flushes per launch (expected kept
// centers of the launch / its workgroups, from the corpus statistics); the
// context rows flush at half of it. Staleness is the model change between
// flushes, i.e. the launch's fraction between them: a long launch can flush
// less often with the same fraction, a short one (a small corpus, a
// replica's slice) keeps 64.
// Round 2 set 128 flushes per workgroup and a 256 cap (configs[1] 152 -> 173
// M words/s; the planted corpus lost 3-5 similarity points when forced to
// 256). Round 5, with the private rows' LDS adds no longer the bottleneck
// (priv_add's per-row lock), the flush atomics and the rows' write traffic are: configs[1]
// at 256 / 128 / 512 / 1024 node-interval (context at half) runs 331-341 /
// 426 / 443 M words/s (profiles/r05i_1_*, r05j_1_ab_c2_flush.log), its
// headline-scale paired gate +13.3 / +6.3, +16.4 / +6.3, +13.5 / +2.5
// (analogy / similarity against the sequential oracle, r05j_2_*): 1024 / 512
// is the fastest, but not reproducible: the same gate ran +19.3 / +6.0 in the
// next lease (both seeds moved together, profiles/r05n_tests_*), where 256 /
// 128 held +13.1..+13.7 / +5.2..+6.5 over five leases and 512 / 256 +16.4 /
// +6.3 and +17.3 / +6.45 over two. So 32 flushes per workgroup and a 1024
// cap: configs[1] (25 K kept centers per workgroup) and the text8-like corpus
// (32 K) take 512 / 256 (text8-like there: +20.0..+26.8 / +13.0..+14.1, as at
// 128 / 64, r05j_3_*), text8_small (13 K) 256 / 128 (+25.6 / +19.5,
// r05j_4_*), the planted corpus (2.4 K) keeps 64 / 32.
constexpr double kHsFlushes = 32.0;
constexpr int32_t kHsFlushMax = 1024;
int32_t auto_hs_flush(const PolicyInput& in, int64_t G) {
  if (!in.stats.stats_ok || in.n_sent <= 0 || G <= 0) return 64;
  const double cpw = in.stats.kept_tokens * ((double)in.count / (double)in.n_sent) / (double)G;
  int32_t fe = 64;
  while (fe < kHsFlushMax && 2.0 * fe * kHsFlushes <= cpw) fe *= 2;
  return fe;
}

// Atomic hot Huffman nodes (hot_s .. V - 2 below the LDS-private ones): each
// of their updates is a memory-side add computed from the node as the wave
// read it, while `waves` x m(node) other updates of the node are in flight
// (m = its expected updates per kept center: skip-gram (window + 1) x the
// token share below it, CBOW the kept-center share). With W2V_HS_HOT_AVG = S
// their deltas are scaled by 1 / max(1, waves m / S): at most S concurrent
// stale contributions, the damping the private nodes' averaged flush gives
// the nodes above them.
void hot_node_scales(const PolicyInput& in, LaunchPlan& p, double waves, int64_t nodes) {
  const RowStats& st = in.stats;
  const double S = in.knobs.hs_hot_avg >= 0.0 ? in.knobs.hs_hot_avg : 0.0;
  p.hs_hot_avg = 0.0;
  if (!in.hs || !parallel(in) || !(S > 0.0) || nodes <= 0) return;
  if (!st.stats_ok || !st.has_nodes(in.V)) return;
  const double win1 = win1_of(in);
  p.hot_sc.resize((size_t)nodes);
  for (int64_t k = 0; k < nodes; ++k)
    p.hot_sc[(size_t)k] = (float)(1.0 / std::max(1.0, waves * st.node_rate(p.hot_s + k, in.cbow, win1) / S));
  p.hs_hot_avg = S;
}

// LDS privatisation of the output layer's hottest rows (the NS target matrix
// — C for skip-gram, W for CBOW — or the top of the Huffman tree for HS)
// and, for CBOW, of the hottest context rows of C (contexts are not
// subsampled: the most frequent words sit in most windows): as many rows as
// fit 10 KiB per wave of the workgroup, <= kPrivMax per range (the dirty masks),
// the output rows first. Layout: kLdsHeaderWords in w2v_limits.hpp. Parallel
// schedule only: the reference-exact schedule keeps per-update rounding.
void plan_private_rows(const PolicyInput& in, LaunchPlan& p, int wpb, bool plain_cache) {
  const Knobs& kn = in.knobs;
  const int64_t max_waves = p.max_waves;
  const int64_t row_bytes = (int64_t)in.nv * kWave * (int64_t)sizeof(float);
  int64_t per_wave = 10 * 1024;
  if (kn.lds_per_wave > 0) per_wave = kn.lds_per_wave;  // experiments
  int64_t budget = std::min<int64_t>(160 * 1024, per_wave * (int64_t)wpb) - 4 * kLdsHeaderWords;
  if (plain_cache) {
    const int64_t n_cu = in.n_cu > 0 ? in.n_cu : 1;
    const int64_t wg_per_cu = std::max<int64_t>(1, ((max_waves + n_cu - 1) / n_cu + wpb - 1) / wpb);
    budget = 160 * 1024 / wg_per_cu - 4 * kLdsHeaderWords;
  }
  int64_t fit = budget / row_bytes;
  // <= 64 output rows by default for CBOW and HS. Skip-gram NS takes
  // kSgNsPrivRows (96), on a large vocabulary (>= kWidePrivVocab) up to 128,
  // rows past the 64th flushed with the gentler kPrivTailAverage
  // (priv_scales): 128 at the top rows' average cost 12 points of text8-like
  // similarity (the averaged flush under-trains the less contended rows);
  // at V >= 500 K rows 64..127 are function words a 50 M-token launch moves
  // constantly, in a 70-100 K vocabulary rows 96..127 are evaluation words
  // (text8: "world", "city", "states", "war"). An explicit private_rows may
  // ask for up to kPrivMax.
  // CBOW-HS on a vocabulary >= kWideHsVocab takes 96 nodes when the LDS
  // still holds 64 context rows beside them (kCbowHsPrivNodes).
  const bool sg_ns = !in.cbow && !in.hs;
  const bool wide_hs = in.cbow && in.hs && in.V >= kWideHsVocab && fit >= kCbowHsPrivNodes + kCtxMax - 1;
  const bool sg_hs = !in.cbow && in.hs;
  // Skip-gram NS rows past the 64th only on an uncapped launch: they were
  // measured (and their tail average set) with the chip's whole grid. Under a
  // wave cap that leaves 16- or 8-wave workgroups but fewer of them, the
  // top rows' flush scale (priv_scales: per launch workgroup) doubles, and
  // together with the tail rows configs[0]'s corpus collapsed: 2048 / 4096
  // waves -41.0 / -68.7 analogy against the sequential golden, 64 rows at the
  // same caps -0.09 / +0.12, the uncapped launch at 112 rows -0.29
  // (profiles/r06ai_c1_probe.log, r06aj_*, r06ak_*).
  const bool tail_ok = max_waves <= 0;
  const int64_t auto_rows = sg_hs ? kPrivMax
                            : !sg_ns ? (wide_hs ? kCbowHsPrivNodes : 64)
                            : !tail_ok ? 64
                                     : in.V >= kWidePrivVocab ? kPrivMax : kSgNsPrivRows;
  const bool plain_hs = wide_hs_rule(in);  // large-vocabulary HS: no LDS-private nodes / context rows
  int64_t P = std::min<int64_t>(fit, in.private_rows > 0 || plain_cache ? kPrivMax : plain_hs ? 0 : auto_rows);
  if (in.private_rows >= 0) P = std::min<int64_t>(P, in.private_rows);
  const int64_t avail = in.hs ? in.V - 1 : in.V;
  if (P > avail) P = avail;
  std::pair<int64_t, int64_t> by_rate{P, kCtxMax};
  const double rate = private_rate_for(in, max_waves);
  p.private_rate = rate;
  if (rate > 0.0) {
    by_rate = private_by_rate(in, rate);
    if (in.private_rows < 0) P = std::min(P, by_rate.first);
  }
  if (P > 0) {
    p.priv_lo = (int32_t)(in.hs ? avail - P : 0);  // HS: the P internal nodes nearest the root (V-2)
    p.priv_n = (int32_t)P;
    if (plain_cache) {  // a write-combining cache: summed, flushed after every center of a wave
      p.priv_avg = 0.0f;
      if (in.flush_centers <= 0) p.flush_every = wpb;
    }
  }
  // Auto for CBOW. It doubles CBOW-HS throughput and raises its planted-
  // corpus scores. CBOW-NS (hot rows privatised on both sides of every dot
  // product) failed the similarity gate at every flush interval while its
  // context rows were averaged like the output rows (profiles/r01_context_rows.log;
  // round 5, 8 averaged contributions at 256 / 64 / 32 / 16 centers: planted
  // similarity -45 / -37 / -20 / -2.6, r05t_2_*). With up to kCtxAvgNs = 128
  // contributions (priv_scales) at 256 centers it scores as the atomic context
  // rows do: planted +2.6 / +0.2 (r05u_2_*), configs[1]'s corpus +3.0..+3.5 /
  // +3.0..+3.6 against +3.2..+3.7 / +3.2..+3.4 (three runs each,
  // r05w_*_policy_probe.log); 32 / 64 over-train the planted analogy (+41 / +21),
  // a plain sum is noisy there (per seed -4.4..+5.3 similarity). It runs 4.6x
  // the atomic context rows on configs[2]'s corpus (50.5 -> 232 M words/s)
  // and 5.8x on configs[1]'s at d200 / negative 5 (106 -> 613 M; r05v_2_*, r05v_3_*).
  int64_t Q = in.cbow ? std::min<int64_t>({fit - P, (int64_t)kCtxMax, in.V}) : 0;
  if (in.context_rows >= 0) Q = std::min<int64_t>(Q, in.context_rows);
  else if (plain_hs) Q = 0;
  else if (rate > 0.0) Q = std::min(Q, by_rate.second);
  if (Q > 0) p.ctx_n = (int32_t)Q;
  if (P + Q > 0) p.lds_bytes = kLdsHeaderWords * (int64_t)sizeof(float) + (P + Q) * row_bytes;
}

// Sentence segments as work items (parallel Philox schedule): the launch's
// last round shrinks from a whole sentence per wave to one segment. With
// ~1000-token sentences and a few thousand resident waves, whole sentences
// leave most of the chip idle for the last ~1/rounds of the launch. Only
// when the sentences alone fill the grid: segments must not raise the
// number of waves training at once (a small corpus would train its
// frequent rows from more waves at once than whole sentences do; the
// planted CBOW-HS gate loses 3.6 points of similarity that way).
void plan_segments(const PolicyInput& in, LaunchPlan& p) {
  p.nseg = 1;
  p.seg_len = 0;
  if (!parallel(in) || in.rng != W2V_RNG_PHILOX || in.count < p.grid * p.wpb) return;
  int64_t seg = kSegLen;
  if (in.knobs.seg_len >= 0) seg = in.knobs.seg_len;  // experiments; 0 = whole sentences
  if (seg <= 0) return;
  seg = (seg + kWave - 1) / kWave * kWave;
  int64_t nseg = (in.max_len + seg - 1) / seg;
  if (nseg > kMaxSeg) nseg = kMaxSeg;  // very long sentences: longer segments, not more
  // the dequeue head is 32-bit: items plus one extra dequeue per wave
  while (nseg > 1 && in.count * nseg > (int64_t)UINT32_MAX - (1 << 24)) --nseg;
  if (nseg > 1) {
    p.nseg = (int32_t)nseg;
    p.seg_len = (int32_t)(((in.max_len + nseg - 1) / nseg + kWave - 1) / kWave * kWave);
  }
}

}  // namespace

LaunchPlan plan_per_pair(const PolicyInput& in, const Occupancy& occupancy) {
  const Knobs& kn = in.knobs;
  LaunchPlan p;
  // Workgroup shape: up to 16 waves share the LDS-privatised rows (kMaxBlock);
  // under a wave cap, narrower workgroups so the capped grid still spans the CUs.
  const int max_wpb = max_block(in.nv) / kWave;
  int wpb = max_wpb;
  if (kn.wpb > 0) wpb = std::min(max_wpb, kn.wpb);  // experiments
  const int64_t max_waves = effective_max_waves(in);
  p.max_waves = max_waves;
  p.wave_cap = in.max_waves > 0 ? 0 : max_waves;
  if (max_waves > 0) {
    int64_t per = max_waves / (in.n_cu > 0 ? in.n_cu : 1);
    wpb = 1;
    while (wpb * 2 <= max_wpb && wpb * 2 <= per) wpb *= 2;
  }
  // The low-occupancy deep-pipeline kernel (train_epoch_deep_kernel) for a
  // capped HS launch (<= 4 waves per workgroup; W2V_DEEP_HS=1 forces it for
  // any HS launch without negatives, sequential schedules included: parity
  // tests; 0 never)
  const bool deep_ok = in.hs && in.negative <= 0 && in.rng != W2V_RNG_REPLAY && in.nv <= 12 &&
                       !(in.cbow && 2 * in.window + 1 > kWave);
  p.deep = deep_ok && (kn.deep_hs == 1 || (kn.deep_hs != 0 && parallel(in) && max_waves > 0 && wpb * kWave <= kDeepBlock));
  if (p.deep) wpb = std::min(wpb, kDeepBlock / kWave);
  // Flush interval of the privatised rows, in centers of the workgroup (about
  // 64 centers per wave for NS, 4 per wave for HS whose top nodes every
  // update touches), and the averaging of their deltas (flush_private). A
  // flush stalls the flushing wave (its later loads wait for its atomics,
  // vmcnt is in order) behind every other workgroup's atomics on the same
  // rows: CBOW-HS runs 105 / 122 / 141 M words/s at 16 / 32 / 64, SG-NS d300
  // 78 / 90 / 96 M at 64 / 256 / 1024, with the gates passing throughout
  // (profiles/r01_hs_flush.log, profiles/r01_ns_flush.log).
  p.flush_every = in.flush_centers > 0 ? in.flush_centers : (in.hs ? 64 : 1024);
  p.ctx_flush_every = in.context_flush > 0 ? in.context_flush : (in.hs ? 32 : 256);
  p.priv_avg = in.private_average;
  // Large-vocabulary HS (wide_hs_rule) under its wave cap: the top Huffman
  // nodes in LDS as a write-combining cache, not a damped average — the
  // workgroup's waves read node + pending delta (each wave's own updates stay
  // visible to it, as the reference's thread sees its own), and the pending
  // deltas are added to HBM as a plain SUM after every center of a wave
  // (flush_every = waves per workgroup). Every node a wave's path visits is
  // updated once per center in HBM instead of once per context: SG-HS at
  // configs[2]'s scale -0.66 / +0.11 against the sequential golden at ~2x the
  // speed (profiles/r06p_1_*; a flush every 8 centers -1.54 / -0.06). The
  // cap's waves per CU decide the LDS budget (1 workgroup per CU for
  // skip-gram's 256 waves: 127 nodes at d300). Skip-gram only: CBOW-HS's 1536
  // waves share a cache four waves to a workgroup, and with it configs[2]'s
  // corpus scored -0.16..-0.62 against the sequential golden in two runs
  // (38.5 M words/s, 2x) and DIVERGED in the third (profiles/r06q_*, r06r_*).
  const bool plain_cache = wide_hs_rule(in) && !in.cbow && in.private_rows < 0 && max_waves > 0;
  int64_t resident_waves = 1, resident_wg = 1, uncapped_wg = 1;
  if (parallel(in)) {
    plan_private_rows(in, p, wpb, plain_cache);
    p.threads = wpb * kWave;
    p.wpb = wpb;
    // (the write-combining node cache of a capped HS launch does not change
    // which nodes the chip's waves contend on: its hot set is counted as
    // without the cache, the set its quality was measured with: the hot-row
    // rule counts the regular kernel's residency)
    const int per_cu = std::max(1, occupancy(p.deep ? kOccTrainDeep : kOccTrain, p.threads, p.lds_bytes));
    const int per_cu_occ = std::max(1, occupancy(kOccTrain, p.threads, plain_cache ? 0 : p.lds_bytes));
    const int64_t resident = (int64_t)per_cu * in.n_cu;
    resident_waves = (int64_t)per_cu_occ * in.n_cu * (max_wpb);
    resident_wg = resident;
    // the workgroups of max_wpb waves the launch would run without its cap
    uncapped_wg = std::min<int64_t>((in.count + max_wpb - 1) / max_wpb, (int64_t)per_cu_occ * wpb * in.n_cu / max_wpb);
    const int64_t need = (in.count + wpb - 1) / wpb;
    int64_t g = need < resident ? need : resident;
    if (max_waves > 0 && (max_waves + wpb - 1) / wpb < g) g = (max_waves + wpb - 1) / wpb;
    if (kn.max_blocks > 0 && kn.max_blocks < g) g = kn.max_blocks;  // diagnostics only
    p.grid = g;
  }
  // The rule counts every wave the chip could run, not this launch's grid:
  // a small launch (a round's slice, a wave cap) still spreads over the XCDs,
  // whose L2s keep stale copies of the rows they read however few waves run
  // (measured: two replicas on one GPU trained in 1/8-epoch slices collapsed
  // to analogy 3 with the launch-grid count; tests/test_gpu_replicas.py).
  const std::pair<int64_t, int64_t> hot = hot_for(in, p, (double)resident_waves);
  p.hot_wc = (int32_t)hot.first;
  p.hot_s = (int32_t)((in.V - 1) - hot.second);  // the `nodes` internal nodes nearest the root (the root is V-2)
  p.hot_rows = hot.first;
  p.hot_nodes = in.hs ? hot.second : 0;
  hot_node_scales(in, p, (double)resident_waves, hot.second);
  plan_segments(in, p);
  // Flush scales from the launch's own grid (the workgroups that actually
  // race). Counting the chip's resident workgroups instead (W2V_SCALE_RESIDENT)
  // helps small launches (CBOW-HS in 16 slices per epoch, text8-like: analogy
  // 24.5 vs 12.2) but over-damps a corpus with fewer sentences than the chip
  // holds waves (planted CBOW-HS: similarity -13 vs the oracle; profiles/r02l_*, r02r_*).
  // A wave cap that keeps the uncapped launch's workgroup shape runs fewer of
  // its workgroups; the flush interval and scales then count the uncapped
  // launch's workgroups, the ones they were measured with. Counted from the
  // capped grid, c1hs (SG-HS, configs[0]'s corpus) at 4096 waves collapsed to
  // -43.9 analogy against the sequential golden (the uncapped launch +2.8),
  // counted this way +17.7 (profiles/r06al_c1hs_probe.log, r06an_*). Narrower
  // workgroups keep their own grid: at 2048 waves (8-wave workgroups) the
  // uncapped count moved configs[1]'s corpus from -1.7 to -4.2, and one wave's
  // flush must stay its own exact sum.
  int64_t g_flush = p.grid;
  if (max_waves > 0 && wpb == max_wpb && parallel(in)) g_flush = std::max(g_flush, uncapped_wg);
  if (parallel(in) && in.hs && p.priv_n + p.ctx_n > 0 && !plain_cache) {
    const int32_t fe = auto_hs_flush(in, g_flush);
    if (in.flush_centers <= 0) p.flush_every = fe;
    if (in.context_flush <= 0) p.ctx_flush_every = std::max<int32_t>(1, fe / 2);
  }
  priv_scales(in, p, kn.scale_resident ? resident_wg : g_flush);
  if (in.cbow && in.window > kMaxWideWindow) {  // cbow_center_huge: one id slice per wave
    p.wide_stride = huge_stride(in.window);
    p.wide_scratch = p.grid * p.wpb * p.wide_stride;
  }
  return p;
}

// The shared-negatives minibatch: 2-wave workgroups, static LDS.
LaunchPlan plan_shared_negatives(const PolicyInput& in, const Occupancy& occupancy) {
  const Knobs& kn = in.knobs;
  LaunchPlan p;
  p.shared = true;
  p.max_waves = in.max_waves;
  p.priv_avg = in.private_average;
  p.ctx_flush_every = in.context_flush > 0 ? in.context_flush : 256;  // not read by this kernel
  if (parallel(in)) p.private_rate = private_rate_for(in, in.max_waves);
  // LDS row slots (kSnPriv in w2v_shared.hpp: 20 KiB of rows, <= 32), parallel
  // schedule only. The first priv_n hold the workgroup's pending deltas of
  // the hottest C rows, added to HBM with atomics every flush_centers centers
  // (auto: up to 10, every 1024 centers); the rest stage the atomic rows'
  // deltas of each center. Measured on configs[4]: 4 private rows + staged
  // atomics 72 M words/s vs 61 M with neither, and higher planted /
  // text8-like scores (profiles/r01_sn_atomic_rows.log); private rows in
  // every slot run faster still with the same scores: of 8 slots, 8 private
  // rows +4 % over 4 + 4 staging; of 10 slots (single transpose buffer), 10
  // private +3.8 % over 4 (profiles/r02z_priv.log, r02z_c5_slots10.log,
  // r02z_sn_quality_probe*.log). Those measurements are at negative 5. At
  // configs[4]'s own negative 15 every center draws three times as many of
  // the hottest C rows, a workgroup's 1024-center pending delta of them is
  // three times as stale, and the averaged flush costs the text8-like gate 8
  // similarity points (90.7-91.6 / 62.8-65.1 with 2-32 averaged contributions
  // against 98.1 / 72.2 with no private rows, the sequential minibatch
  // scoring 98.3 / 69.7: profiles/r03q_c5_*.log). Round 5 (configs[4]'s
  // paired gate against the sequential minibatch, 3 seeds per run): 10 rows
  // fail at every average (1-8: -0.9..-2.1 / -1.7..-5.4; 128 and the plain
  // sum diverge), 2 / 4 / 6 rows at 4 or 8 pass in every run (4 at 8: +0.16..
  // +0.45 / +0.27..+1.06 in three; at 4: -0.01..+0.26 / -0.67..+1.30 in five;
  // the configuration without them +0.04..+0.34 / -0.71..+0.84) and run
  // 71.7 / 73.2 / 74.0 M words/s against 66.7 M (profiles/r05y_*, r05z_*,
  // r05aa_*). Above negative 5 the automatic setting keeps 4 private rows
  // (the other slots stage atomic rows) — for a handle that trains alone:
  // two replicas summed by the exchange then lose -0.6 / -2.2 analogy on
  // the 400 M-token replica gate (r05ab_tests.log, r05ad_tests.log; the
  // rows' divisor assumes one replica's concurrency), so replicas keep none.
  const int64_t slots = std::min<int64_t>(32, kSnPrivBytes / (in.pitch * (int64_t)sizeof(float)));
  const int64_t wide = in.replicas > 1 ? 0 : kSnPrivRowsWide;
  const int64_t want = in.private_rows < 0 ? std::min<int64_t>(in.negative <= 5 ? 10 : wide, slots) : in.private_rows;
  p.priv_n = parallel(in) ? (int32_t)std::min<int64_t>({slots, in.V, want}) : 0;
  p.flush_every = in.flush_centers > 0 ? in.flush_centers : 1024;
  p.threads = in.sn_waves * kWave;
  p.wpb = in.sn_waves;
  // device-coherent rows (rows_rsrc in w2v_shared.hpp): all for hot_rows =
  // -1, else at least the rows two XCD L2s' capacity could keep resident
  const int64_t l2_rows = (int64_t)(8 << 20) / (in.pitch * (int64_t)sizeof(float));
  int64_t g = 1, g_res = 1;
  if (parallel(in)) {
    int per_cu = std::max(1, occupancy(kOccSharedNeg, p.threads, 0));
    // Concurrency a vocab can take: every center holds its 2 window + negative
    // + 1 rows for its whole update, so a small vocab's frequent rows are held
    // by hundreds of workgroups at once. Workgroups in flight are capped at
    // kSnPressure x V / (rows per center) (at least one per CU). Measured on
    // the text8-like gate corpus (V 98K, d512, negative 15, window 5: 26 rows;
    // the paired gate against the sequential minibatch, 3 seeds, two runs
    // each, profiles/r05a_2_policy_probe.log): 2 workgroups per CU -1.06 /
    // +2.57 and -0.78 / +3.00 (analogy / similarity), 1 per CU +0.40 / +0.66
    // and +0.36 / +0.04. The cap allows 0.06 x 98K / 26 = 226 workgroups there
    // (-> 1 per CU) and leaves configs[4]'s V 740K at full occupancy (4 per CU:
    // 1708). Round 1 measured quality holding at 1 per CU for V 3.4K and
    // collapsing at 4 for V 98K (profiles/r01_sn_residency_experiment.log).
    if (in.max_waves == 0) {
      const double rows = 2.0 * in.window + in.negative + 1.0;
      const double cap = kSnPressure * (double)in.V / rows / (double)std::max(1, in.n_cu);
      per_cu = std::max(1, std::min(per_cu, (int)cap));
    }
    if (kn.sn_per_cu > 0) per_cu = std::min(per_cu, kn.sn_per_cu);  // experiments
    g_res = (int64_t)per_cu * in.n_cu;
    g = std::min<int64_t>(g_res, in.count);
    if (in.max_waves > 0) g = std::max<int64_t>(1, std::min<int64_t>(g, in.max_waves / in.sn_waves));
  }
  p.grid = g;
  // the hot rows (one updater per workgroup) take atomic deltas, as in the
  // per-pair kernel (parallel schedule only: the sequential one is exact
  // either way), and at least the rows two XCD L2s could keep resident are
  // device-coherent
  // (automatic: at least the fixed 1000 rows of round 1 — a shared-negatives
  // center holds its ~22 rows for its whole update, longer than a per-pair
  // update holds one, and the rate rule alone left the text8-like gate 2.4
  // similarity points below the oracle; profiles/r02s_gpu_tests.log)
  int64_t hot = hot_for(in, p, (double)g_res).first;
  if (in.hot_rows == W2V_HOT_AUTO) hot = std::max<int64_t>(hot, std::min<int64_t>(in.V, 1000));
  p.hot_wc = (int32_t)(in.hot_rows == -1 ? in.V : std::min<int64_t>(in.V, std::max<int64_t>(hot, l2_rows)));
  if (kn.sn_coherent_rows >= 0) p.hot_wc = (int32_t)std::min<int64_t>(in.V, kn.sn_coherent_rows);  // experiments
  p.hot_atomic = parallel(in) ? hot : 0;
  if (kn.sn_atomic_rows >= 0) p.hot_atomic = std::min<int64_t>(in.V, kn.sn_atomic_rows);  // experiments
  p.hot_rows = p.hot_atomic;
  priv_scales(in, p, kn.scale_resident ? g_res : g);
  return p;
}

}  // namespace w2v
