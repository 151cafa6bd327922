// word2vec — command-line driver with the reference CLI's flags, defaults and
// validation (/root/reference/main.cpp:94-204), training on an MI355X.
//
// Kept as in the reference: the defaults of main.cpp:105-121 (not those of the
// help text), the hs/ns validation (:164-178), init_alpha forced to 0.05
// because cbow_mean is hard-wired true (:117,180-181), min_alpha derived from
// the pre-override 0.025 (:116), 1000-token sentences (:66), and which matrix
// is written (:196-201). Additive: -train is honoured (the reference always
// reads ./text8), -binary, -gpu, -replay, -shared-negatives, and the
// multi-GPU flags -gpus, -sync-words, -overlap, -replica-mode (Word2Vec::gpu_devices), -gpu-ingest,
// -classes (in the reference's help text, never parsed by its main),
// -phrase / -phrase-min-count (word2phrase passes before the vocabulary), and
// -score / -score-output (the trained model's log-likelihood of a text).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "Word2Vec.h"

namespace {

void usage() {
  std::cout << "word2vec (MI355X) — skip-gram / CBOW with negative sampling or hierarchical softmax\n\n"
               "  -train <file>         training text (default: ./text8)\n"
               "  -output <file>        word vectors to write (default: text8-sgns.txt)\n"
               "  -size <int>           vector dimension (default 200)\n"
               "  -window <int>         max context distance (default 5)\n"
               "  -subsample <float>    frequent-word down-sampling threshold (default 1e-4)\n"
               "  -train_method <hs|ns> hierarchical softmax or negative sampling (default ns)\n"
               "  -negative <int>       negatives per target (default 0; required > 0 for ns)\n"
               "  -threads <int>        host threads (kept for compatibility; default 1)\n"
               "  -iter <int>           epochs (default 1)\n"
               "  -min-count <int>      drop words rarer than this (default 5)\n"
               "  -alpha <float>        accepted, but the start rate is 0.05 (cbow_mean is always on)\n"
               "  -save-vocab <file>    write the vocabulary\n"
               "  -read-vocab <file>    accepted, unused (as in the reference CLI)\n"
               "  -model <cbow|sg>      architecture (default sg)\n"
               "  -binary <0|1>         write vectors in the binary layout (default 0)\n"
               "  -gpu <int>            HIP device (default 0)\n"
               "  -replay <0|1>         reference-exact deterministic RNG replay on one wavefront\n"
               "  -shared-negatives <0|1> skip-gram NS as the shared-negatives minibatch on the matrix cores\n"
               "  -gpus <int>           data-parallel replicas on devices gpu .. gpu+n-1, averaged with RCCL (default 1)\n"
               "  -sync-words <int>     exchange the replicas' updates every this many words of a shard\n"
               "                        (default 0: 64 exchanges per epoch)\n"
               "  -overlap <0|1>        overlap the averaging with the next round's training (default 1)\n"
               "  -replica-mode <auto|sum|average|row_average|adaptive> how the replicas' updates combine\n"
               "                        (default auto: average for <= 4 replicas of >= 256 M words each, else sum for 2, adaptive for more)\n"
               "  -gpu-ingest <0|1>     count and map the corpus on the GPU (default 0: host threads)\n"
               "  -classes <int>        output word classes rather than word vectors: k-means over the vectors on the\n"
               "                        GPU, one \"word class\" line per word (default 0: vectors are written)\n"
               "  -phrase <t1[,t2...]>  join word pairs into phrases (new_york) on the GPU before training: one word2phrase\n"
               "                        pass per comma-separated threshold >= 0, e.g. 200,100 (default: off)\n"
               "  -phrase-min-count <int> words and pairs rarer than this never join (default 5)\n"
               "  -score <file>         after training, score this text (read as -train is) under the model on the GPU and\n"
               "                        print its sentences, targets, log-likelihood and log-likelihood per target\n"
               "  -score-output <file>  with -score: one \"log-likelihood targets\" line per sentence\n\n"
               "example: ./word2vec -train text8 -output vec.txt -size 300 -window 5 -subsample 1e-4 "
               "-negative 5 -model sg -train_method ns -iter 3\n";
}

int find_flag(const char* name, int argc, char** argv) {
  for (int i = 1; i < argc; ++i)
    if (!std::strcmp(name, argv[i])) {
      if (i == argc - 1) {
        std::printf("Argument missing for %s\n", name);
        std::exit(1);
      }
      return i;
    }
  return -1;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 1) {
    usage();
    return 0;
  }
  std::string input_file = "", output_file = "text8-sgns.txt", save_vocab_file = "", read_vocab_file = "";
  std::string model = "sg", train_method = "ns";
  int table_size = 100000000, word_dim = 200, window = 5, negative = 0, num_threads = 1, iter = 1, min_count = 5;
  float init_alpha = 0.025f, subsample_threshold = 0.0001f;
  const float min_alpha = init_alpha * 0.0001;
  const bool cbow_mean = true;
  int binary = 0, gpu = 0, replay = 0, shared = 0, gpus = 1, overlap = 1, gpu_ingest = 0, classes = 0;
  long long sync_words = 0;
  std::string replica_mode = "auto";
  int i;
  if ((i = find_flag("-size", argc, argv)) > 0) word_dim = std::atoi(argv[i + 1]);
  if ((i = find_flag("-train", argc, argv)) > 0) input_file = argv[i + 1];
  if ((i = find_flag("-save-vocab", argc, argv)) > 0) save_vocab_file = argv[i + 1];
  if ((i = find_flag("-read-vocab", argc, argv)) > 0) read_vocab_file = argv[i + 1];
  if ((i = find_flag("-model", argc, argv)) > 0) model = argv[i + 1];
  if ((i = find_flag("-alpha", argc, argv)) > 0) init_alpha = (float)std::atof(argv[i + 1]);
  if ((i = find_flag("-output", argc, argv)) > 0) output_file = argv[i + 1];
  if ((i = find_flag("-window", argc, argv)) > 0) window = std::atoi(argv[i + 1]);
  if ((i = find_flag("-subsample", argc, argv)) > 0) subsample_threshold = (float)std::atof(argv[i + 1]);
  if ((i = find_flag("-train_method", argc, argv)) > 0) train_method = argv[i + 1];
  if ((i = find_flag("-negative", argc, argv)) > 0) negative = std::atoi(argv[i + 1]);
  if ((i = find_flag("-threads", argc, argv)) > 0) num_threads = std::atoi(argv[i + 1]);
  if ((i = find_flag("-iter", argc, argv)) > 0) iter = std::atoi(argv[i + 1]);
  if ((i = find_flag("-min-count", argc, argv)) > 0) min_count = std::atoi(argv[i + 1]);
  if ((i = find_flag("-binary", argc, argv)) > 0) binary = std::atoi(argv[i + 1]);
  if ((i = find_flag("-gpu", argc, argv)) > 0) gpu = std::atoi(argv[i + 1]);
  if ((i = find_flag("-replay", argc, argv)) > 0) replay = std::atoi(argv[i + 1]);
  if ((i = find_flag("-shared-negatives", argc, argv)) > 0) shared = std::atoi(argv[i + 1]);
  if ((i = find_flag("-gpus", argc, argv)) > 0) gpus = std::atoi(argv[i + 1]);
  if ((i = find_flag("-sync-words", argc, argv)) > 0) sync_words = std::atoll(argv[i + 1]);
  if ((i = find_flag("-overlap", argc, argv)) > 0) overlap = std::atoi(argv[i + 1]);
  if ((i = find_flag("-replica-mode", argc, argv)) > 0) replica_mode = argv[i + 1];
  if ((i = find_flag("-gpu-ingest", argc, argv)) > 0) gpu_ingest = std::atoi(argv[i + 1]);
  if ((i = find_flag("-classes", argc, argv)) > 0) classes = std::atoi(argv[i + 1]);
  std::string score_file = "", score_output = "";
  if ((i = find_flag("-score", argc, argv)) > 0) score_file = argv[i + 1];
  if ((i = find_flag("-score-output", argc, argv)) > 0) score_output = argv[i + 1];
  if (score_file.empty() && !score_output.empty()) {
    std::cout << "Please set -score with -score-output!" << std::endl;
    return 1;
  }
  std::vector<float> phrase_thresholds;
  int phrase_min_count = 5;
  bool phrase_ok = true;
  if ((i = find_flag("-phrase", argc, argv)) > 0) {
    const std::string list = argv[i + 1];
    size_t b = 0;
    while (b <= list.size()) {  // comma-separated, every piece a finite float >= 0
      const size_t e = std::min(list.find(',', b), list.size());
      const std::string piece = list.substr(b, e - b);
      char* end = nullptr;
      const float t = std::strtof(piece.c_str(), &end);
      if (piece.empty() || *end != '\0' || !(t >= 0.0f) || t > 3.0e38f) phrase_ok = false;
      phrase_thresholds.push_back(t);
      b = e + 1;
    }
  }
  if ((i = find_flag("-phrase-min-count", argc, argv)) > 0) phrase_min_count = std::atoi(argv[i + 1]);
  if (!phrase_ok || phrase_min_count < 1) {
    std::cout << "Please set -phrase to comma-separated thresholds >= 0 and -phrase-min-count >= 1!" << std::endl;
    return 1;
  }
  if (classes < 0) {
    std::cout << "Please set -classes >= 0!" << std::endl;
    return 1;
  }
  if (gpus < 1 || sync_words < 0) {
    std::cout << "Please set -gpus >= 1 and -sync-words >= 0!" << std::endl;
    return 1;
  }
  int replica_mode_id = -1;
  {
    const char* names[] = {"sum", "average", "row_average", "adaptive"};
    for (int k = 0; k < 4; ++k)
      if (replica_mode == names[k]) replica_mode_id = k;  // W2V_GROUP_SUM .. W2V_GROUP_ADAPTIVE
  }
  if (replica_mode_id < 0 && replica_mode != "auto") {
    std::cout << "Please set -replica-mode to auto, sum, average, row_average or adaptive!" << std::endl;
    return 1;
  }

  if (model.empty()) {
    model = "sg";
    std::cout << "Default use skip gram model" << std::endl;
  }
  if (train_method.empty()) {
    train_method = "ns";
    std::cout << "Default use negative sampling model" << std::endl;
  }
  if (train_method == "ns" && negative <= 0) {
    std::cout << "Please set -negative > 0!" << std::endl;
    return 1;
  }
  if (train_method == "hs" && negative > 0) {
    std::cout << "Do not set -negative under hierarchical softmax!" << std::endl;
    return 1;
  }
  if (train_method == "hs" && model.find("align") != std::string::npos) {
    std::cout << "Please use negative sampling in aligned skip gram model!" << std::endl;
    return 1;
  }
  {  // the GPU kernels' range (w2v_dev_limits); the reference accepts any value
    int32_t md = 0, mw = 0, mn = 0, smw = 0, smn = 0;
    w2v_dev_limits(&md, &mw, &mn, &smw, &smn);
    if (word_dim < 1 || word_dim > md) {
      std::cout << "Please set -size in [1, " << md << "] (the GPU kernels' range)!" << std::endl;
      return 1;
    }
    if (window < 0 || window > mw) {
      std::cout << "Please set -window in [0, " << mw << "] (the GPU kernels' range)!" << std::endl;
      return 1;
    }
    if (negative > mn) {
      std::cout << "Please set -negative <= " << mn << " (the GPU kernels' range)!" << std::endl;
      return 1;
    }
    int32_t cw = 0, cn = 0;
    w2v_dev_score_limits(nullptr, &cw, &cn);
    if (!score_file.empty() && (window > cw || negative > cn)) {
      std::cout << "Please set -window <= " << cw << " and -negative <= " << cn << " with -score!" << std::endl;
      return 1;
    }
    int32_t sdim = 0;
    w2v_dev_shared_limits(&sdim, nullptr, nullptr);
    if (shared && (window > smw || negative > smn || word_dim > sdim)) {
      std::cout << "Please set -window <= " << smw << ", -negative <= " << smn << " and -size <= " << sdim
                << " with -shared-negatives 1!" << std::endl;
      return 1;
    }
  }
  if (cbow_mean) init_alpha = 0.05f;

  Word2Vec w2v(iter, window, min_count, table_size, word_dim, negative, subsample_threshold, init_alpha,
               min_alpha, cbow_mean, num_threads, train_method, model);
  w2v.gpu_device = gpu;
  w2v.replay_rng = replay != 0;
  w2v.shared_negatives = shared != 0;
  if (gpus > 1)
    for (int k = 0; k < gpus; ++k) w2v.gpu_devices.push_back(gpu + k);
  w2v.sync_words = sync_words;
  w2v.overlap_average = overlap != 0;
  w2v.replica_mode = replica_mode_id;
  w2v.gpu_ingest = gpu_ingest != 0;
  if (!phrase_thresholds.empty()) {
    w2v.phrase = true;
    w2v.phrase_thresholds = phrase_thresholds;
    w2v.phrase_min_count = phrase_min_count;
  }
  // main.cpp:63-92's reader (1000-token sentences), streamed from the mapped
  // file by host threads: the same vocabulary and samples as building
  // vector<vector<string>> first (Word2Vec::build_vocab_file / train_file)
  const std::string corpus = input_file.empty() ? "text8" : input_file;
  try {
    w2v.build_vocab_file(corpus, "text8");
  } catch (const std::exception& e) {
    std::cerr << e.what() << std::endl;
    return 1;
  }
  w2v.init_weights(w2v.vocab.size());
  if (!save_vocab_file.empty()) w2v.save_vocab(save_vocab_file);
  try {
    w2v.train_file(corpus, "text8");
  } catch (const std::exception& e) {
    std::cerr << e.what() << std::endl;
    return 2;
  }
  if (!output_file.empty()) {
    const RMatrixXf& out = (train_method == "hs" && model == "cbow") ? w2v.C : w2v.W;
    if (classes > 0) {
      try {
        w2v.save_classes(output_file, out, classes);
      } catch (const std::exception& e) {
        std::cerr << e.what() << std::endl;
        return 2;
      }
    } else {
      w2v.save_word2vec(output_file, out, binary != 0);
    }
  }
  if (!score_file.empty()) {
    try {
      std::vector<double> ll;
      std::vector<int64_t> targets;
      const double total = w2v.score_file(score_file, "text8", 0, &ll, &targets);
      const w2v_score_summary& sm = w2v.last_score;
      std::printf("score: sentences %lld targets %lld ll %.17g ll_per_target %.17g\n", (long long)sm.sentences,
                  (long long)sm.targets, total, sm.targets > 0 ? total / (double)sm.targets : 0.0);
      if (!score_output.empty()) {
        std::FILE* f = std::fopen(score_output.c_str(), "w");
        if (!f) throw std::runtime_error("cannot write " + score_output);
        for (size_t s = 0; s < ll.size(); ++s) std::fprintf(f, "%.17g %lld\n", ll[s], (long long)targets[s]);
        std::fclose(f);
      }
    } catch (const std::exception& e) {
      std::cerr << e.what() << std::endl;
      return 2;
    }
  }
  return 0;
}
