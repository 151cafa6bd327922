// host_selftest.cpp — exercises the host side of the boundary (the Word2Vec
// class's vocabulary, Huffman, table, sampling, weight init, corpus readers,
// vector/vocab files, and the C bridge's argument checks) with no device call,
// for the AddressSanitizer / UndefinedBehaviorSanitizer build
// (make -C word2vec_amd/csrc asan; tests/test_host_sanitizers.py).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "Word2Vec.h"
#include "w2v_corpus.h"
#include "w2v_host.h"
#include "w2v_model.h"

namespace {

int failures = 0;
void expect(bool ok, const char* what) {
  if (!ok) {
    std::fprintf(stderr, "FAIL: %s\n", what);
    ++failures;
  }
}

std::vector<std::vector<std::string>> corpus(int n_sent, int len, int vmax, unsigned seed) {
  std::mt19937 g(seed);
  std::vector<std::vector<std::string>> out;
  for (int s = 0; s < n_sent; ++s) {
    std::vector<std::string> sent;
    for (int t = 0; t < len; ++t) {
      // Zipf-ish: rank = floor(vmax^u) - 1
      const double u = std::uniform_real_distribution<double>(0.0, 1.0)(g);
      sent.push_back("w" + std::to_string((int)std::pow((double)vmax, u) - 1));
    }
    out.push_back(sent);
  }
  return out;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : "/tmp";
  auto sents = corpus(60, 120, 400, 7);
  for (const char* method : {"hs", "ns"}) {
    for (const char* model : {"sg", "cbow"}) {
      const bool ns = std::string(method) == "ns";
      Word2Vec w(1, 5, 2, 20000, 24, ns ? 5 : 0, 1e-3f, 0.025f, 1e-6f, true, 1, method, model);
      w.generator.seed(11);
      w.build_vocab(sents);
      expect(!w.vocab.empty(), "vocab built");
      for (size_t i = 1; i < w.vocab.size(); ++i) expect(w.vocab[i - 1]->count >= w.vocab[i]->count, "sorted by count");
      if (!ns) {
        for (Word* v : w.vocab) expect(v->codes.size() == v->points.size() && !v->codes.empty(), "huffman path");
      } else {
        expect(w.table.size() == 20000, "table size");
      }
      w.init_weights(w.vocab.size());
      expect(w.W.rows() == (long)w.vocab.size(), "W rows");
      auto samples = w.build_sample(sents);
      expect(samples.size() == sents.size(), "build_sample");
      const std::string vec = dir + "/selftest_vec.txt", vecb = dir + "/selftest_vec.bin", voc = dir + "/selftest_vocab.txt";
      w.save_word2vec(vec, w.W, false);
      w.save_word2vec(vecb, w.W, true);
      w.save_vocab(voc);
      RMatrixXf keep = w.W;
      w.load_word2vec(vecb, true);
      bool same = true;
      for (long k = 0; k < keep.size(); ++k) same = same && keep.data()[k] == w.W.data()[k];
      expect(same, "binary round trip");
      w.load_word2vec(vec, false);
      Word2Vec r;
      r.read_vocab(voc);
      expect(r.vocab.size() == w.vocab.size(), "read_vocab");
    }
  }
  {  // corpus file readers
    const std::string path = dir + "/selftest_corpus.txt";
    {
      std::ofstream f(path);
      for (auto& s : sents) {
        for (size_t t = 0; t < s.size(); ++t) f << (t ? " " : "") << s[t];
        f << "\n";
      }
    }
    Word2Vec a(1, 5, 2, 20000, 16, 5, 1e-3f, 0.025f, 1e-6f, true, 1, "ns", "sg");
    Word2Vec b(1, 5, 2, 20000, 16, 5, 1e-3f, 0.025f, 1e-6f, true, 1, "ns", "sg");
    a.build_vocab(sents);
    b.build_vocab_file(path, "lines", 2);
    expect(a.vocab.size() == b.vocab.size(), "build_vocab_file == build_vocab");
    for (size_t i = 0; i < a.vocab.size() && i < b.vocab.size(); ++i)
      expect(a.vocab[i]->text == b.vocab[i]->text && a.vocab[i]->count == b.vocab[i]->count, "same vocab order");
    std::vector<int32_t> ids;
    std::vector<int64_t> off;
    int64_t tw = 0;
    b.file_samples(path, "text8", 3, ids, off, tw);
    expect(tw == 60 * 120, "train_words");
  }
  {  // phrase words: composed recursively from earlier ids; a bad half is refused
    std::vector<std::string> words{"new", "york", "city"};
    const int32_t left[2] = {0, 3}, right[2] = {1, 2};
    w2v_corpus::append_phrase_words(words, left, right, 2);
    expect(words.size() == 5 && words[3] == "new_york" && words[4] == "new_york_city", "phrase words");
    const int32_t self[1] = {5}, zero[1] = {0};
    bool threw = false;
    try {
      w2v_corpus::append_phrase_words(words, self, zero, 1);
    } catch (const std::out_of_range&) {
      threw = true;
    }
    expect(threw && words.size() == 5, "phrase half beyond the earlier ids rejected");
    Word2Vec w(1, 5, 2, 20000, 16, 5, 1e-3f, 0.025f, 1e-6f, true, 1, "ns", "sg");
    w.phrase = true;
    threw = false;
    try {
      w.build_vocab(sents);
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    expect(threw, "build_vocab(sentences) refused in phrase mode");
  }
  {  // C bridge argument checks
    w2v_model* m = w2v_model_new(1, 5, 2, 20000, 16, 5, 1e-3f, 0.025f, 1e-6f, 1, 1, "ns", "sg");
    std::string text;
    for (auto& s : sents) {
      for (auto& t : s) text += t + " ";
      text += "\n";
    }
    expect(w2v_model_build_vocab(m, text.data(), (int64_t)text.size()) == 0, "bridge build_vocab");
    expect(w2v_model_word(m, -1) == nullptr, "word(-1) rejected");
    expect(w2v_model_word(m, 1 << 30) == nullptr, "word(big) rejected");
    expect(w2v_model_word_count(m, 1 << 30) == -1, "count(big) rejected");
    std::vector<float> mat(4 * 16, 0.5f);
    expect(w2v_model_set_matrix(m, 0, mat.data(), 4, 17) != 0, "set_matrix wrong width rejected");
    expect(w2v_model_set_matrix(m, 0, mat.data(), 4, 16) == 0, "set_matrix ok");
    int32_t bad[2] = {0, 1 << 30};
    expect(w2v_model_train_sentence(m, bad, 2, 0.01f, 0) != 0, "train_sentence bad id rejected");
    float x[16] = {0}, g[16] = {0};
    expect(w2v_model_negative_sampling(m, 1 << 30, x, g, 1, 0.01f) != 0, "negative_sampling bad id rejected");
    // most_similar / analogy: an unknown word is refused before any device call
    int32_t oi[4];
    float os[4];
    int32_t on = -1;
    expect(w2v_model_most_similar_words(m, "w0 no-such-word", "w1", 4, 0, oi, os, &on) != 0, "most_similar unknown word");
    expect(std::string(w2v_model_last_error(m)).find("no-such-word") != std::string::npos, "the error names the word");
    expect(w2v_model_analogy(m, "w0", "w1", "no-such-word", 1, 0, oi, os, &on) != 0, "analogy unknown word");
    expect(w2v_model_most_similar_words(m, "w0", "", 4, 0, nullptr, os, &on) != 0, "most_similar null output");
    w2v_model_free(m);
  }
  {  // the class members themselves: last_error and the exception
    Word2Vec w(1, 5, 2, 20000, 16, 5, 1e-3f, 0.025f, 1e-6f, true, 1, "ns", "sg");
    w.build_vocab(sents);
    bool threw = false;
    try {
      w.analogy("w0", "w1", "no-such-word");
    } catch (const std::runtime_error&) {
      threw = true;
    }
    expect(threw && w.last_error.find("no-such-word") != std::string::npos, "Word2Vec::analogy unknown word");
  }
  {  // score_ids: the host-side argument checks come before any device call
    Word2Vec w(1, 5, 2, 20000, 16, 5, 1e-3f, 0.025f, 1e-6f, true, 1, "ns", "sg");
    w.build_vocab(sents);
    w.init_weights(w.vocab.size());
    auto refused = [&](const std::vector<int32_t>& ids, const std::vector<int64_t>& off) {
      try {
        w.score_ids(ids, off);
      } catch (const std::invalid_argument&) {
        return true;
      } catch (...) {
      }
      return false;
    };
    const int32_t V = (int32_t)w.vocab.size();
    expect(refused({0, 1}, {}), "score_ids: empty offsets");
    expect(refused({0, 1}, {0, 1}), "score_ids: offsets short of the ids");
    expect(refused({0, 1}, {1, 2}), "score_ids: offsets not from 0");
    expect(refused({0, 1, 0}, {0, 2, 1, 3}), "score_ids: decreasing offsets");
    expect(refused({0, V}, {0, 2}), "score_ids: id past the vocabulary");
    expect(refused({-1, 0}, {0, 2}), "score_ids: negative id");
    w.window = 128;
    expect(refused({0, 1}, {0, 2}), "score_ids: window past the scoring limit");
    w.window = 5;
    w.negative = 64;
    expect(refused({0, 1}, {0, 2}), "score_ids: negative past the scoring limit");
    w.negative = 5;
    {  // hs together with negative > 0: refused by score_ids, and by train with a (valid) held-out set
      w.train_method = "hs";
      expect(refused({0, 1}, {0, 2}), "score_ids: hs together with negative > 0");
      w.heldout_ids = {0, 1};
      w.heldout_offsets = {0, 2};
      std::vector<int32_t> ids{0, 1};
      std::vector<int64_t> off{0, 2};
      const std::vector<float> w0(w.W.data(), w.W.data() + (size_t)w.W.rows() * (size_t)w.W.cols());
      bool threw = false;
      try {
        w.train_ids(ids, off, 2);
      } catch (const std::invalid_argument& e) {
        threw = std::string(e.what()).find("no single objective") != std::string::npos;
      }
      expect(threw, "train: hs together with negative > 0 and a held-out set is refused before any device call");
      expect(w0.size() == (size_t)w.W.rows() * (size_t)w.W.cols() && w0.size() > 0 &&
                 std::equal(w0.begin(), w0.end(), w.W.data()),
             "train: a refused held-out set leaves the weights as init_weights set them");
      w.train_method = "ns";
      w.heldout_ids.clear();
      w.heldout_offsets.clear();
    }
    w.W.resize(1, 16);
    expect(refused({0, 1}, {0, 2}), "score_ids: matrices of another shape");
    w.heldout_ids = {0, V};
    w.heldout_offsets = {0, 2};
    std::vector<int32_t> ids{0, 1};
    std::vector<int64_t> off{0, 2};
    bool threw = false;
    try {
      w.train_ids(ids, off, 2);
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    expect(threw, "train: a bad held-out set is refused before any device call");
  }
  std::printf("host selftest: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
