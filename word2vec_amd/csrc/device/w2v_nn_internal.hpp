// w2v_nn_internal.hpp — the index behind w2v_nn_* (include/w2v_dev.h), shared
// by the units that serve it: w2v_nn.hip (queries) and w2v_kmeans.hip (word
// classes). Not part of the public boundary.
#pragma once
#include "w2v_dev_internal.hpp"

struct w2v_nn {
  int device = 0;
  hipStream_t stream = nullptr;
  w2v_dev* h = nullptr;  // attached: the handle whose matrix is borrowed
  int32_t which = 0;
  const float* rows = nullptr;   // the matrix the kernels read: the handle's, or rows_own
  w2v::DevBuf<float> rows_own;  // empty when attached
  int64_t n_rows = 0;
  int32_t dim = 0;
  int32_t cols = 0;  // dim rounded up to 16
  int64_t pitch = 0;
  w2v::DevBuf<float> inv_norm;
  // scratch, grown on demand
  w2v::DevBuf<float> q, wts, p_score, o_score;
  w2v::DevBuf<int32_t> ids, p_id, o_id;
  int64_t strip_rows_set = 0;
  int64_t plan_strips = 0, plan_strip_rows = 0;

  ~w2v_nn() {  // the buffers free themselves after this
    (void)hipSetDevice(device);
    if (stream) {
      (void)hipStreamSynchronize(stream);
      (void)hipStreamDestroy(stream);
    }
  }
};
