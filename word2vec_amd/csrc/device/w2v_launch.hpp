// Kernel entry points per row width (defined in w2v_inst.hip, one object per width).
#pragma once
#include <stdint.h>

namespace w2v {

struct TrainArgs;
using KernelFn = void (*)(TrainArgs);
using ApplyFn = void (*)(float*, int64_t, int, const float*, float*, const uint8_t*, int, float, int);

// The instantiated row widths (floats per lane), ascending: one object each
// (the Makefile's NVS repeats the list).
#define W2V_FOR_EACH_NV(X) X(1) X(2) X(3) X(4) X(5) X(6) X(8) X(12) X(16) X(24) X(32)

#define W2V_DECLARE_NV(N)                                            \
  KernelFn pick_train_nv##N(bool cbow, bool hs, bool ns, bool replay, bool wide); \
  KernelFn pick_train_deep_nv##N(bool cbow); \
  ApplyFn pick_apply_nv##N();
W2V_FOR_EACH_NV(W2V_DECLARE_NV)
#undef W2V_DECLARE_NV

// A width's pickers; kNvKernels lists the widths in ascending order.
struct NvKernels {
  int nv;
  KernelFn (*pick_train)(bool cbow, bool hs, bool ns, bool replay, bool wide);
  KernelFn (*pick_train_deep)(bool cbow);
  ApplyFn (*pick_apply)();
};
#define W2V_NV_ROW(N) {N, pick_train_nv##N, pick_train_deep_nv##N, pick_apply_nv##N},
inline const NvKernels kNvKernels[] = {W2V_FOR_EACH_NV(W2V_NV_ROW)};
#undef W2V_NV_ROW

// Shared-negatives minibatch SG (w2v_shared.hip) for a row pitch (floats, a
// multiple of 64 up to 1024, not 576/704/832/960); *waves = wavefronts per
// workgroup; occ = register budget in waves per SIMD (3; else the
// compiler's choice). Null for a pitch without an instantiation.
KernelFn pick_shared_neg(int64_t pitch, int occ, int* waves);

}  // namespace w2v
