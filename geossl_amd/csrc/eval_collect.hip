// The one launch an evaluation pass makes per batch behind the backbone and the head (eval() of finetune_qm9.py:278-384,
// finetune_lba.py:68-101, finetune_lep.py:66-101): the batch's error sums onto a persistent accumulator and its rows into
// the loader-long result arrays, so that the loop reads nothing back.
//
// geossl_eval_collect, k_eval_collect (one block of kLossBlock threads):
//   per row b < B, in fp32 (the reference's tensors are):
//     kind 0 (regression):         d = pred_b - target_b (one rounding), a = |d|, s = d d (one rounding);
//     kind 1 (BCE with logits):    z = pred_b, y = target_b, a = (max(z, 0) - z y) + log1p(exp(-|z|)), every operation
//                                  rounded on its own, s = 0;
//   thread t adds the rows t, t + 256, ... in order into fp64, then the block tree of head_common.h; thread 0 ADDS the
//   two sums and B onto acc = [sum a (f64), sum s (f64), rows (i64), unused (i64)], which the caller zeroes before a pass
//   and reads once behind it;
//   out_pred[offset + b] = pred_b, out_true[offset + b] = target_b (either may be null: the sums alone).
// `offset` is a host value: the launch is made eagerly behind a graph replay.  A fixed order and no atomics: the same
// inputs give the same bits.  All stores are plain vector stores.
#include "geossl_hip.h"
#include "head_common.h"

using namespace geossl;

namespace {

enum Kind { kRegression = 0, kBceLogits = 1 };

struct EvalSums {
  double a, s;
  __device__ __forceinline__ EvalSums& operator+=(const EvalSums& o) {
    a += o.a;
    s += o.s;
    return *this;
  }
};

template <int KIND>
__global__ __launch_bounds__(kLossBlock) void k_eval_collect(const float* __restrict__ pred,
                                                             const float* __restrict__ target, int B, int64_t offset,
                                                             float* __restrict__ out_pred, float* __restrict__ out_true,
                                                             double* __restrict__ sums, long long* __restrict__ rows) {
  __shared__ EvalSums red[kLossBlock];
  EvalSums m{0.0, 0.0};
  for (int b = threadIdx.x; b < B; b += kLossBlock) {
    const float p = pred[b], t = target[b];
    if constexpr (KIND == kRegression) {
      const float d = sub_rn(p, t);
      m.a += (double)fabsf(d);
      m.s += (double)mul_rn(d, d);
    } else {
      const float lin = sub_rn(fmaxf(p, 0.0f), mul_rn(p, t));
      m.a += (double)add_rn(lin, log1pf(expf(-fabsf(p))));
    }
    if (out_pred != nullptr) out_pred[offset + b] = p;
    if (out_true != nullptr) out_true[offset + b] = t;
  }
  const EvalSums tot = block_sum<kLossBlock>(m, red);
  if (threadIdx.x == 0) {
    sums[0] += tot.a;
    sums[1] += tot.s;
    rows[0] += (long long)B;
  }
}

}  // namespace

extern "C" int geossl_eval_collect(const float* pred, const float* target, int64_t B, int kind, int64_t offset,
                                   float* out_pred, float* out_true, void* acc, hipStream_t stream) {
  if (B < 0 || B >= (1 << 24) || offset < 0 || offset >= ((int64_t)1 << 40) || acc == nullptr ||
      (kind != kRegression && kind != kBceLogits) || (B > 0 && (pred == nullptr || target == nullptr)))
    return (int)hipErrorInvalidValue;
  if (B == 0) return 0;
  double* sums = reinterpret_cast<double*>(acc);
  long long* rows = reinterpret_cast<long long*>(sums + 2);
  if (kind == kRegression)
    hipLaunchKernelGGL(k_eval_collect<kRegression>, dim3(1), dim3(kLossBlock), 0, stream, pred, target, (int)B, offset,
                       out_pred, out_true, sums, rows);
  else
    hipLaunchKernelGGL(k_eval_collect<kBceLogits>, dim3(1), dim3(kLossBlock), 0, stream, pred, target, (int)B, offset,
                       out_pred, out_true, sums, rows);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}
