// Dropout of the Transformer_RCNN head in training mode (`--tf_rcnn --dropout p`): the element-wise sites (dropout1, the
// feed-forward's dropout, dropout2).  Dropout on the softmax probabilities is part of the attention kernels (csrc/mha.hip).
// Masks come from the counter generator of nbm_philox.h and are never stored: the backward evaluates them again.
#include "nbm_common.h"
#include "nbm_philox.h"

namespace {

// y = (res ? res : 0) + (keep ? x * scale : 0).  One thread per quad of four elements: one Philox evaluation, 16-byte accesses;
// the n % 4 elements behind the last whole quad are one thread's scalar work.  __fmul_rn / __fadd_rn: no contraction, the result is
// that of the two separately rounded float32 operations.
__global__ __launch_bounds__(256) void dropout_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                      float* __restrict__ y, long long n, uint32_t threshold, float scale,
                                                      uint64_t seed, uint32_t call, uint32_t site_id) {
  const long long n4 = n >> 2;
  const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
  const f32x4* r4 = reinterpret_cast<const f32x4*>(res);
  f32x4* y4 = reinterpret_cast<f32x4*>(y);
  for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < n4; q += (long long)gridDim.x * blockDim.x) {
    uint32_t w[4];
    nbm_dropout_words(seed, call, site_id, (uint64_t)q, w);
    const f32x4 xv = x4[q];
    f32x4 out;
#pragma unroll
    for (int e = 0; e < 4; ++e) out[e] = w[e] >= threshold ? __fmul_rn(xv[e], scale) : 0.f;
    if (res) {
      const f32x4 rv = r4[q];
#pragma unroll
      for (int e = 0; e < 4; ++e) out[e] = __fadd_rn(rv[e], out[e]);
    }
    y4[q] = out;
  }
  if ((n & 3) && blockIdx.x == 0 && threadIdx.x == 0) {
    uint32_t w[4];
    nbm_dropout_words(seed, call, site_id, (uint64_t)n4, w);
    for (int e = 0; e < (int)(n & 3); ++e) {
      const long long i = n4 * 4 + e;
      const float v = w[e] >= threshold ? __fmul_rn(x[i], scale) : 0.f;
      y[i] = res ? __fadd_rn(res[i], v) : v;
    }
  }
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int nbm_dropout(const float* x, const float* residual, float* y, int64_t n, uint32_t threshold, float scale,
                           uint64_t seed, uint32_t call, uint32_t site_id, void* stream) {
  if (!x || !y || n <= 0) return NBM_EINVAL;
  if (!nbm_aligned16(x) || !nbm_aligned16(y) || (residual && !nbm_aligned16(residual))) return NBM_EALIGN;
  const long long quads = ((long long)n + 3) >> 2;
  const long long blocks = (quads + 255) / 256;
  hipLaunchKernelGGL(dropout_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, ST, x, residual, y,
                     (long long)n, threshold, scale, seed, call, site_id);
  return nbm_launch_status();
}
