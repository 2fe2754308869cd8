// The two MBConv operations the GEMM kernels do not cover (EfficientNet-B0..B4 bodies, nets/backbone.py:_MBConv):
//   nbm_dwconv_bn_act   depthwise k x k / stride s convolution (k in {3, 5}, s in {1, 2}, pad (k - 1) / 2, multiplier 1) of an NHWC fp32
//                       map with the folded norm (scale, shift) and an activation in the epilogue, and optionally the per-(image, channel)
//                       partial sums of the activated output for the squeeze-and-excitation pool;
//   nbm_se_gate         the rest of squeeze-and-excitation in one launch: mean, squeeze FC + SiLU, excite FC + sigmoid -> gate [B, C], and
//                       optionally the project convolution's weights with the gate folded in, one copy per image.
// Both are memory-bound; neither uses an atomic or relies on a zeroed buffer, so two runs give the same bits and a captured graph holds
// kernel nodes only.
#include <type_traits>
#include "nbm_common.h"

namespace {

constexpr int DW_TPB = 256;
constexpr int DW_STRIP = 32;      // output rows a workgroup walks down (nbm_dwconv_strip_rows)

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// A thread owns one output column and four consecutive channels and walks down DW_STRIP output rows.  Input rows arrive once, in
// ascending order; each is K 16-byte loads (the thread's K columns -- its neighbours in the workgroup read the same lines, so HBM sees a
// value about once, the strip's K - S halo rows aside) and goes straight into the (K + S - 1) / S output rows that are still open: the
// thread holds accumulators, not input rows.  An output element receives its K * K products in (r, s) order with a product of zero for a
// tap outside the image, whatever the strip or the position -- the bits do not depend on how the map was cut.  The K * K weight vectors
// of the thread's channels stay in registers.  All offsets are 64-bit (the widest map of b0 at B = 64 holds 2.4 G floats).
//
// Pool partials (`part` != nullptr): the workgroup's sum of its activated outputs per channel goes to slot
// (strip * n_xblocks + xblock) of part[B][n_slots][C]: per thread over its rows in order, then over the workgroup's columns in order.
template <int K, int S>
__global__ void __launch_bounds__(DW_TPB)
dwconv_bn_act_kernel(const float* __restrict__ x, const float* __restrict__ wt, const float* __restrict__ scale,
                     const float* __restrict__ shift, float* __restrict__ y, float* __restrict__ part, int H, int W, int C, int Ho, int Wo,
                     int act, int cq_log2, int n_xblocks, int n_cchunks) {
  constexpr int P = (K - 1) / 2, NACC = (K + S - 1) / S;
  __shared__ __attribute__((aligned(16))) float red[DW_TPB * 4];
  const int CQ = 1 << cq_log2, TW = DW_TPB >> cq_log2;
  const int tid = threadIdx.x, cq = tid & (CQ - 1), tx = tid >> cq_log2;
  const int xb = blockIdx.x % n_xblocks, cc = blockIdx.x / n_xblocks;
  const int strip = blockIdx.y, b = blockIdx.z;
  const int ox = xb * TW + tx, c = (cc * CQ + cq) * 4;
  const bool live = ox < Wo && c < C;
  const int cl = live ? c : 0;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  f32x4 w[K * K];
#pragma unroll
  for (int t = 0; t < K * K; ++t) w[t] = ld4(wt + (long long)t * C + cl);
  const f32x4 sc = scale ? ld4(scale + cl) : f32x4{1.f, 1.f, 1.f, 1.f};
  const f32x4 sh = shift ? ld4(shift + cl) : zero4;

  // the thread's K input columns: clamped addresses, zeroed outside the image (every load of a row is in flight before the first use)
  long long col_off[K];
  bool col_ok[K];
#pragma unroll
  for (int s = 0; s < K; ++s) {
    const int ix = ox * S - P + s;
    col_ok[s] = live && (unsigned)ix < (unsigned)W;
    col_off[s] = (long long)min(max(ix, 0), W - 1) * C + cl;
  }
  const float* __restrict__ xb_ = x + (long long)b * H * W * C;
  float* __restrict__ yb = y + (long long)b * Ho * Wo * C;

  f32x4 acc[NACC];
#pragma unroll
  for (int j = 0; j < NACC; ++j) acc[j] = zero4;
  f32x4 pool = zero4;

  // input row iy, the T-th row of the window of the oldest open output row: row r = T - j S of the j-th open output
  auto feed = [&](auto T_, int iy) {
    constexpr int T = decltype(T_)::value;
    const bool row_ok = (unsigned)iy < (unsigned)H;
    const float* rp = xb_ + (long long)min(max(iy, 0), H - 1) * W * C;
    f32x4 xs[K];
#pragma unroll
    for (int s = 0; s < K; ++s) xs[s] = ld4(rp + col_off[s]);
#pragma unroll
    for (int s = 0; s < K; ++s)
      if (!(row_ok && col_ok[s])) xs[s] = zero4;
#pragma unroll
    for (int j = 0; j < NACC; ++j) {
      const int r = T - j * S;
      if (r >= 0 && r < K) {
#pragma unroll
        for (int s = 0; s < K; ++s)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[j][e] = fmaf(xs[s][e], w[r * K + s][e], acc[j][e]);
      }
    }
  };

  const int oy0 = strip * DW_STRIP, oy1 = min(oy0 + DW_STRIP, Ho);
  // rows 0 .. K - S - 1 of the first window; every step below then feeds the S rows that complete the oldest open output
  {
    const int iy0 = oy0 * S - P;
    if constexpr (K - S > 0) feed(std::integral_constant<int, 0>{}, iy0);
    if constexpr (K - S > 1) feed(std::integral_constant<int, 1>{}, iy0 + 1);
    if constexpr (K - S > 2) feed(std::integral_constant<int, 2>{}, iy0 + 2);
    if constexpr (K - S > 3) feed(std::integral_constant<int, 3>{}, iy0 + 3);
  }
  for (int oy = oy0; oy < oy1; ++oy) {
    const int iy0 = oy * S - P;
    feed(std::integral_constant<int, K - S>{}, iy0 + K - S);
    if constexpr (S == 2) feed(std::integral_constant<int, K - 1>{}, iy0 + K - 1);
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = fmaf(acc[0][e], sc[e], sh[e]);
      if (act == NBM_ACT_SILU) v[e] = v[e] / (1.0f + expf(-v[e]));       // (nbm_silu's expression)
    }
    if (live) {
      *reinterpret_cast<f32x4*>(yb + ((long long)oy * Wo + ox) * C + c) = v;
#pragma unroll
      for (int e = 0; e < 4; ++e) pool[e] += v[e];
    }
#pragma unroll
    for (int j = 0; j + 1 < NACC; ++j) acc[j] = acc[j + 1];
    acc[NACC - 1] = zero4;
  }

  if (part) {       // (uniform over the grid)
    *reinterpret_cast<f32x4*>(red + tid * 4) = pool;       // dead threads hold zeros
    __syncthreads();
    if (tx == 0 && c < C) {
      f32x4 s = zero4;
      for (int i = 0; i < TW; ++i) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(red + ((i << cq_log2) + cq) * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] += q[e];
      }
      const long long n_slots = (long long)gridDim.y * n_xblocks;
      *reinterpret_cast<f32x4*>(part + ((long long)b * n_slots + (long long)strip * n_xblocks + xb) * C + c) = s;
    }
  }
}

// channel quads per workgroup (a power of two in 4 .. 16): the choice with the least padded width; ties to the wider chunk
inline int dw_cq_log2(int C) {
  const int q = C >> 2;
  int best = 2, waste = 1 << 30;
  for (int l = 2; l <= 4; ++l) {
    const int cqn = 1 << l, pad = (q + cqn - 1) / cqn * cqn - q;
    if (pad <= waste) { waste = pad; best = l; }
  }
  return best;
}

// One workgroup per (image, slice of the project rows).  Every workgroup of an image computes the image's gate (the same instructions on
// the same operands: the same bits); slice 0 stores it.  LDS: mean [C] | squeeze [Csq] | gate [C].
__global__ void __launch_bounds__(256)
se_gate_kernel(const float* __restrict__ part, int n_slots, float inv_hw, int C, int Csq, const float* __restrict__ w1,
               const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ gate,
               const float* __restrict__ wproj, int wp_ld, int N, float* __restrict__ wb, int w_ld) {
  extern __shared__ __attribute__((aligned(16))) float se_lds[];
  float* mean = se_lds;
  float* sq = se_lds + C;
  float* gt = sq + Csq;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* pb = part + (long long)b * n_slots * C;
  for (int c = tid; c < C; c += 256) {
    float s = 0.f;
    for (int i = 0; i < n_slots; ++i) s += pb[(long long)i * C + c];        // the slots in a fixed order
    mean[c] = s * inv_hw;
  }
  __syncthreads();
  for (int j = wave; j < Csq; j += 4) {          // one squeeze unit per wave: lanes stride the channels, then a butterfly sum
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s = fmaf(w1[(long long)j * C + c], mean[c], s);
    s = nbm_wave_sum(s) + b1[j];
    if (lane == 0) sq[j] = s / (1.0f + expf(-s));
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    float s = b2[c];
    for (int j = 0; j < Csq; ++j) s = fmaf(w2[(long long)c * Csq + j], sq[j], s);
    const float g = 1.0f / (1.0f + expf(-s));
    gt[c] = g;
    if (blockIdx.y == 0) gate[(long long)b * C + c] = g;
  }
  if (!wb) return;
  __syncthreads();
  // Wb[b][n][c] = Wproj[n][c] * gate[b][c]; the pad columns C .. w_ld - 1 are written as zeros
  const int rows_per = (N + gridDim.y - 1) / gridDim.y;
  const int n0 = blockIdx.y * rows_per, n1 = min(n0 + rows_per, N);
  const int q_ld = w_ld >> 2;
  for (int i = tid; i < (n1 - n0) * q_ld; i += 256) {
    const int n = n0 + i / q_ld, c = (i % q_ld) * 4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (c < C) {             // (C % 4 == 0: a quad is inside or outside as a whole)
      v = ld4(wproj + (long long)n * wp_ld + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] *= gt[c + e];
    }
    *reinterpret_cast<f32x4*>(wb + ((long long)b * N + n) * w_ld + c) = v;
  }
}

}  // namespace

extern "C" int nbm_dwconv_strip_rows(void) { return DW_STRIP; }

extern "C" int nbm_dwconv_pool_slots(int C, int Ho, int Wo) {
  if (C <= 0 || (C & 3) || Ho <= 0 || Wo <= 0) return NBM_EINVAL;
  const int TW = DW_TPB >> dw_cq_log2(C);
  return ((Ho + DW_STRIP - 1) / DW_STRIP) * ((Wo + TW - 1) / TW);
}

extern "C" int nbm_dwconv_bn_act(const float* x, int B, int H, int W, int C, int k, int stride, const float* w_taps, const float* scale,
                                 const float* shift, int act, float* y, int Ho, int Wo, float* pool_part, void* stream) {
  if (!x || !w_taps || !y || B <= 0 || H <= 0 || W <= 0 || C <= 0) return NBM_EINVAL;
  if ((k != 3 && k != 5) || (stride != 1 && stride != 2) || (C & 3) || (act != NBM_ACT_NONE && act != NBM_ACT_SILU)) return NBM_EUNSUPPORTED;
  const int p = (k - 1) / 2;
  if ((H + 2 * p - k) / stride + 1 != Ho || (W + 2 * p - k) / stride + 1 != Wo) return NBM_EINVAL;
  if (!nbm_aligned16(x) || !nbm_aligned16(w_taps) || !nbm_aligned16(y) || (scale && !nbm_aligned16(scale)) || (shift && !nbm_aligned16(shift)) ||
      (pool_part && !nbm_aligned16(pool_part)))
    return NBM_EALIGN;
  const int l2 = dw_cq_log2(C), CQ = 1 << l2, TW = DW_TPB >> l2;
  const int n_xblocks = (Wo + TW - 1) / TW, n_cchunks = ((C >> 2) + CQ - 1) / CQ, n_strips = (Ho + DW_STRIP - 1) / DW_STRIP;
  if (B > 65535 || n_strips > 65535) return NBM_EUNSUPPORTED;
  const dim3 grid((unsigned)(n_xblocks * n_cchunks), (unsigned)n_strips, (unsigned)B), blk(DW_TPB);
  hipStream_t st = (hipStream_t)stream;
#define NBM_DW_LAUNCH(K_, S_)                                                                                                          \
  hipLaunchKernelGGL((dwconv_bn_act_kernel<K_, S_>), grid, blk, 0, st, x, w_taps, scale, shift, y, pool_part, H, W, C, Ho, Wo, act, l2, \
                     n_xblocks, n_cchunks)
  if (k == 3 && stride == 1) NBM_DW_LAUNCH(3, 1);
  else if (k == 3) NBM_DW_LAUNCH(3, 2);
  else if (stride == 1) NBM_DW_LAUNCH(5, 1);
  else NBM_DW_LAUNCH(5, 2);
#undef NBM_DW_LAUNCH
  return nbm_launch_status();
}

extern "C" int nbm_se_gate(const float* pool_part, int B, int n_slots, int C, float inv_hw, const float* w1, const float* b1, int Csq,
                           const float* w2, const float* b2, float* gate, const float* wproj, int wp_ld, int N, float* wb, int w_ld,
                           void* stream) {
  if (!pool_part || !w1 || !b1 || !w2 || !b2 || !gate || B <= 0 || n_slots <= 0 || C <= 0 || Csq <= 0) return NBM_EINVAL;
  if (C & 3) return NBM_EUNSUPPORTED;
  if (B > 65535) return NBM_EUNSUPPORTED;
  const size_t lds = (size_t)(2 * C + Csq) * sizeof(float);
  if (lds > 48 * 1024) return NBM_EUNSUPPORTED;
  int slices = 1;
  if (wb) {
    if (!wproj || N <= 0 || wp_ld < C || w_ld < C || (w_ld & 31) || (wp_ld & 3)) return NBM_EINVAL;
    if (!nbm_aligned16(wproj) || !nbm_aligned16(wb)) return NBM_EALIGN;
    // 32 project rows per workgroup: a rule of the layer, not of B.  (NEGATIVE: 2 Csq rows per slice, so that a slice writes about as many
    // floats as its recomputation of the gate reads -- 90 -> 114 us at C = 1152 / N = 192, 494 -> 580 us at C = 2688 / N = 448, B = 64:
    // the gate phase is a chain of dependent steps, not traffic, and fewer slices leave fewer workgroups to overlap it)
    slices = (N + 31) / 32;
  }
  hipLaunchKernelGGL(se_gate_kernel, dim3((unsigned)B, (unsigned)slices), dim3(256), lds, (hipStream_t)stream, pool_part, n_slots, inv_hw,
                     C, Csq, w1, b1, w2, b2, gate, wproj, wp_ld, N, wb, w_ld);
  return nbm_launch_status();
}
