// Dropout of the Transformer_RCNN head in training mode (`--tf_rcnn --dropout p`): the element-wise sites (dropout1, the
// feed-forward's dropout, dropout2) and multi-head attention with dropout on the softmax probabilities, forward and backward.
// Masks come from the counter generator of nbm_philox.h and are never stored: the backward kernels evaluate them again.
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

// ---- nbm_mha_small with dropout on the probabilities.  Layout, limits and *n_valid handling are mha_small_kernel's
// (csrc/pointwise.hip): one workgroup per (batch entry n, head), K and V of the group in LDS, each wave owns query rows.
// A[r][j] = keep ? (e_j / sum) * drop_scale : 0, out = A V; the mask element of (n, h, r, j) is that of a dense
// [N][nhead][S][S] tensor with S the launch's S (not *n_valid).
#define MHA_SMAX 128

__device__ __forceinline__ bool mha_keep(uint64_t seed, uint32_t call, uint32_t site_id, uint64_t row_base, int j,
                                         uint32_t threshold) {
  return nbm_dropout_word(seed, call, site_id, row_base + (uint64_t)j) >= threshold;
}

__global__ __launch_bounds__(256) void mha_small_drop_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                             const float* __restrict__ v, int q_ld, int k_ld, int v_ld,
                                                             float* __restrict__ out, int out_ld, int S, int nhead, int hd,
                                                             long long seq_stride, long long batch_stride,
                                                             const int* __restrict__ n_valid, float scale, uint32_t threshold,
                                                             float drop_scale, uint64_t seed, uint32_t call, uint32_t site_id) {
  __shared__ float Ks[MHA_SMAX][65];
  __shared__ float Vs[MHA_SMAX][64];
  __shared__ float qs[4][64];
  __shared__ float ps[4][MHA_SMAX];
  const int n = blockIdx.x / nhead, h = blockIdx.x - n * nhead;
  const int nv = n_valid ? min(*n_valid, S) : S;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < nv * hd; i += 256) {
    const int j = i / hd, d = i - j * hd;
    const long long row = j * seq_stride + n * batch_stride;
    Ks[j][d] = k[row * k_ld + h * hd + d];
    Vs[j][d] = v[row * v_ld + h * hd + d];
  }
  __syncthreads();
  for (int r = wave; r < nv; r += 4) {
    const long long row = r * seq_stride + n * batch_stride;
    const uint64_t row_base = ((uint64_t)blockIdx.x * (uint64_t)S + (uint64_t)r) * (uint64_t)S;
    if (lane < hd) qs[wave][lane] = q[row * q_ld + h * hd + lane] * scale;
    __builtin_amdgcn_wave_barrier();
    float sc[MHA_SMAX / 64];
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < MHA_SMAX / 64; ++t) {
      const int j = lane + 64 * t;
      float a = -INFINITY;
      if (j < nv) {
        a = 0.f;
        for (int d = 0; d < hd; ++d) a += qs[wave][d] * Ks[j][d];
      }
      sc[t] = a;
      m = fmaxf(m, a);
    }
    m = nbm_wave_max(m);
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < MHA_SMAX / 64; ++t) {
      sc[t] = (lane + 64 * t < nv) ? expf(sc[t] - m) : 0.f;
      sum += sc[t];
    }
    sum = nbm_wave_sum(sum);
#pragma unroll
    for (int t = 0; t < MHA_SMAX / 64; ++t) {
      const int j = lane + 64 * t;
      if (j < nv) ps[wave][j] = mha_keep(seed, call, site_id, row_base, j, threshold) ? (sc[t] / sum) * drop_scale : 0.f;
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < hd) {
      float o = 0.f;
      for (int j = 0; j < nv; ++j) o += ps[wave][j] * Vs[j][lane];
      out[row * out_ld + h * hd + lane] = o;
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// Backward, pass 1 (a wave per query row): recompute P and the mask, dA = dO V^T, dP = keep ? dA * drop_scale : 0,
// dS = P (dP - sum(P dP)), dQ = scale dS K.  The workspace gets A (the dropped probabilities, for dV = A^T dO) and dS.
__global__ __launch_bounds__(256) void mha_small_drop_bwd_rows_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, const float* __restrict__ go,
    int q_ld, int k_ld, int v_ld, int go_ld, float* __restrict__ gq, int gq_ld, float* __restrict__ ws, int S, int nhead,
    int hd, long long seq_stride, long long batch_stride, const int* __restrict__ n_valid, float scale, uint32_t threshold,
    float drop_scale, uint64_t seed, uint32_t call, uint32_t site_id) {
  __shared__ float Ks[MHA_SMAX][65];
  __shared__ float Vs[MHA_SMAX][65];
  __shared__ float qs[4][64];
  __shared__ float gs[4][64];
  __shared__ float ds[4][MHA_SMAX];
  const int n = blockIdx.x / nhead, h = blockIdx.x - n * nhead;
  const int nv = n_valid ? min(*n_valid, S) : S;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < nv * hd; i += 256) {
    const int j = i / hd, d = i - j * hd;
    const long long row = j * seq_stride + n * batch_stride;
    Ks[j][d] = k[row * k_ld + h * hd + d];
    Vs[j][d] = v[row * v_ld + h * hd + d];
  }
  __syncthreads();
  float* A = ws + (long long)blockIdx.x * 2 * S * S;
  float* D = A + (long long)S * S;
  for (int r = wave; r < nv; r += 4) {
    const long long row = r * seq_stride + n * batch_stride;
    const uint64_t row_base = ((uint64_t)blockIdx.x * (uint64_t)S + (uint64_t)r) * (uint64_t)S;
    if (lane < hd) {
      qs[wave][lane] = q[row * q_ld + h * hd + lane] * scale;
      gs[wave][lane] = go[row * go_ld + h * hd + lane];
    }
    __builtin_amdgcn_wave_barrier();
    float sc[MHA_SMAX / 64], dp[MHA_SMAX / 64];
    bool keep[MHA_SMAX / 64];
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < MHA_SMAX / 64; ++t) {
      const int j = lane + 64 * t;
      float a = -INFINITY, b = 0.f;
      keep[t] = false;
      if (j < nv) {
        a = 0.f;
        for (int d = 0; d < hd; ++d) { a += qs[wave][d] * Ks[j][d]; b += gs[wave][d] * Vs[j][d]; }
        keep[t] = mha_keep(seed, call, site_id, row_base, j, threshold);
      }
      sc[t] = a;
      dp[t] = keep[t] ? b * drop_scale : 0.f;
      m = fmaxf(m, a);
    }
    m = nbm_wave_max(m);
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < MHA_SMAX / 64; ++t) {
      sc[t] = (lane + 64 * t < nv) ? expf(sc[t] - m) : 0.f;
      sum += sc[t];
    }
    sum = nbm_wave_sum(sum);
    float dot = 0.f;
#pragma unroll
    for (int t = 0; t < MHA_SMAX / 64; ++t) { sc[t] /= sum; dot += sc[t] * dp[t]; }
    dot = nbm_wave_sum(dot);
#pragma unroll
    for (int t = 0; t < MHA_SMAX / 64; ++t) {
      const int j = lane + 64 * t;
      if (j < nv) {
        const float dsv = sc[t] * (dp[t] - dot);
        ds[wave][j] = dsv;
        A[(long long)r * S + j] = keep[t] ? sc[t] * drop_scale : 0.f;
        D[(long long)r * S + j] = dsv;
      }
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < hd) {
      float o = 0.f;
      for (int j = 0; j < nv; ++j) o += ds[wave][j] * Ks[j][lane];
      gq[row * gq_ld + h * hd + lane] = o * scale;
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// Pass 2 (a wave per key row): dK = scale dS^T Q, dV = A^T dO from the workspace of pass 1.
__global__ __launch_bounds__(256) void mha_small_drop_bwd_keys_kernel(
    const float* __restrict__ q, const float* __restrict__ go, int q_ld, int go_ld, const float* __restrict__ ws,
    float* __restrict__ gk, float* __restrict__ gv, int gk_ld, int gv_ld, int S, int nhead, int hd, long long seq_stride,
    long long batch_stride, const int* __restrict__ n_valid, float scale) {
  const int n = blockIdx.x / nhead, h = blockIdx.x - n * nhead;
  const int nv = n_valid ? min(*n_valid, S) : S;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* A = ws + (long long)blockIdx.x * 2 * S * S;
  const float* D = A + (long long)S * S;
  if (lane >= hd) return;
  for (int j = wave; j < nv; j += 4) {
    float ak = 0.f, av = 0.f;
    for (int r = 0; r < nv; ++r) {
      const long long row = r * seq_stride + n * batch_stride;
      ak += D[(long long)r * S + j] * q[row * q_ld + h * hd + lane];
      av += A[(long long)r * S + j] * go[row * go_ld + h * hd + lane];
    }
    const long long rowj = j * seq_stride + n * batch_stride;
    gk[rowj * gk_ld + h * hd + lane] = ak * scale;
    gv[rowj * gv_ld + h * hd + lane] = av;
  }
}

// LayerNorm backward whose parameter gradients are summed in a fixed order, for the dropout path: a (seed, call) pair is meant to
// reproduce a step's gradients bit for bit, which layernorm_bwd_kernel's float atomics (csrc/pointwise_bwd.hip) do not.  Row
// arithmetic as there, one wave per row; every wave stores its share of dW = sum g * xhat and dB = sum g to its own slot
// part[slot][2][E] (a wave that met no row stores zeros), and layernorm_bwd_det_finish_kernel adds the slots in ascending order.
__global__ __launch_bounds__(256) void layernorm_bwd_det_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                const float* __restrict__ g, long long rows, int E, float eps,
                                                                float* __restrict__ gx, float* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  float aw[16], ab[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) aw[k] = ab[k] = 0.f;
  for (long long row = blockIdx.x * 4ll + (threadIdx.x >> 6); row < rows; row += (long long)gridDim.x * 4) {
    const float* xr = x + row * E;
    const float* gr = g + row * E;
    float s = 0.f;
    for (int c = lane; c < E; c += 64) s += xr[c];
    const float mean = nbm_wave_sum(s) / (float)E;
    float q = 0.f;
    for (int c = lane; c < E; c += 64) { const float d = xr[c] - mean; q += d * d; }
    const float rstd = 1.0f / sqrtf(nbm_wave_sum(q) / (float)E + eps);
    float c1 = 0.f, c2 = 0.f;
    for (int c = lane; c < E; c += 64) {
      const float xh = (xr[c] - mean) * rstd, gw_ = gr[c] * w[c];
      c1 += gw_;
      c2 += gw_ * xh;
    }
    c1 = nbm_wave_sum(c1) / (float)E;
    c2 = nbm_wave_sum(c2) / (float)E;
    float* o = gx + row * E;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int c = lane + 64 * k;
      if (c < E) {
        const float xh = (xr[c] - mean) * rstd, gv = gr[c];
        o[c] = rstd * (gv * w[c] - c1 - xh * c2);
        aw[k] += gv * xh;
        ab[k] += gv;
      }
    }
  }
  float* slot = part + ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 2 * E;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int c = lane + 64 * k;
    if (c < E) { slot[c] = aw[k]; slot[E + c] = ab[k]; }
  }
}

__global__ __launch_bounds__(256) void layernorm_bwd_det_finish_kernel(const float* __restrict__ part, int slots, int E,
                                                                       float* __restrict__ gw, float* __restrict__ gb) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= E) return;
  float sw = 0.f, sb = 0.f;
  for (int s = 0; s < slots; ++s) {
    sw += part[(long long)s * 2 * E + c];
    sb += part[(long long)s * 2 * E + E + c];
  }
  gw[c] = sw;
  gb[c] = sb;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int nbm_layernorm_bwd_det(const float* x, const float* w, const float* g, int64_t rows, int E, float eps, float* gx,
                                     float* gw, float* gb, float* workspace, int64_t workspace_floats, void* stream) {
  if (!x || !w || !g || !gx || !gw || !gb || !workspace || rows <= 0 || E <= 0 || E > 1024) return NBM_EINVAL;
  long long blocks = ((long long)rows + 3) / 4;
  if (blocks > 256) blocks = 256;
  if (workspace_floats < blocks * 8 * E) return NBM_EINVAL;          // 4 waves x (dW, dB) x E floats per workgroup
  hipLaunchKernelGGL(layernorm_bwd_det_kernel, dim3((unsigned)blocks), dim3(256), 0, ST, x, w, g, (long long)rows, E, eps, gx,
                     workspace);
  hipLaunchKernelGGL(layernorm_bwd_det_finish_kernel, dim3((E + 255) / 256), dim3(256), 0, ST, workspace, (int)(blocks * 4), E,
                     gw, gb);
  return nbm_launch_status();
}

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

extern "C" int nbm_mha_small_drop(const float* q, const float* k, const float* v, int q_ld, int k_ld, int v_ld, float* out,
                                  int out_ld, int S, int N, int nhead, int hd, int64_t seq_stride, int64_t batch_stride,
                                  const int32_t* n_valid, float scale, uint32_t threshold, float drop_scale, uint64_t seed,
                                  uint32_t call, uint32_t site_id, void* stream) {
  if (!q || !k || !v || !out || S <= 0 || S > MHA_SMAX || N <= 0 || nhead <= 0 || hd <= 0 || hd > 64) return NBM_EINVAL;
  if (q_ld < nhead * hd || k_ld < nhead * hd || v_ld < nhead * hd || out_ld < nhead * hd) return NBM_EINVAL;
  hipLaunchKernelGGL(mha_small_drop_kernel, dim3(N * nhead), dim3(256), 0, ST, q, k, v, q_ld, k_ld, v_ld, out, out_ld, S,
                     nhead, hd, (long long)seq_stride, (long long)batch_stride, n_valid, scale, threshold, drop_scale, seed,
                     call, site_id);
  return nbm_launch_status();
}

extern "C" int nbm_mha_small_drop_bwd(const float* q, const float* k, const float* v, const float* go, int q_ld, int k_ld,
                                      int v_ld, int go_ld, float* gq, float* gk, float* gv, int gq_ld, int gk_ld, int gv_ld,
                                      float* workspace, int S, int N, int nhead, int hd, int64_t seq_stride,
                                      int64_t batch_stride, const int32_t* n_valid, float scale, uint32_t threshold,
                                      float drop_scale, uint64_t seed, uint32_t call, uint32_t site_id, void* stream) {
  if (!q || !k || !v || !go || !gq || !gk || !gv || !workspace) return NBM_EINVAL;
  if (S <= 0 || S > MHA_SMAX || N <= 0 || nhead <= 0 || hd <= 0 || hd > 64) return NBM_EINVAL;
  const int E = nhead * hd;
  if (q_ld < E || k_ld < E || v_ld < E || go_ld < E || gq_ld < E || gk_ld < E || gv_ld < E) return NBM_EINVAL;
  hipLaunchKernelGGL(mha_small_drop_bwd_rows_kernel, dim3(N * nhead), dim3(256), 0, ST, q, k, v, go, q_ld, k_ld, v_ld, go_ld,
                     gq, gq_ld, workspace, S, nhead, hd, (long long)seq_stride, (long long)batch_stride, n_valid, scale,
                     threshold, drop_scale, seed, call, site_id);
  hipLaunchKernelGGL(mha_small_drop_bwd_keys_kernel, dim3(N * nhead), dim3(256), 0, ST, q, go, q_ld, go_ld, workspace, gk, gv,
                     gk_ld, gv_ld, S, nhead, hd, (long long)seq_stride, (long long)batch_stride, n_valid, scale);
  return nbm_launch_status();
}
