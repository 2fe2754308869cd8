// Train-mode BatchNorm (+ residual, + ReLU) over NHWC rows [M][C] for the backbone's 53 norms (include/nbm_hip.h: nbm_bn_act_*).
//
// A thread owns ONE channel quad (16 bytes) for its whole life and walks rows; the rows are strided over the threads of a workgroup
// and over the workgroups.  TQ = the smallest power of two >= C / 4 (at most 256) quads side by side, RPB = 256 / TQ rows per step of a
// workgroup, so that with C / 4 a power of two a step reads 4 KiB of consecutive memory.  Every global access of the three streaming
// kernels is a 16-byte access; no per-element division or modulo.
//   forward : reduce (z -> per-workgroup sums, double) -> finish (slots summed in ascending order; mean, invstd, running statistics)
//             -> apply (z [, residual] -> y)
//   backward: reduce (gy, y, z -> per-workgroup sums) -> finish (gbeta, ggamma and the two means) -> apply (gy, y, z -> gz [, gres])
// No atomics, nothing relies on a zeroed buffer: every slot that is read was written by the same call.
#include "nbm_common.h"

namespace {

constexpr int BN_TPB = 256;
constexpr int BN_UNROLL = 4;            // rows in flight per thread
constexpr int BN_MAX_PARTS = 1024;      // 4 workgroups on each of 256 CUs
constexpr int BN_APPLY_WGS = 2048;

struct BnGeom {
  int C4, TQ, shift, RPB, GY, parts, apply_wgs;
};

// Host only: a function of (M, C) alone.
inline BnGeom bn_geom(int64_t M, int C) {
  BnGeom g;
  g.C4 = C / 4;
  g.TQ = 1; g.shift = 0;
  while (g.TQ < g.C4 && g.TQ < BN_TPB) { g.TQ <<= 1; ++g.shift; }
  g.RPB = BN_TPB / g.TQ;
  g.GY = (g.C4 + g.TQ - 1) / g.TQ;
  // a workgroup gets at least 2 * BN_UNROLL steps of rows before a second one is opened (toy sizes: few workgroups); at the
  // backbone's sizes the cap decides: GY * parts = BN_MAX_PARTS workgroups
  const int64_t rows_per_wg = (int64_t)g.RPB * BN_UNROLL * 2;
  int64_t p = (M + rows_per_wg - 1) / rows_per_wg;
  const int64_t cap = BN_MAX_PARTS / g.GY > 0 ? BN_MAX_PARTS / g.GY : 1;
  g.parts = (int)(p < 1 ? 1 : p > cap ? cap : p);
  const int64_t rows_per_awg = (int64_t)g.RPB * BN_UNROLL;
  int64_t a = (M + rows_per_awg - 1) / rows_per_awg;
  const int64_t acap = BN_APPLY_WGS / g.GY > 0 ? BN_APPLY_WGS / g.GY : 1;
  g.apply_wgs = (int)(a < 1 ? 1 : a > acap ? acap : a);
  return g;
}
inline int64_t bn_ws_bytes(const BnGeom& g, int C) {
  // double part[parts][2][C], then float tail[2][C] (backward: the two means the apply kernel reads)
  return (int64_t)g.parts * 2 * C * 8 + (int64_t)2 * C * 4;
}

// Sum of the workgroup's rows: 8 doubles per thread -> LDS -> one sum per (quantity, quad) over the RPB row lanes in ascending order
// -> slot blockIdx.x of part[parts][2][C].
__device__ __forceinline__ void bn_block_store(const double (&s)[4], const double (&q)[4], int TQ, int shift, int C,
                                               double* __restrict__ part) {
  __shared__ double red[8][BN_TPB];
#pragma unroll
  for (int j = 0; j < 4; ++j) { red[j][threadIdx.x] = s[j]; red[4 + j][threadIdx.x] = q[j]; }
  __syncthreads();
  const int RPB = BN_TPB >> shift;
  for (int o = threadIdx.x; o < 8 * TQ; o += BN_TPB) {
    const int k = o >> shift, ql = o & (TQ - 1);
    double acc = 0.0;
    for (int r = 0; r < RPB; ++r) acc += red[k][(r << shift) + ql];
    const int c = 4 * ((int)blockIdx.y * TQ + ql) + (k & 3);
    if (c < C) part[((size_t)blockIdx.x * 2 + (k >> 2)) * C + c] = acc;
  }
}

__global__ __launch_bounds__(BN_TPB) void bn_act_reduce_kernel(const f32x4* __restrict__ z, long long M, int C, int TQ, int shift,
                                                               double* __restrict__ part) {
  const int ql = threadIdx.x & (TQ - 1), r = threadIdx.x >> shift;
  const int qi = (int)blockIdx.y * TQ + ql, C4 = C >> 2;
  const int RPB = BN_TPB >> shift;
  double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
  if (qi < C4) {
    const long long step = (long long)gridDim.x * RPB;
    long long m = (long long)blockIdx.x * RPB + r;
    for (; m + (BN_UNROLL - 1) * step < M; m += BN_UNROLL * step) {
      f32x4 v[BN_UNROLL];
#pragma unroll
      for (int u = 0; u < BN_UNROLL; ++u) v[u] = z[(m + u * step) * C4 + qi];
#pragma unroll
      for (int u = 0; u < BN_UNROLL; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) { const double d = (double)v[u][j]; s[j] += d; q[j] += d * d; }
    }
    for (; m < M; m += step) {
      const f32x4 v = z[m * C4 + qi];
#pragma unroll
      for (int j = 0; j < 4; ++j) { const double d = (double)v[j]; s[j] += d; q[j] += d * d; }
    }
  }
  bn_block_store(s, q, TQ, shift, C, part);
}

// One thread per (channel, quarter of the slots): the slots of a quarter in ascending order, then the four quarters in ascending order.
__device__ __forceinline__ void bn_sum_slots(const double* __restrict__ part, int parts, int C, int c, double& S, double& Q) {
  __shared__ double fs[4][64], fq[4][64];
  const int seg = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int per = (parts + 3) >> 2;
  double s = 0.0, q = 0.0;
  if (c < C) {
    const int p1 = (seg + 1) * per < parts ? (seg + 1) * per : parts;
    for (int p = seg * per; p < p1; ++p) { s += part[((size_t)p * 2) * C + c]; q += part[((size_t)p * 2 + 1) * C + c]; }
  }
  fs[seg][lane] = s; fq[seg][lane] = q;
  __syncthreads();
  S = ((fs[0][lane] + fs[1][lane]) + fs[2][lane]) + fs[3][lane];
  Q = ((fq[0][lane] + fq[1][lane]) + fq[2][lane]) + fq[3][lane];
}

// mean, invstd; running statistics (momentum, unbiased variance for M > 1): nn.BatchNorm2d semantics
__global__ __launch_bounds__(BN_TPB) void bn_act_fwd_finish_kernel(const double* __restrict__ part, int parts, long long M, int C,
                                                                   float eps, float momentum, float* __restrict__ mean,
                                                                   float* __restrict__ invstd, float* __restrict__ run_mean,
                                                                   float* __restrict__ run_var) {
  const int c = (int)blockIdx.x * 64 + (threadIdx.x & 63);
  double S, Q;
  bn_sum_slots(part, parts, C, c, S, Q);
  if ((threadIdx.x >> 6) != 0 || c >= C) return;
  const double mu = S / (double)M;
  double var = Q / (double)M - mu * mu;
  if (var < 0.0) var = 0.0;
  mean[c] = (float)mu;
  invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
  if (run_mean) run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * (float)mu;
  if (run_var) {
    const double unb = M > 1 ? var * (double)M / (double)(M - 1) : var;
    run_var[c] = (1.f - momentum) * run_var[c] + momentum * (float)unb;
  }
}

template <bool RELU, bool RES>
__global__ __launch_bounds__(BN_TPB) void bn_act_apply_kernel(const f32x4* __restrict__ z, const f32x4* __restrict__ res, long long M,
                                                              int C, int TQ, int shift, const f32x4* __restrict__ mean,
                                                              const f32x4* __restrict__ invstd, const f32x4* __restrict__ gamma,
                                                              const f32x4* __restrict__ beta, f32x4* __restrict__ y) {
  const int ql = threadIdx.x & (TQ - 1), r = threadIdx.x >> shift;
  const int qi = (int)blockIdx.y * TQ + ql, C4 = C >> 2;
  if (qi >= C4) return;
  const int RPB = BN_TPB >> shift;
  const f32x4 mu = mean[qi], a = gamma[qi] * invstd[qi], b = beta[qi];
  const long long step = (long long)gridDim.x * RPB;
  long long m = (long long)blockIdx.x * RPB + r;
  for (; m + (BN_UNROLL - 1) * step < M; m += BN_UNROLL * step) {
    f32x4 v[BN_UNROLL], w[BN_UNROLL];
#pragma unroll
    for (int u = 0; u < BN_UNROLL; ++u) {
      v[u] = z[(m + u * step) * C4 + qi];
      if (RES) w[u] = res[(m + u * step) * C4 + qi];
    }
#pragma unroll
    for (int u = 0; u < BN_UNROLL; ++u) {
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float t = fmaf(v[u][j] - mu[j], a[j], b[j]);
        if (RES) t += w[u][j];
        o[j] = RELU ? fmaxf(t, 0.f) : t;
      }
      y[(m + u * step) * C4 + qi] = o;
    }
  }
  for (; m < M; m += step) {
    const f32x4 v = z[m * C4 + qi];
    f32x4 w = {0.f, 0.f, 0.f, 0.f}, o;
    if (RES) w = res[m * C4 + qi];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float t = fmaf(v[j] - mu[j], a[j], b[j]);
      if (RES) t += w[j];
      o[j] = RELU ? fmaxf(t, 0.f) : t;
    }
    y[m * C4 + qi] = o;
  }
}

// backward pass 1: per-workgroup {sum g', sum g' * xhat} with g' = gy * (y > 0)
template <bool RELU>
__global__ __launch_bounds__(BN_TPB) void bn_act_bwd_reduce_kernel(const f32x4* __restrict__ gy, const f32x4* __restrict__ y,
                                                                   const f32x4* __restrict__ z, long long M, int C, int TQ, int shift,
                                                                   const f32x4* __restrict__ mean, const f32x4* __restrict__ invstd,
                                                                   double* __restrict__ part) {
  const int ql = threadIdx.x & (TQ - 1), r = threadIdx.x >> shift;
  const int qi = (int)blockIdx.y * TQ + ql, C4 = C >> 2;
  const int RPB = BN_TPB >> shift;
  double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
  if (qi < C4) {
    const f32x4 mu = mean[qi], is = invstd[qi];
    const long long step = (long long)gridDim.x * RPB;
    long long m = (long long)blockIdx.x * RPB + r;
    for (; m + (BN_UNROLL - 1) * step < M; m += BN_UNROLL * step) {
      f32x4 g[BN_UNROLL], v[BN_UNROLL], a[BN_UNROLL];
#pragma unroll
      for (int u = 0; u < BN_UNROLL; ++u) {
        g[u] = gy[(m + u * step) * C4 + qi];
        v[u] = z[(m + u * step) * C4 + qi];
        if (RELU) a[u] = y[(m + u * step) * C4 + qi];
      }
#pragma unroll
      for (int u = 0; u < BN_UNROLL; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float gm = (!RELU || a[u][j] > 0.f) ? g[u][j] : 0.f;
          const double d = (double)gm;
          s[j] += d; q[j] += d * (double)((v[u][j] - mu[j]) * is[j]);
        }
    }
    for (; m < M; m += step) {
      const f32x4 g = gy[m * C4 + qi], v = z[m * C4 + qi];
      f32x4 a = {1.f, 1.f, 1.f, 1.f};
      if (RELU) a = y[m * C4 + qi];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float gm = (!RELU || a[j] > 0.f) ? g[j] : 0.f;
        const double d = (double)gm;
        s[j] += d; q[j] += d * (double)((v[j] - mu[j]) * is[j]);
      }
    }
  }
  bn_block_store(s, q, TQ, shift, C, part);
}

// gbeta, ggamma, and the two means of the apply kernel: tail[0][C] = sum g' / M, tail[1][C] = sum g' xhat / M
__global__ __launch_bounds__(BN_TPB) void bn_act_bwd_finish_kernel(const double* __restrict__ part, int parts, long long M, int C,
                                                                   float* __restrict__ tail, float* __restrict__ ggamma,
                                                                   float* __restrict__ gbeta) {
  const int c = (int)blockIdx.x * 64 + (threadIdx.x & 63);
  double S, Q;
  bn_sum_slots(part, parts, C, c, S, Q);
  if ((threadIdx.x >> 6) != 0 || c >= C) return;
  gbeta[c] = (float)S;
  ggamma[c] = (float)Q;
  tail[c] = (float)(S / (double)M);
  tail[C + c] = (float)(Q / (double)M);
}

// backward pass 2: gz = gamma * invstd * (g' - sum g' / M - xhat * sum g' xhat / M); gres = g'
template <bool RELU, bool GRES>
__global__ __launch_bounds__(BN_TPB) void bn_act_bwd_apply_kernel(const f32x4* __restrict__ gy, const f32x4* __restrict__ y,
                                                                  const f32x4* __restrict__ z, long long M, int C, int TQ, int shift,
                                                                  const f32x4* __restrict__ mean, const f32x4* __restrict__ invstd,
                                                                  const f32x4* __restrict__ gamma, const f32x4* __restrict__ tail,
                                                                  f32x4* __restrict__ gz, f32x4* __restrict__ gres) {
  const int ql = threadIdx.x & (TQ - 1), r = threadIdx.x >> shift;
  const int qi = (int)blockIdx.y * TQ + ql, C4 = C >> 2;
  if (qi >= C4) return;
  const int RPB = BN_TPB >> shift;
  const f32x4 mu = mean[qi], is = invstd[qi], a = gamma[qi] * is, sg = tail[qi], sgx = tail[C4 + qi];
  const long long step = (long long)gridDim.x * RPB;
  long long m = (long long)blockIdx.x * RPB + r;
  for (; m + (BN_UNROLL - 1) * step < M; m += BN_UNROLL * step) {
    f32x4 g[BN_UNROLL], v[BN_UNROLL], yy[BN_UNROLL];
#pragma unroll
    for (int u = 0; u < BN_UNROLL; ++u) {
      g[u] = gy[(m + u * step) * C4 + qi];
      v[u] = z[(m + u * step) * C4 + qi];
      if (RELU) yy[u] = y[(m + u * step) * C4 + qi];
    }
#pragma unroll
    for (int u = 0; u < BN_UNROLL; ++u) {
      f32x4 gm, o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        gm[j] = (!RELU || yy[u][j] > 0.f) ? g[u][j] : 0.f;
        const float xh = (v[u][j] - mu[j]) * is[j];
        o[j] = a[j] * (gm[j] - sg[j] - xh * sgx[j]);
      }
      gz[(m + u * step) * C4 + qi] = o;
      if (GRES) gres[(m + u * step) * C4 + qi] = gm;
    }
  }
  for (; m < M; m += step) {
    const f32x4 g = gy[m * C4 + qi], v = z[m * C4 + qi];
    f32x4 yy = {1.f, 1.f, 1.f, 1.f}, gm, o;
    if (RELU) yy = y[m * C4 + qi];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      gm[j] = (!RELU || yy[j] > 0.f) ? g[j] : 0.f;
      const float xh = (v[j] - mu[j]) * is[j];
      o[j] = a[j] * (gm[j] - sg[j] - xh * sgx[j]);
    }
    gz[m * C4 + qi] = o;
    if (GRES) gres[m * C4 + qi] = gm;
  }
}

inline int bn_check(int64_t M, int C) {
  if (M <= 0 || C <= 0) return NBM_EINVAL;
  if (C & 3) return NBM_EUNSUPPORTED;
  return NBM_OK;
}

}  // namespace

#define ST ((hipStream_t)stream)
#define F4(p) reinterpret_cast<const f32x4*>(p)

extern "C" int nbm_bn_act_plan(int64_t M, int C, int* parts, int64_t* workspace_bytes) {
  if (!parts || !workspace_bytes) return NBM_EINVAL;
  const int rc = bn_check(M, C);
  if (rc != NBM_OK) return rc;
  const BnGeom g = bn_geom(M, C);
  *parts = g.parts;
  *workspace_bytes = bn_ws_bytes(g, C);
  return NBM_OK;
}

extern "C" int nbm_bn_act_train_fwd(const float* z, int64_t M, int C, const float* gamma, const float* beta, float eps, float momentum,
                                    float* run_mean, float* run_var, const float* residual, int relu, void* workspace,
                                    int64_t workspace_bytes, float* mean, float* invstd, float* y, void* stream) {
  if (!z || !gamma || !beta || !workspace || !mean || !invstd || !y || (!run_mean) != (!run_var)) return NBM_EINVAL;
  const int rc = bn_check(M, C);
  if (rc != NBM_OK) return rc;
  if (!nbm_aligned16(z) || !nbm_aligned16(gamma) || !nbm_aligned16(beta) || !nbm_aligned16(workspace) || !nbm_aligned16(mean) ||
      !nbm_aligned16(invstd) || !nbm_aligned16(y) || !nbm_aligned16(residual) || !nbm_aligned16(run_mean) || !nbm_aligned16(run_var))
    return NBM_EALIGN;
  const BnGeom g = bn_geom(M, C);
  if (workspace_bytes < bn_ws_bytes(g, C)) return NBM_EINVAL;
  double* part = (double*)workspace;
  hipLaunchKernelGGL(bn_act_reduce_kernel, dim3(g.parts, g.GY), dim3(BN_TPB), 0, ST, F4(z), (long long)M, C, g.TQ, g.shift, part);
  hipLaunchKernelGGL(bn_act_fwd_finish_kernel, dim3((C + 63) / 64), dim3(BN_TPB), 0, ST, part, g.parts, (long long)M, C, eps, momentum,
                     mean, invstd, run_mean, run_var);
  const dim3 grid(g.apply_wgs, g.GY);
#define BN_APPLY(RELU, RES)                                                                                                     \
  hipLaunchKernelGGL((bn_act_apply_kernel<RELU, RES>), grid, dim3(BN_TPB), 0, ST, F4(z), F4(residual), (long long)M, C, g.TQ, \
                     g.shift, F4(mean), F4(invstd), F4(gamma), F4(beta), reinterpret_cast<f32x4*>(y))
  if (relu) { if (residual) BN_APPLY(true, true); else BN_APPLY(true, false); }
  else { if (residual) BN_APPLY(false, true); else BN_APPLY(false, false); }
#undef BN_APPLY
  return nbm_launch_status();
}

extern "C" int nbm_bn_act_train_bwd(const float* gy, const float* y, const float* z, int64_t M, int C, const float* mean,
                                    const float* invstd, const float* gamma, int relu, void* workspace, int64_t workspace_bytes,
                                    float* gz, float* ggamma, float* gbeta, float* gres, void* stream) {
  if (!gy || !z || !mean || !invstd || !gamma || !workspace || !gz || !ggamma || !gbeta || (relu && !y)) return NBM_EINVAL;
  const int rc = bn_check(M, C);
  if (rc != NBM_OK) return rc;
  if (!nbm_aligned16(gy) || !nbm_aligned16(y) || !nbm_aligned16(z) || !nbm_aligned16(mean) || !nbm_aligned16(invstd) ||
      !nbm_aligned16(gamma) || !nbm_aligned16(workspace) || !nbm_aligned16(gz) || !nbm_aligned16(ggamma) || !nbm_aligned16(gbeta) ||
      !nbm_aligned16(gres))
    return NBM_EALIGN;
  const BnGeom g = bn_geom(M, C);
  if (workspace_bytes < bn_ws_bytes(g, C)) return NBM_EINVAL;
  double* part = (double*)workspace;
  float* tail = (float*)(part + (size_t)g.parts * 2 * C);       // parts * 2 * C * 8 bytes: a multiple of 16 (C % 4 == 0)
  const dim3 rgrid(g.parts, g.GY), agrid(g.apply_wgs, g.GY);
  if (relu)
    hipLaunchKernelGGL((bn_act_bwd_reduce_kernel<true>), rgrid, dim3(BN_TPB), 0, ST, F4(gy), F4(y), F4(z), (long long)M, C, g.TQ,
                       g.shift, F4(mean), F4(invstd), part);
  else
    hipLaunchKernelGGL((bn_act_bwd_reduce_kernel<false>), rgrid, dim3(BN_TPB), 0, ST, F4(gy), F4(y), F4(z), (long long)M, C, g.TQ,
                       g.shift, F4(mean), F4(invstd), part);
  hipLaunchKernelGGL(bn_act_bwd_finish_kernel, dim3((C + 63) / 64), dim3(BN_TPB), 0, ST, part, g.parts, (long long)M, C, tail, ggamma,
                     gbeta);
#define BN_BAPPLY(RELU, GRES)                                                                                                    \
  hipLaunchKernelGGL((bn_act_bwd_apply_kernel<RELU, GRES>), agrid, dim3(BN_TPB), 0, ST, F4(gy), F4(y), F4(z), (long long)M, C,  \
                     g.TQ, g.shift, F4(mean), F4(invstd), F4(gamma), F4(tail), reinterpret_cast<f32x4*>(gz),                    \
                     reinterpret_cast<f32x4*>(gres))
  if (relu) { if (gres) BN_BAPPLY(true, true); else BN_BAPPLY(true, false); }
  else { if (gres) BN_BAPPLY(false, true); else BN_BAPPLY(false, false); }
#undef BN_BAPPLY
  return nbm_launch_status();
}
