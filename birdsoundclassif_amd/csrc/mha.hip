// Multi-head attention of the Transformer_RCNN head (`--tf_rcnn`) over SHORT sequences: S = images per batch or RoIs per image,
// <= MHA_SMAX; head dim <= MHA_HDMAX.  Every attention kernel of the head is here -- evaluation (nbm_mha_small), segmented bulk
// evaluation (nbm_mha_segments), training with and without dropout on the softmax probabilities (nbm_mha_small_drop, the two
// backwards) -- and every one of them gets a query row's arithmetic from one place: mha_row forward, mha_bwd_rows_kernel backward.
// Dropout masks come from the counter generator of nbm_philox.h and are never stored: the backward evaluates them again.
#include <initializer_list>
#include "nbm_common.h"
#include "nbm_philox.h"

#define MHA_SMAX 128      // longest sequence: a score row is MHA_SMAX / 64 values per lane (ops.MHA_SMAX mirrors it)
#define MHA_SHORT 8       // nbm_mha_segments: segments of up to this many images are a wave's own work
#define MHA_HDMAX 64      // head dim: one lane per output column

namespace {

// Dropout on the probabilities: the mask element of (n, h, r, j) is that of a dense [N][nhead][S][S] tensor.
struct MhaDrop {
  uint32_t threshold;
  float drop_scale;
  uint64_t seed;
  uint32_t call, site_id;
};

__device__ __forceinline__ bool mha_keep(const MhaDrop& dr, uint64_t row_base, int j) {
  return nbm_dropout_word(dr.seed, dr.call, dr.site_id, row_base + (uint64_t)j) >= dr.threshold;
}

// One query row by one wave: scores against the nv keys of Kp (keys beyond them masked), softmax, times Vp.
//   DROP = false: psw[j] = e_j, out = (sum_j psw[j] V[j]) / sum
//   DROP = true:  psw[j] = keep ? (e_j / sum) * drop_scale : 0, out = sum_j psw[j] V[j]; row_base: the row's first mask element
// The two forms round differently and each is what its entry point has always computed.
// (hd stays a run-time value: with a constant 64 the unrolled dot product is compiled into packed multiplies and separate
// additions where these are fused multiply-adds, and the last bit moves.)
template <bool DROP>
__device__ __forceinline__ void mha_row(const float* __restrict__ qrow, float* __restrict__ orow, int hd, int nv, float scale,
                                        const float (*Kp)[65], const float (*Vp)[64], float* qsw, float* psw, int lane,
                                        const MhaDrop& dr, uint64_t row_base) {
  if (lane < hd) qsw[lane] = qrow[lane] * scale;
  __builtin_amdgcn_wave_barrier();
  float sc[MHA_SMAX / 64];
  float m = -INFINITY;
#pragma unroll
  for (int t = 0; t < MHA_SMAX / 64; ++t) {
    const int j = lane + 64 * t;
    float a = -INFINITY;
    if (j < nv) {
      a = 0.f;
      for (int d = 0; d < hd; ++d) a += qsw[d] * Kp[j][d];
    }
    sc[t] = a;
    m = fmaxf(m, a);
  }
  m = nbm_wave_max(m);
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < MHA_SMAX / 64; ++t) {
    const int j = lane + 64 * t;
    const float e = j < nv ? expf(sc[t] - m) : 0.f;
    if constexpr (DROP) sc[t] = e;
    else if (j < nv) psw[j] = e;
    sum += e;
  }
  sum = nbm_wave_sum(sum);
  if constexpr (DROP) {
#pragma unroll
    for (int t = 0; t < MHA_SMAX / 64; ++t) {
      const int j = lane + 64 * t;
      if (j < nv) psw[j] = mha_keep(dr, row_base, j) ? (sc[t] / sum) * dr.drop_scale : 0.f;
    }
  }
  __builtin_amdgcn_wave_barrier();
  if (lane < hd) {
    float o = 0.f;
    for (int j = 0; j < nv; ++j) o += psw[j] * Vp[j][lane];
    orow[lane] = DROP ? o : o / sum;
  }
  __builtin_amdgcn_wave_barrier();
}

// nbm_mha_small / nbm_mha_small_drop.  One workgroup per (batch entry n, head); K and V of the group live in LDS, each wave
// owns query rows.  Token (s, n) is row s * seq_stride + n * batch_stride of q/k/v/out; keys >= *n_valid (device counter) are
// masked.  The mask tensor's S is the launch's S, not *n_valid.
template <bool DROP>
__global__ __launch_bounds__(256) void mha_small_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                        const float* __restrict__ v, int q_ld, int k_ld, int v_ld,
                                                        float* __restrict__ out, int out_ld, int S, int nhead, int hd,
                                                        long long seq_stride, long long batch_stride,
                                                        const int* __restrict__ n_valid, float scale, MhaDrop dr) {
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
    mha_row<DROP>(q + row * q_ld + h * hd, out + row * out_ld + h * hd, hd, nv, scale, Ks, Vs, qs[wave], ps[wave], lane, dr,
                  row_base);
  }
}

// Segmented form of mha_small_kernel for the evaluation head with per-image RoI counts (nbm_mha_segments): token (b, r) is
// row b * R + r.  One workgroup per (image b, head) and R query rows of work in each, whatever the segments look like:
//   ACROSS_ROIS    the one sequence of image b, rows b * R + j, j < n_roi[b], K and V staged by the whole workgroup;
//   ACROSS_IMAGES  the sequence of slot r is the images first .. first + cnt - 1 of b's segment (rows (first + j) * R + r) and
//                  exists iff r < n_roi[first].  The cnt images of a segment share its slots out: image first + i takes the
//                  slots i, i + cnt, ... -- cnt query rows each.  cnt <= MHA_SHORT: every wave takes slots of its own and
//                  stages their K and V in its own slice of Ks / Vs (no workgroup barrier; B * R * nhead workgroups of 1 - 4
//                  tokens otherwise); longer: the workgroup stages one slot at a time, as mha_small_kernel does.
// The workgroup of (b, head) also writes the zeros of its image's rows that are no valid token, so every row of `out` is
// written.  A table entry that is not a segment holding b within [0, B) with cnt <= max_count makes b's rows zero.
// Rows go through mha_row<false>, as nbm_mha_small's do: a segment's results are the bits nbm_mha_small gives on it alone.
__global__ __launch_bounds__(256) void mha_segments_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                           const float* __restrict__ v, int q_ld, int k_ld, int v_ld,
                                                           float* __restrict__ out, int out_ld, int B, int R, int nhead,
                                                           int hd, int mode, const int* __restrict__ segments,
                                                           const int* __restrict__ n_roi, int max_count, float scale) {
  __shared__ float Ks[MHA_SMAX][65];
  __shared__ float Vs[MHA_SMAX][64];
  __shared__ float qs[4][64];
  __shared__ float ps[4][MHA_SMAX];
  const int b = blockIdx.x / nhead, h = blockIdx.x - b * nhead;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long col = (long long)h * hd;
  const MhaDrop none = {};
  int first = b, cnt = 1;
  bool ok = true;
  if (mode == NBM_MHA_ACROSS_IMAGES) {
    first = segments[b];
    cnt = segments[B + b];
    ok = first >= 0 && first <= b && cnt >= 1 && cnt <= max_count && b - first < cnt && first + cnt <= B;
  }
  const int n = ok ? min(max(n_roi[first], 0), R) : 0;
  for (int r = n + wave; r < R; r += 4)
    if (lane < hd) out[((long long)b * R + r) * out_ld + col + lane] = 0.f;
  if (mode == NBM_MHA_ACROSS_ROIS) {
    const long long row0 = (long long)b * R;
    for (int i = threadIdx.x; i < n * hd; i += 256) {
      const int j = i / hd, d = i - j * hd;
      Ks[j][d] = k[(row0 + j) * k_ld + col + d];
      Vs[j][d] = v[(row0 + j) * v_ld + col + d];
    }
    __syncthreads();
    for (int r = wave; r < n; r += 4)
      mha_row<false>(q + (row0 + r) * q_ld + col, out + (row0 + r) * out_ld + col, hd, n, scale, Ks, Vs, qs[wave], ps[wave],
                     lane, none, 0);
    return;
  }
  const int me = b - first;
  if (cnt <= MHA_SHORT) {
    float(*Kw)[65] = Ks + wave * MHA_SHORT;
    float(*Vw)[64] = Vs + wave * MHA_SHORT;
    for (int r = me + wave * cnt; r < n; r += 4 * cnt) {
      if (lane < hd)
        for (int j = 0; j < cnt; ++j) {
          const long long row = (long long)(first + j) * R + r;
          Kw[j][lane] = k[row * k_ld + col + lane];
          Vw[j][lane] = v[row * v_ld + col + lane];
        }
      __builtin_amdgcn_wave_barrier();
      for (int i = 0; i < cnt; ++i) {
        const long long row = (long long)(first + i) * R + r;
        mha_row<false>(q + row * q_ld + col, out + row * out_ld + col, hd, cnt, scale, Kw, Vw, qs[wave], ps[wave], lane, none,
                       0);
      }
    }
    return;
  }
  for (int r = me; r < n; r += cnt) {                       // r, n, cnt are uniform over the workgroup: so are the barriers
    __syncthreads();
    for (int i = threadIdx.x; i < cnt * hd; i += 256) {
      const int j = i / hd, d = i - j * hd;
      const long long row = (long long)(first + j) * R + r;
      Ks[j][d] = k[row * k_ld + col + d];
      Vs[j][d] = v[row * v_ld + col + d];
    }
    __syncthreads();
    for (int i = wave; i < cnt; i += 4) {
      const long long row = (long long)(first + i) * R + r;
      mha_row<false>(q + row * q_ld + col, out + row * out_ld + col, hd, cnt, scale, Ks, Vs, qs[wave], ps[wave], lane, none, 0);
    }
  }
}

// Backward of nbm_mha_small / nbm_mha_small_drop (same token layout).  Pass 1, a wave per query row: recompute the probabilities
// P (and the mask), dA = dO V^T, dP = keep ? dA * drop_scale : 0, dS = P (dP - sum(P dP)), dQ = scale dS K.  The workspace gets
// A = keep ? P * drop_scale : 0 (for dV = A^T dO) and dS; without dropout keep is true, drop_scale is absent and A = P.
template <bool DROP>
__global__ __launch_bounds__(256) void mha_bwd_rows_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, const float* __restrict__ go,
    int q_ld, int k_ld, int v_ld, int go_ld, float* __restrict__ gq, int gq_ld, float* __restrict__ ws, int S, int nhead,
    int hd, long long seq_stride, long long batch_stride, const int* __restrict__ n_valid, float scale, MhaDrop dr) {
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
        keep[t] = DROP ? mha_keep(dr, row_base, j) : true;
      }
      sc[t] = a;
      dp[t] = !DROP ? b : keep[t] ? b * dr.drop_scale : 0.f;
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
        A[(long long)r * S + j] = !DROP ? sc[t] : keep[t] ? sc[t] * dr.drop_scale : 0.f;
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
__global__ __launch_bounds__(256) void mha_bwd_keys_kernel(
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

// What the four nbm_mha_small* entry points ask of their geometry; pitches: every row pitch passed, each >= nhead * hd.
bool mha_small_geometry_ok(int S, int N, int nhead, int hd, std::initializer_list<int> pitches) {
  if (S <= 0 || S > MHA_SMAX || N <= 0 || nhead <= 0 || hd <= 0 || hd > MHA_HDMAX) return false;
  for (int ld : pitches)
    if (ld < nhead * hd) return false;
  return true;
}

template <bool DROP>
int mha_small_launch(const float* q, const float* k, const float* v, int q_ld, int k_ld, int v_ld, float* out, int out_ld, int S,
                     int N, int nhead, int hd, int64_t seq_stride, int64_t batch_stride, const int32_t* n_valid, float scale,
                     const MhaDrop& dr, void* stream) {
  if (!q || !k || !v || !out || !mha_small_geometry_ok(S, N, nhead, hd, {q_ld, k_ld, v_ld, out_ld})) return NBM_EINVAL;
  hipLaunchKernelGGL(mha_small_kernel<DROP>, dim3(N * nhead), dim3(256), 0, (hipStream_t)stream, q, k, v, q_ld, k_ld, v_ld, out,
                     out_ld, S, nhead, hd, (long long)seq_stride, (long long)batch_stride, n_valid, scale, dr);
  return nbm_launch_status();
}

template <bool DROP>
int mha_small_bwd_launch(const float* q, const float* k, const float* v, const float* go, int q_ld, int k_ld, int v_ld,
                         int go_ld, float* gq, float* gk, float* gv, int gq_ld, int gk_ld, int gv_ld, float* workspace, int S,
                         int N, int nhead, int hd, int64_t seq_stride, int64_t batch_stride, const int32_t* n_valid, float scale,
                         const MhaDrop& dr, void* stream) {
  if (!q || !k || !v || !go || !gq || !gk || !gv || !workspace) return NBM_EINVAL;
  if (!mha_small_geometry_ok(S, N, nhead, hd, {q_ld, k_ld, v_ld, go_ld, gq_ld, gk_ld, gv_ld})) return NBM_EINVAL;
  hipLaunchKernelGGL(mha_bwd_rows_kernel<DROP>, dim3(N * nhead), dim3(256), 0, (hipStream_t)stream, q, k, v, go, q_ld, k_ld,
                     v_ld, go_ld, gq, gq_ld, workspace, S, nhead, hd, (long long)seq_stride, (long long)batch_stride, n_valid,
                     scale, dr);
  hipLaunchKernelGGL(mha_bwd_keys_kernel, dim3(N * nhead), dim3(256), 0, (hipStream_t)stream, q, go, q_ld, go_ld, workspace, gk,
                     gv, gk_ld, gv_ld, S, nhead, hd, (long long)seq_stride, (long long)batch_stride, n_valid, scale);
  return nbm_launch_status();
}

}  // namespace

extern "C" int nbm_mha_small(const float* q, const float* k, const float* v, int q_ld, int k_ld, int v_ld, float* out,
                             int out_ld, int S, int N, int nhead, int hd, int64_t seq_stride, int64_t batch_stride,
                             const int32_t* n_valid, float scale, void* stream) {
  return mha_small_launch<false>(q, k, v, q_ld, k_ld, v_ld, out, out_ld, S, N, nhead, hd, seq_stride, batch_stride, n_valid,
                                 scale, MhaDrop{}, stream);
}

extern "C" int nbm_mha_small_drop(const float* q, const float* k, const float* v, int q_ld, int k_ld, int v_ld, float* out,
                                  int out_ld, int S, int N, int nhead, int hd, int64_t seq_stride, int64_t batch_stride,
                                  const int32_t* n_valid, float scale, uint32_t threshold, float drop_scale, uint64_t seed,
                                  uint32_t call, uint32_t site_id, void* stream) {
  return mha_small_launch<true>(q, k, v, q_ld, k_ld, v_ld, out, out_ld, S, N, nhead, hd, seq_stride, batch_stride, n_valid,
                                scale, MhaDrop{threshold, drop_scale, seed, call, site_id}, stream);
}

extern "C" int nbm_mha_small_bwd(const float* q, const float* k, const float* v, const float* go, int q_ld, int k_ld,
                                 int v_ld, int go_ld, float* gq, float* gk, float* gv, int gq_ld, int gk_ld, int gv_ld,
                                 float* workspace, int S, int N, int nhead, int hd, int64_t seq_stride,
                                 int64_t batch_stride, const int32_t* n_valid, float scale, void* stream) {
  return mha_small_bwd_launch<false>(q, k, v, go, q_ld, k_ld, v_ld, go_ld, gq, gk, gv, gq_ld, gk_ld, gv_ld, workspace, S, N,
                                     nhead, hd, seq_stride, batch_stride, n_valid, scale, MhaDrop{}, stream);
}

extern "C" int nbm_mha_small_drop_bwd(const float* q, const float* k, const float* v, const float* go, int q_ld, int k_ld,
                                      int v_ld, int go_ld, float* gq, float* gk, float* gv, int gq_ld, int gk_ld, int gv_ld,
                                      float* workspace, int S, int N, int nhead, int hd, int64_t seq_stride,
                                      int64_t batch_stride, const int32_t* n_valid, float scale, uint32_t threshold,
                                      float drop_scale, uint64_t seed, uint32_t call, uint32_t site_id, void* stream) {
  return mha_small_bwd_launch<true>(q, k, v, go, q_ld, k_ld, v_ld, go_ld, gq, gk, gv, gq_ld, gk_ld, gv_ld, workspace, S, N,
                                    nhead, hd, seq_stride, batch_stride, n_valid, scale,
                                    MhaDrop{threshold, drop_scale, seed, call, site_id}, stream);
}

extern "C" int nbm_mha_segments(const float* q, const float* k, const float* v, int q_ld, int k_ld, int v_ld, float* out,
                                int out_ld, int B, int R, int nhead, int hd, int mode, const int32_t* segments,
                                const int32_t* n_roi, int max_count, float scale, void* stream) {
  if (!q || !k || !v || !out || !n_roi || B <= 0 || R <= 0 || nhead <= 0 || hd <= 0 || hd > MHA_HDMAX) return NBM_EINVAL;
  if (q_ld < nhead * hd || k_ld < nhead * hd || v_ld < nhead * hd || out_ld < nhead * hd) return NBM_EINVAL;
  if (mode == NBM_MHA_ACROSS_ROIS) {
    if (R > MHA_SMAX) return NBM_EINVAL;
  } else if (mode == NBM_MHA_ACROSS_IMAGES) {
    if (!segments || max_count < 1 || max_count > MHA_SMAX) return NBM_EINVAL;
  } else {
    return NBM_EINVAL;
  }
  hipLaunchKernelGGL(mha_segments_kernel, dim3(B * nhead), dim3(256), 0, (hipStream_t)stream, q, k, v, q_ld, k_ld, v_ld, out,
                     out_ld, B, R, nhead, hd, mode, segments, n_roi, max_count, scale);
  return nbm_launch_status();
}
