// Multi-head attention of the Transformer_RCNN head (`--tf_rcnn`): S = images per batch or RoIs per image, head dim <= MHA_HDWIDE.
// SHORT sequences, S <= MHA_SMAX: one lane per output column up to MHA_HDMAX, the chunked wide kernels above it; LONG sequences,
// MHA_SMAX < S <= MHA_SLONG (RoIs per image only): K and V in blocks of MHA_SMAX keys through LDS, the score rows in LDS, any head
// dim.  The host launchers choose, on the launch's S and hd, and nbm_mha_plan reports the choice.  Every attention kernel of the head is here -- evaluation (nbm_mha_small), segmented bulk
// evaluation (nbm_mha_segments, which keeps its limit of MHA_HDMAX, and nbm_mha_segments_wide), training with and without
// dropout on the softmax probabilities (nbm_mha_small_drop, the two backwards) -- and every one of them gets a query row's arithmetic from one place: mha_row forward, mha_bwd_rows_kernel backward
// (mha_wide_rows and mha_wide_bwd_rows_kernel for the wide heads, mha_long_rows and mha_long_bwd_rows_kernel for the long sequences).
// Dropout masks come from the counter generator of nbm_philox.h and are never stored: the backward evaluates them again.
#include <initializer_list>
#include "nbm_common.h"
#include "nbm_philox.h"

#define MHA_SMAX 128      // longest sequence of the short kernels: a score row is MHA_SMAX / 64 values per lane (ops.MHA_SMAX mirrors it)
#define MHA_SLONG 1024    // longest sequence of the long kernels: score rows wait in LDS (ops.MHA_SLONG mirrors it)
#ifndef MHA_LROWS         // for scripts/bench_tf_long.py --alt_root only: -DMHA_LROWS=4 builds the 16-row block that DESIGN 4u measures
                          // against this one and drops; the suite pins 2 (tests/test_mha_plan_cpu.py)
#define MHA_LROWS 2       // long kernels: query rows a wave carries through the key blocks ...
#endif
#define MHA_LBLOCK (4 * MHA_LROWS)  // ... and a workgroup: 8
#define MHA_LKEYS 8       // long backward, pass 2: consecutive keys a wave accumulates
#define MHA_SHORT 8       // nbm_mha_segments: segments of up to this many images are a wave's own work
#define MHA_HDMAX 64      // head dim of the narrow kernels: one lane per output column
#define MHA_HDWIDE 512    // head dim of the wide kernels: 64-column chunks of K and V pass through LDS
#define MHA_WROWS 8       // wide kernels: query rows a wave carries through the chunks ...
#define MHA_WBLOCK 32     // ... and a workgroup
#define MHA_KEYBLOCKS 4   // wide backward, pass 2: sets of key rows per (entry, head, chunk)

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

// LDS of the narrow kernels: K and V of one (entry, head) whole, and per wave a query row (and dO row) and a score row.  The
// kernels declare their arrays with these types, one __shared__ array each as they always did (held together in one struct the
// same kernels' launches ran 5 % slower in training and 18 % in evaluation: profiles/tf_long_struct_control.txt), and nbm_mha_plan adds up
// the same types -- an array added to a kernel has to be added to the sums below.
typedef float MhaNarrowK[MHA_SMAX][65];
typedef float MhaNarrowV[MHA_SMAX][64];
typedef float MhaNarrowRow[4][64];
typedef float MhaNarrowScores[4][MHA_SMAX];
constexpr int MHA_NARROW_LDS = sizeof(MhaNarrowK) + sizeof(MhaNarrowV) + sizeof(MhaNarrowRow) + sizeof(MhaNarrowScores);
constexpr int MHA_NARROW_BWD_LDS = 2 * sizeof(MhaNarrowK) + 2 * sizeof(MhaNarrowRow) + sizeof(MhaNarrowScores);

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
  __shared__ MhaNarrowK Ks;
  __shared__ MhaNarrowV Vs;
  __shared__ MhaNarrowRow qs;
  __shared__ MhaNarrowScores ps;
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
  __shared__ MhaNarrowK Ks;
  __shared__ MhaNarrowV Vs;
  __shared__ MhaNarrowRow qs;
  __shared__ MhaNarrowScores ps;
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
  __shared__ MhaNarrowK Ks;
  __shared__ MhaNarrowK Vs;
  __shared__ MhaNarrowRow qs;
  __shared__ MhaNarrowRow gs;
  __shared__ MhaNarrowScores ds;
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

// --------------------------------------------------------------------------------- wide heads: MHA_HDMAX < hd <= MHA_HDWIDE
// K and V of one (entry, head) no longer fit LDS whole (2 x 128 x 512 x 4 bytes at the limit), so the head dimension is staged
// in chunks of 64 columns and the probabilities of a block of query rows wait in LDS between the two products.  A wave carries
// MHA_WROWS query rows through every chunk -- one LDS read of K[j][d] or V[j][c] serves all of them -- and a workgroup a block of
// MHA_WBLOCK.  As on the narrow path every entry point gets a query row's arithmetic from one place (mha_wide_dots, the softmax
// of mha_wide_rows, mha_wide_pv; the backward's softmax in mha_wide_bwd_rows_kernel), and every product-sum is an explicit fmaf
// chain in ascending d or j: the bits of a row depend neither on the chunking nor on which wave, block or kernel computed it.
static_assert(MHA_SHORT <= MHA_WROWS && MHA_WBLOCK == 4 * MHA_WROWS && MHA_SMAX % 64 == 0, "wide attention: a wave's rows");

struct MhaWideLds {
  float Y[MHA_SMAX][65];                  // the current 64-column chunk of K or V, one row per key
  float x[MHA_WBLOCK][64];                // the same chunk of the query-side rows (q * scale, or dO); wave w owns rows 8w .. 8w + 7
  float P[MHA_WBLOCK][MHA_SMAX];          // forward: the probabilities of those rows; backward: dS
};

// A sequence: key / query j is row off + j * stride of every operand, nv of them.
struct MhaSeq {
  long long off, stride;
  int nv;
};

// WG = true: the workgroup stages Y (all of it) and shares it; false: the wave stages its own sequence of <= MHA_SHORT keys in
// its MHA_WROWS-row slice of Y and meets no workgroup barrier.
template <bool WG>
__device__ __forceinline__ void mha_wide_sync() {
  if constexpr (WG) __syncthreads();
  else __builtin_amdgcn_wave_barrier();
}

template <bool WG>
__device__ __forceinline__ void mha_wide_stage(float (*Y)[65], const float* __restrict__ src, int ld, long long col, int dn,
                                               const MhaSeq& sq) {
  for (int i = WG ? threadIdx.x : (threadIdx.x & 63); i < sq.nv * 64; i += WG ? 256 : 64) {
    const int j = i >> 6, d = i & 63;
    if (d < dn) Y[j][d] = src[(sq.off + j * sq.stride) * ld + col + d];
  }
}

// acc[i][t] += sum_d (xsrc[query rw0 + i][d] * xmul) * ysrc[key lane + 64 t][d] over the whole head dimension.
template <bool WG>
__device__ __forceinline__ void mha_wide_dots(float (&acc)[MHA_WROWS][MHA_SMAX / 64], const float* __restrict__ xsrc, int x_ld,
                                              float xmul, const float* __restrict__ ysrc, int y_ld, long long col, int hd,
                                              const MhaSeq& sq, int rw0, MhaWideLds& L, float (*Y)[65]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float(*xw)[64] = L.x + wave * MHA_WROWS;
  for (int c0 = 0; c0 < hd; c0 += 64) {
    const int dn = min(64, hd - c0);
    mha_wide_sync<WG>();                                    // the last readers of Y and x are done
    mha_wide_stage<WG>(Y, ysrc, y_ld, col + c0, dn, sq);
#pragma unroll
    for (int i = 0; i < MHA_WROWS; ++i) {
      const int r = rw0 + i;
      xw[i][lane] = (r < sq.nv && lane < dn) ? xsrc[(sq.off + r * sq.stride) * x_ld + col + c0 + lane] * xmul : 0.f;
    }
    mha_wide_sync<WG>();
#pragma unroll
    for (int t = 0; t < MHA_SMAX / 64; ++t) {
      const int j = lane + 64 * t;
      if (j < sq.nv)
        for (int d = 0; d < dn; ++d) {
          const float y = Y[j][d];
#pragma unroll
          for (int i = 0; i < MHA_WROWS; ++i) acc[i][t] = fmaf(xw[i][d], y, acc[i][t]);
        }
    }
  }
}

// put(i, c, sum_j P[query rw0 + i][j] * ysrc[key j][c]) for the wave's rows i and every column c < hd.
template <bool WG, class Put>
__device__ __forceinline__ void mha_wide_pv(const float* __restrict__ ysrc, int y_ld, long long col, int hd, const MhaSeq& sq,
                                            MhaWideLds& L, float (*Y)[65], Put&& put) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float(*Pw)[MHA_SMAX] = L.P + wave * MHA_WROWS;
  for (int c0 = 0; c0 < hd; c0 += 64) {
    const int dn = min(64, hd - c0);
    mha_wide_sync<WG>();
    mha_wide_stage<WG>(Y, ysrc, y_ld, col + c0, dn, sq);
    mha_wide_sync<WG>();
    if (lane < dn) {
      float o[MHA_WROWS] = {};
      for (int j = 0; j < sq.nv; ++j) {
        const float y = Y[j][lane];
#pragma unroll
        for (int i = 0; i < MHA_WROWS; ++i) o[i] = fmaf(Pw[i][j], y, o[i]);
      }
#pragma unroll
      for (int i = 0; i < MHA_WROWS; ++i) put(i, c0 + lane, o[i]);
    }
  }
}

// The queries rw0 .. rw0 + MHA_WROWS - 1 of sequence sq by one wave, in the two forms of mha_row.  mask_base: the first mask
// element of the sequence's (entry, head); mask_S: the mask tensor's S.
template <bool DROP, bool WG>
__device__ __forceinline__ void mha_wide_rows(const float* __restrict__ q, const float* __restrict__ k,
                                              const float* __restrict__ v, int q_ld, int k_ld, int v_ld, float* __restrict__ out,
                                              int out_ld, long long col, int hd, const MhaSeq& sq, int rw0, float scale,
                                              const MhaDrop& dr, uint64_t mask_base, int mask_S, MhaWideLds& L, float (*Y)[65]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float(*Pw)[MHA_SMAX] = L.P + wave * MHA_WROWS;
  float acc[MHA_WROWS][MHA_SMAX / 64] = {};
  mha_wide_dots<WG>(acc, q, q_ld, scale, k, k_ld, col, hd, sq, rw0, L, Y);
  float sum[MHA_WROWS];
#pragma unroll
  for (int i = 0; i < MHA_WROWS; ++i) {
    const int r = rw0 + i;
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < MHA_SMAX / 64; ++t) m = fmaxf(m, lane + 64 * t < sq.nv ? acc[i][t] : -INFINITY);
    m = nbm_wave_max(m);
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < MHA_SMAX / 64; ++t) {
      acc[i][t] = lane + 64 * t < sq.nv ? expf(acc[i][t] - m) : 0.f;
      s += acc[i][t];
    }
    s = nbm_wave_sum(s);
    sum[i] = s;
    const uint64_t row_base = mask_base + (uint64_t)r * (uint64_t)mask_S;
#pragma unroll
    for (int t = 0; t < MHA_SMAX / 64; ++t) {
      const int j = lane + 64 * t;
      if (j < sq.nv && r < sq.nv) {
        if constexpr (DROP) Pw[i][j] = mha_keep(dr, row_base, j) ? (acc[i][t] / s) * dr.drop_scale : 0.f;
        else Pw[i][j] = acc[i][t];
      }
    }
  }
  mha_wide_pv<WG>(v, v_ld, col, hd, sq, L, Y, [&](int i, int c, float o) {
    const int r = rw0 + i;
    if (r < sq.nv) out[(sq.off + r * sq.stride) * out_ld + col + c] = DROP ? o : o / sum[i];
  });
}

// nbm_mha_small / nbm_mha_small_drop, wide: one workgroup per (batch entry n, head) and block of MHA_WBLOCK query rows.
template <bool DROP>
__global__ __launch_bounds__(256) void mha_wide_small_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                             const float* __restrict__ v, int q_ld, int k_ld, int v_ld,
                                                             float* __restrict__ out, int out_ld, int S, int nhead, int hd,
                                                             long long seq_stride, long long batch_stride,
                                                             const int* __restrict__ n_valid, float scale, MhaDrop dr) {
  __shared__ MhaWideLds L;
  const int n = blockIdx.x / nhead, h = blockIdx.x - n * nhead;
  const int nv = n_valid ? min(*n_valid, S) : S;
  const int r0 = blockIdx.y * MHA_WBLOCK;
  if (r0 >= nv) return;
  const MhaSeq sq = {n * batch_stride, seq_stride, nv};
  mha_wide_rows<DROP, true>(q, k, v, q_ld, k_ld, v_ld, out, out_ld, (long long)h * hd, hd, sq,
                            r0 + (int)(threadIdx.x >> 6) * MHA_WROWS, scale, dr, (uint64_t)blockIdx.x * (uint64_t)S * (uint64_t)S,
                            S, L, L.Y);
}

// nbm_mha_segments, wide: mha_segments_kernel's division of the work -- a workgroup per (image b, head), in ACROSS_ROIS times a
// block of query rows -- with the rows going through mha_wide_rows<false>, as the wide nbm_mha_small's do.
__global__ __launch_bounds__(256) void mha_wide_segments_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                const float* __restrict__ v, int q_ld, int k_ld, int v_ld,
                                                                float* __restrict__ out, int out_ld, int B, int R, int nhead,
                                                                int hd, int mode, const int* __restrict__ segments,
                                                                const int* __restrict__ n_roi, int max_count, float scale) {
  __shared__ MhaWideLds L;
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
  for (int r = n + wave + 4 * (int)blockIdx.y; r < R; r += 4 * (int)gridDim.y)
    for (int c = lane; c < hd; c += 64) out[((long long)b * R + r) * out_ld + col + c] = 0.f;
  if (mode == NBM_MHA_ACROSS_ROIS) {
    const MhaSeq sq = {(long long)b * R, 1, n};
    for (int r0 = blockIdx.y * MHA_WBLOCK; r0 < n; r0 += gridDim.y * MHA_WBLOCK)
      mha_wide_rows<false, true>(q, k, v, q_ld, k_ld, v_ld, out, out_ld, col, hd, sq, r0 + wave * MHA_WROWS, scale, none, 0, 0, L,
                                 L.Y);
    return;
  }
  const int me = b - first;
  if (cnt <= MHA_SHORT) {                                   // a slot's cnt queries are one wave's rows
    for (int r = me + wave * cnt; r < n; r += 4 * cnt) {
      const MhaSeq sq = {(long long)first * R + r, R, cnt};
      mha_wide_rows<false, false>(q, k, v, q_ld, k_ld, v_ld, out, out_ld, col, hd, sq, 0, scale, none, 0, 0, L,
                                  L.Y + wave * MHA_WROWS);
    }
    return;
  }
  for (int r = me; r < n; r += cnt) {                       // r, n, cnt are uniform over the workgroup: so are the barriers
    const MhaSeq sq = {(long long)first * R + r, R, cnt};
    for (int r0 = 0; r0 < cnt; r0 += MHA_WBLOCK)
      mha_wide_rows<false, true>(q, k, v, q_ld, k_ld, v_ld, out, out_ld, col, hd, sq, r0 + wave * MHA_WROWS, scale, none, 0, 0, L,
                                 L.Y);
  }
}

// Pass 1 of the backward, wide: mha_bwd_rows_kernel's quantities for a block of MHA_WBLOCK query rows.  The scores and dA
// accumulate over the chunks of K and of V; dQ leaves chunk by chunk.
template <bool DROP>
__global__ __launch_bounds__(256) void mha_wide_bwd_rows_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, const float* __restrict__ go,
    int q_ld, int k_ld, int v_ld, int go_ld, float* __restrict__ gq, int gq_ld, float* __restrict__ ws, int S, int nhead,
    int hd, long long seq_stride, long long batch_stride, const int* __restrict__ n_valid, float scale, MhaDrop dr) {
  __shared__ MhaWideLds L;
  const int n = blockIdx.x / nhead, h = blockIdx.x - n * nhead;
  const int nv = n_valid ? min(*n_valid, S) : S;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if ((int)blockIdx.y * MHA_WBLOCK >= nv) return;
  const int rw0 = blockIdx.y * MHA_WBLOCK + wave * MHA_WROWS;
  const long long col = (long long)h * hd;
  const MhaSeq sq = {n * batch_stride, seq_stride, nv};
  float(*Pw)[MHA_SMAX] = L.P + wave * MHA_WROWS;
  float* A = ws + (long long)blockIdx.x * 2 * S * S;
  float* D = A + (long long)S * S;
  float sc[MHA_WROWS][MHA_SMAX / 64] = {}, dp[MHA_WROWS][MHA_SMAX / 64] = {};
  mha_wide_dots<true>(sc, q, q_ld, scale, k, k_ld, col, hd, sq, rw0, L, L.Y);
  mha_wide_dots<true>(dp, go, go_ld, 1.f, v, v_ld, col, hd, sq, rw0, L, L.Y);
#pragma unroll
  for (int i = 0; i < MHA_WROWS; ++i) {
    const int r = rw0 + i;
    const uint64_t row_base = ((uint64_t)blockIdx.x * (uint64_t)S + (uint64_t)r) * (uint64_t)S;
    bool keep[MHA_SMAX / 64];
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < MHA_SMAX / 64; ++t) {
      const int j = lane + 64 * t;
      keep[t] = j < nv && r < nv && (DROP ? mha_keep(dr, row_base, j) : true);
      if constexpr (DROP) dp[i][t] = keep[t] ? dp[i][t] * dr.drop_scale : 0.f;
      m = fmaxf(m, j < nv ? sc[i][t] : -INFINITY);
    }
    m = nbm_wave_max(m);
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < MHA_SMAX / 64; ++t) {
      sc[i][t] = (lane + 64 * t < nv) ? expf(sc[i][t] - m) : 0.f;
      sum += sc[i][t];
    }
    sum = nbm_wave_sum(sum);
    float dot = 0.f;
#pragma unroll
    for (int t = 0; t < MHA_SMAX / 64; ++t) { sc[i][t] /= sum; dot = fmaf(sc[i][t], dp[i][t], dot); }
    dot = nbm_wave_sum(dot);
#pragma unroll
    for (int t = 0; t < MHA_SMAX / 64; ++t) {
      const int j = lane + 64 * t;
      if (j < nv && r < nv) {
        const float dsv = sc[i][t] * (dp[i][t] - dot);
        Pw[i][j] = dsv;
        A[(long long)r * S + j] = !DROP ? sc[i][t] : keep[t] ? sc[i][t] * dr.drop_scale : 0.f;
        D[(long long)r * S + j] = dsv;
      }
    }
  }
  mha_wide_pv<true>(k, k_ld, col, hd, sq, L, L.Y, [&](int i, int c, float o) {
    const int r = rw0 + i;
    if (r < nv) gq[(sq.off + r * sq.stride) * gq_ld + col + c] = o * scale;
  });
}

// Pass 2, wide: mha_bwd_keys_kernel with the columns and the key rows spread over the grid -- (entry, head) x 64-column chunk
// x MHA_KEYBLOCKS interleaved sets of key rows.
__global__ __launch_bounds__(256) void mha_wide_bwd_keys_kernel(
    const float* __restrict__ q, const float* __restrict__ go, int q_ld, int go_ld, const float* __restrict__ ws,
    float* __restrict__ gk, float* __restrict__ gv, int gk_ld, int gv_ld, int S, int nhead, int hd, long long seq_stride,
    long long batch_stride, const int* __restrict__ n_valid, float scale) {
  const int n = blockIdx.x / nhead, h = blockIdx.x - n * nhead;
  const int nv = n_valid ? min(*n_valid, S) : S;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* A = ws + (long long)blockIdx.x * 2 * S * S;
  const float* D = A + (long long)S * S;
  const int c = blockIdx.y * 64 + lane;
  if (c >= hd) return;
  for (int j = blockIdx.z * 4 + wave; j < nv; j += 4 * MHA_KEYBLOCKS) {
    float ak = 0.f, av = 0.f;
    for (int r = 0; r < nv; ++r) {
      const long long row = r * seq_stride + n * batch_stride;
      ak = fmaf(D[(long long)r * S + j], q[row * q_ld + h * hd + c], ak);
      av = fmaf(A[(long long)r * S + j], go[row * go_ld + h * hd + c], av);
    }
    const long long rowj = j * seq_stride + n * batch_stride;
    gk[rowj * gk_ld + h * hd + c] = ak * scale;
    gv[rowj * gv_ld + h * hd + c] = av;
  }
}

// ------------------------------------------------------------------------ long sequences: MHA_SMAX < S <= MHA_SLONG, any hd
// Neither the keys of a sequence nor a lane's share of a score row fit where the two families above keep them, so K and V pass
// through LDS in blocks of MHA_SMAX keys by 64-column chunks and the score rows of a block of queries wait in LDS whole
// (P[MHA_LBLOCK][MHA_SLONG], 32 KiB; with the staging chunk 66.5 KiB: two workgroups per CU).  A wave carries MHA_LROWS query rows
// -- one LDS read of K[j][d] / V[j][c] serves all of them -- and a workgroup MHA_LBLOCK.  The softmax is the plain one over the
// complete row (mha_long_softmax), so a row's arithmetic is that of mha_row / mha_wide_rows with more values per lane and does
// not know the blocking: score j is an fmaf chain in ascending d, a lane adds its e_j for j = lane + 64 t in ascending t, output
// column c is the chain over ascending j.  The staged tile is zero outside the block's keys and the chunk's columns, a row of P
// up to the next multiple of four keys, which lets the inner loops read their broadcast operand 16 bytes at a time: fmaf(0, 0, a) == a.
// Every forward entry point gets its rows from mha_long_rows; the backward's pass 1 shares the products and the softmax with it.
static_assert(MHA_SLONG % MHA_SMAX == 0 && MHA_SMAX == 128, "long attention: blocks of 128 keys");

struct __attribute__((aligned(16))) MhaLongLds {
  float P[MHA_LBLOCK][MHA_SLONG];         // forward: raw scores, then e_j or the dropped probabilities; backward: then dS
  float x[MHA_LBLOCK][64];                // the current chunk of the query-side rows (q * scale, or dO); wave w owns MHA_LROWS of them
  float Y[MHA_SMAX][65];                  // the current block of keys by 64-column chunk of K or V
};

// Y[j][d] = src[key j of blk][col + d] for j < blk.nv, d < dn; zeros in every other row and column of Y, so that the lanes and the
// steps of four beyond a short last block multiply zeros.
__device__ __forceinline__ void mha_long_stage(float (*Y)[65], const float* __restrict__ src, int ld, long long col, int dn,
                                               const MhaSeq& blk) {
  for (int i = threadIdx.x; i < MHA_SMAX * 64; i += 256) {
    const int j = i >> 6, d = i & 63;
    Y[j][d] = (j < blk.nv && d < dn) ? src[(blk.off + j * blk.stride) * ld + col + d] : 0.f;
  }
}

// put(i, j, sum_d (xsrc[query rw0 + i][d] * xmul) * ysrc[key j][d]) for the wave's rows i and every key j < sq.nv.
template <class Put>
__device__ __forceinline__ void mha_long_dots(const float* __restrict__ xsrc, int x_ld, float xmul,
                                              const float* __restrict__ ysrc, int y_ld, long long col, int hd, const MhaSeq& sq,
                                              int rw0, MhaLongLds& L, Put&& put) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float(*xw)[64] = L.x + wave * MHA_LROWS;
  for (int j0 = 0; j0 < sq.nv; j0 += MHA_SMAX) {
    const MhaSeq blk = {sq.off + j0 * sq.stride, sq.stride, min(MHA_SMAX, sq.nv - j0)};
    const bool two = blk.nv > 64;                           // uniform: the block has keys for the lanes' second value
    float acc[MHA_LROWS][2] = {};
    for (int c0 = 0; c0 < hd; c0 += 64) {
      const int dn = min(64, hd - c0);
      __syncthreads();                                      // the last readers of Y and x are done
      mha_long_stage(L.Y, ysrc, y_ld, col + c0, dn, blk);
#pragma unroll
      for (int i = 0; i < MHA_LROWS; ++i) {
        const int r = rw0 + i;
        xw[i][lane] = (r < sq.nv && lane < dn) ? xsrc[(sq.off + r * sq.stride) * x_ld + col + c0 + lane] * xmul : 0.f;
      }
      __syncthreads();
      for (int d = 0; d < dn; d += 4) {
        float xv[MHA_LROWS][4];
#pragma unroll
        for (int i = 0; i < MHA_LROWS; ++i) {
          const float4 x4 = *reinterpret_cast<const float4*>(&xw[i][d]);
          xv[i][0] = x4.x; xv[i][1] = x4.y; xv[i][2] = x4.z; xv[i][3] = x4.w;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float y0 = L.Y[lane][d + e];
#pragma unroll
          for (int i = 0; i < MHA_LROWS; ++i) acc[i][0] = fmaf(xv[i][e], y0, acc[i][0]);
          if (two) {
            const float y1 = L.Y[lane + 64][d + e];
#pragma unroll
            for (int i = 0; i < MHA_LROWS; ++i) acc[i][1] = fmaf(xv[i][e], y1, acc[i][1]);
          }
        }
      }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int j = j0 + lane + 64 * t;
      if (j < sq.nv)
#pragma unroll
        for (int i = 0; i < MHA_LROWS; ++i) put(i, j, acc[i][t]);
    }
  }
}

// put(i, c, sum_j P[query rw0 + i][j] * ysrc[key j][c]) for the wave's rows i and every column c < hd; P is zero in
// [sq.nv, next multiple of four).
template <class Put>
__device__ __forceinline__ void mha_long_pv(const float* __restrict__ ysrc, int y_ld, long long col, int hd, const MhaSeq& sq,
                                            MhaLongLds& L, Put&& put) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float(*Pw)[MHA_SLONG] = L.P + wave * MHA_LROWS;
  for (int c0 = 0; c0 < hd; c0 += 64) {
    const int dn = min(64, hd - c0);
    float o[MHA_LROWS] = {};
    for (int j0 = 0; j0 < sq.nv; j0 += MHA_SMAX) {
      const MhaSeq blk = {sq.off + j0 * sq.stride, sq.stride, min(MHA_SMAX, sq.nv - j0)};
      __syncthreads();
      mha_long_stage(L.Y, ysrc, y_ld, col + c0, dn, blk);
      __syncthreads();
      if (lane < dn)
        for (int j = 0; j < blk.nv; j += 4) {
          float pv[MHA_LROWS][4];
#pragma unroll
          for (int i = 0; i < MHA_LROWS; ++i) {
            const float4 p4 = *reinterpret_cast<const float4*>(&Pw[i][j0 + j]);
            pv[i][0] = p4.x; pv[i][1] = p4.y; pv[i][2] = p4.z; pv[i][3] = p4.w;
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float y = L.Y[j + e][lane];
#pragma unroll
            for (int i = 0; i < MHA_LROWS; ++i) o[i] = fmaf(pv[i][e], y, o[i]);
          }
        }
    }
    if (lane < dn)
#pragma unroll
      for (int i = 0; i < MHA_LROWS; ++i) put(i, c0 + lane, o[i]);
  }
}

// The plain softmax of one row by one wave: raw scores P[0 .. nv) -> e_j = exp(score_j - max) in place; returns sum_j e_j.
__device__ __forceinline__ float mha_long_softmax(float* P, int nv, int lane) {
  float m = -INFINITY;
  for (int j = lane; j < nv; j += 64) m = fmaxf(m, P[j]);
  m = nbm_wave_max(m);
  float s = 0.f;
  for (int j = lane; j < nv; j += 64) {
    const float e = expf(P[j] - m);
    P[j] = e;
    s += e;
  }
  return nbm_wave_sum(s);
}

__device__ __forceinline__ void mha_long_pad(float* P, int nv, int lane) {
  if (nv + lane < ((nv + 3) & ~3)) P[nv + lane] = 0.f;
}

// The queries rw0 .. rw0 + MHA_LROWS - 1 of sequence sq by one wave (all four waves of the workgroup call it together), in
// the two forms of mha_row.  mask_base, mask_S: as in mha_wide_rows.
template <bool DROP>
__device__ __forceinline__ void mha_long_rows(const float* __restrict__ q, const float* __restrict__ k,
                                              const float* __restrict__ v, int q_ld, int k_ld, int v_ld, float* __restrict__ out,
                                              int out_ld, long long col, int hd, const MhaSeq& sq, int rw0, float scale,
                                              const MhaDrop& dr, uint64_t mask_base, int mask_S, MhaLongLds& L) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float(*Pw)[MHA_SLONG] = L.P + wave * MHA_LROWS;
  mha_long_dots(q, q_ld, scale, k, k_ld, col, hd, sq, rw0, L, [&](int i, int j, float a) { Pw[i][j] = a; });
  float sum[MHA_LROWS];
#pragma unroll
  for (int i = 0; i < MHA_LROWS; ++i) {
    const int r = rw0 + i;
    sum[i] = 1.f;
    if (r < sq.nv) {                                        // the rows beyond keep their scores, all zero
      const float s = mha_long_softmax(Pw[i], sq.nv, lane);
      sum[i] = s;
      if constexpr (DROP) {
        const uint64_t row_base = mask_base + (uint64_t)r * (uint64_t)mask_S;
        for (int j = lane; j < sq.nv; j += 64) Pw[i][j] = mha_keep(dr, row_base, j) ? (Pw[i][j] / s) * dr.drop_scale : 0.f;
      }
    }
    mha_long_pad(Pw[i], sq.nv, lane);
  }
  mha_long_pv(v, v_ld, col, hd, sq, L, [&](int i, int c, float o) {
    const int r = rw0 + i;
    if (r < sq.nv) out[(sq.off + r * sq.stride) * out_ld + col + c] = DROP ? o : o / sum[i];
  });
}

// nbm_mha_small / nbm_mha_small_drop, long: one workgroup per (batch entry n, head) and block of MHA_LBLOCK query rows.
template <bool DROP>
__global__ __launch_bounds__(256) void mha_long_small_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                             const float* __restrict__ v, int q_ld, int k_ld, int v_ld,
                                                             float* __restrict__ out, int out_ld, int S, int nhead, int hd,
                                                             long long seq_stride, long long batch_stride,
                                                             const int* __restrict__ n_valid, float scale, MhaDrop dr) {
  __shared__ MhaLongLds L;
  const int n = blockIdx.x / nhead, h = blockIdx.x - n * nhead;
  const int nv = n_valid ? min(*n_valid, S) : S;
  const int r0 = blockIdx.y * MHA_LBLOCK;
  if (r0 >= nv) return;
  const MhaSeq sq = {n * batch_stride, seq_stride, nv};
  mha_long_rows<DROP>(q, k, v, q_ld, k_ld, v_ld, out, out_ld, (long long)h * hd, hd, sq, r0 + (int)(threadIdx.x >> 6) * MHA_LROWS,
                      scale, dr, (uint64_t)blockIdx.x * (uint64_t)S * (uint64_t)S, S, L);
}

// nbm_mha_segments_wide in ACROSS_ROIS with more than MHA_SMAX slots: a workgroup per (image b, head) and block of query rows
// through mha_long_rows<false>, as the long nbm_mha_small's go; it also writes its share of the zero rows.
__global__ __launch_bounds__(256) void mha_long_rois_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                            const float* __restrict__ v, int q_ld, int k_ld, int v_ld,
                                                            float* __restrict__ out, int out_ld, int R, int nhead, int hd,
                                                            const int* __restrict__ n_roi, float scale) {
  __shared__ MhaLongLds L;
  const int b = blockIdx.x / nhead, h = blockIdx.x - b * nhead;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long col = (long long)h * hd;
  const int n = min(max(n_roi[b], 0), R);
  for (int r = n + wave + 4 * (int)blockIdx.y; r < R; r += 4 * (int)gridDim.y)
    for (int c = lane; c < hd; c += 64) out[((long long)b * R + r) * out_ld + col + c] = 0.f;
  const int r0 = blockIdx.y * MHA_LBLOCK;
  if (r0 >= n) return;
  const MhaSeq sq = {(long long)b * R, 1, n};
  mha_long_rows<false>(q, k, v, q_ld, k_ld, v_ld, out, out_ld, col, hd, sq, r0 + wave * MHA_LROWS, scale, MhaDrop{}, 0, 0, L);
}

// Pass 1 of the backward, long: mha_bwd_rows_kernel's quantities for a block of MHA_LBLOCK query rows.  The scores wait in P;
// dP = (dO V^T, masked and scaled under dropout) waits in the row's own slot of the workspace's dS plane, and under dropout the
// mask factor (drop_scale or 0) in that of A: a lane reads back only elements it wrote itself.
template <bool DROP>
__global__ __launch_bounds__(256) void mha_long_bwd_rows_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, const float* __restrict__ go,
    int q_ld, int k_ld, int v_ld, int go_ld, float* __restrict__ gq, int gq_ld, float* __restrict__ ws, int S, int nhead,
    int hd, long long seq_stride, long long batch_stride, const int* __restrict__ n_valid, float scale, MhaDrop dr) {
  __shared__ MhaLongLds L;
  const int n = blockIdx.x / nhead, h = blockIdx.x - n * nhead;
  const int nv = n_valid ? min(*n_valid, S) : S;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if ((int)blockIdx.y * MHA_LBLOCK >= nv) return;
  const int rw0 = blockIdx.y * MHA_LBLOCK + wave * MHA_LROWS;
  const long long col = (long long)h * hd;
  const MhaSeq sq = {n * batch_stride, seq_stride, nv};
  float(*Pw)[MHA_SLONG] = L.P + wave * MHA_LROWS;
  float* A = ws + (long long)blockIdx.x * 2 * S * S;
  float* D = A + (long long)S * S;
  mha_long_dots(q, q_ld, scale, k, k_ld, col, hd, sq, rw0, L, [&](int i, int j, float a) { Pw[i][j] = a; });
  mha_long_dots(go, go_ld, 1.f, v, v_ld, col, hd, sq, rw0, L, [&](int i, int j, float a) {
    const int r = rw0 + i;
    if (r >= nv) return;
    const long long at = (long long)r * S + j;
    if constexpr (DROP) {
      const bool keep = mha_keep(dr, ((uint64_t)blockIdx.x * (uint64_t)S + (uint64_t)r) * (uint64_t)S, j);
      D[at] = keep ? a * dr.drop_scale : 0.f;
      A[at] = keep ? dr.drop_scale : 0.f;
    } else {
      D[at] = a;
    }
  });
#pragma unroll
  for (int i = 0; i < MHA_LROWS; ++i) {
    const int r = rw0 + i;
    if (r < nv) {
      float* Ar = A + (long long)r * S;
      float* Dr = D + (long long)r * S;
      const float sum = mha_long_softmax(Pw[i], nv, lane);
      float dot = 0.f;
      for (int j = lane; j < nv; j += 64) {
        const float p = Pw[i][j] / sum;
        Pw[i][j] = p;
        dot = fmaf(p, Dr[j], dot);
      }
      dot = nbm_wave_sum(dot);
      for (int j = lane; j < nv; j += 64) {
        const float p = Pw[i][j];
        const float dsv = p * (Dr[j] - dot);
        Pw[i][j] = dsv;
        Ar[j] = DROP ? p * Ar[j] : p;
        Dr[j] = dsv;
      }
    }
    mha_long_pad(Pw[i], nv, lane);
  }
  mha_long_pv(k, k_ld, col, hd, sq, L, [&](int i, int c, float o) {
    const int r = rw0 + i;
    if (r < nv) gq[(sq.off + r * sq.stride) * gq_ld + col + c] = o * scale;
  });
}

// Pass 2, long: dK = scale dS^T Q, dV = A^T dO.  A wave owns MHA_LKEYS consecutive keys and the 64 columns of a chunk and walks
// the query rows once for all of them: the row of Q and of dO is read once per wave, the elements of dS and A are the same for
// every lane.  Grid: (entry, head) x 64-column chunk x sets of 4 * MHA_LKEYS keys.  Each sum is an fmaf chain in ascending r.
template <bool FULL>
__device__ __forceinline__ void mha_long_keys_run(const float* __restrict__ q, const float* __restrict__ go, int q_ld, int go_ld,
                                                  const float* __restrict__ A, const float* __restrict__ D, int S, int nv, int j0,
                                                  long long off, long long stride, long long c, float (&ak)[MHA_LKEYS],
                                                  float (&av)[MHA_LKEYS]) {
  for (int r = 0; r < nv; ++r) {
    const long long row = off + r * stride;
    const float qv = q[row * q_ld + c], gv = go[row * go_ld + c];
    const float* Dr = D + (long long)r * S;
    const float* Ar = A + (long long)r * S;
#pragma unroll
    for (int e = 0; e < MHA_LKEYS; ++e) {
      const int j = FULL ? j0 + e : min(j0 + e, nv - 1);
      ak[e] = fmaf(Dr[j], qv, ak[e]);
      av[e] = fmaf(Ar[j], gv, av[e]);
    }
  }
}

__global__ __launch_bounds__(256) void mha_long_bwd_keys_kernel(
    const float* __restrict__ q, const float* __restrict__ go, int q_ld, int go_ld, const float* __restrict__ ws,
    float* __restrict__ gk, float* __restrict__ gv, int gk_ld, int gv_ld, int S, int nhead, int hd, long long seq_stride,
    long long batch_stride, const int* __restrict__ n_valid, float scale) {
  const int n = blockIdx.x / nhead, h = blockIdx.x - n * nhead;
  const int nv = n_valid ? min(*n_valid, S) : S;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const float* A = ws + (long long)blockIdx.x * 2 * S * S;
  const float* D = A + (long long)S * S;
  const int cc = blockIdx.y * 64 + lane;
  const int j0 = ((int)blockIdx.z * 4 + wave) * MHA_LKEYS;
  if (cc >= hd || j0 >= nv) return;
  const long long c = (long long)h * hd + cc, off = n * batch_stride;
  float ak[MHA_LKEYS] = {}, av[MHA_LKEYS] = {};
  if (j0 + MHA_LKEYS <= nv) mha_long_keys_run<true>(q, go, q_ld, go_ld, A, D, S, nv, j0, off, seq_stride, c, ak, av);
  else mha_long_keys_run<false>(q, go, q_ld, go_ld, A, D, S, nv, j0, off, seq_stride, c, ak, av);
#pragma unroll
  for (int e = 0; e < MHA_LKEYS; ++e) {
    const int j = j0 + e;
    if (j < nv) {
      const long long rowj = off + j * seq_stride;
      gk[rowj * gk_ld + c] = ak[e] * scale;
      gv[rowj * gv_ld + c] = av[e];
    }
  }
}

// What the four nbm_mha_small* entry points ask of their geometry; pitches: every row pitch passed, each >= nhead * hd.
bool mha_small_geometry_ok(int S, int N, int nhead, int hd, std::initializer_list<int> pitches) {
  if (S <= 0 || S > MHA_SLONG || N <= 0 || nhead <= 0 || hd <= 0 || hd > MHA_HDWIDE) return false;
  for (int ld : pitches)
    if (ld < nhead * hd) return false;
  return true;
}

template <bool DROP>
int mha_small_launch(const float* q, const float* k, const float* v, int q_ld, int k_ld, int v_ld, float* out, int out_ld, int S,
                     int N, int nhead, int hd, int64_t seq_stride, int64_t batch_stride, const int32_t* n_valid, float scale,
                     const MhaDrop& dr, void* stream) {
  if (!q || !k || !v || !out || !mha_small_geometry_ok(S, N, nhead, hd, {q_ld, k_ld, v_ld, out_ld})) return NBM_EINVAL;
  if (S > MHA_SMAX)
    hipLaunchKernelGGL(mha_long_small_kernel<DROP>, dim3(N * nhead, (S + MHA_LBLOCK - 1) / MHA_LBLOCK), dim3(256), 0,
                       (hipStream_t)stream, q, k, v, q_ld, k_ld, v_ld, out, out_ld, S, nhead, hd, (long long)seq_stride,
                       (long long)batch_stride, n_valid, scale, dr);
  else if (hd <= MHA_HDMAX)
    hipLaunchKernelGGL(mha_small_kernel<DROP>, dim3(N * nhead), dim3(256), 0, (hipStream_t)stream, q, k, v, q_ld, k_ld, v_ld, out,
                       out_ld, S, nhead, hd, (long long)seq_stride, (long long)batch_stride, n_valid, scale, dr);
  else
    hipLaunchKernelGGL(mha_wide_small_kernel<DROP>, dim3(N * nhead, (S + MHA_WBLOCK - 1) / MHA_WBLOCK), dim3(256), 0,
                       (hipStream_t)stream, q, k, v, q_ld, k_ld, v_ld, out, out_ld, S, nhead, hd, (long long)seq_stride,
                       (long long)batch_stride, n_valid, scale, dr);
  return nbm_launch_status();
}

template <bool DROP>
int mha_small_bwd_launch(const float* q, const float* k, const float* v, const float* go, int q_ld, int k_ld, int v_ld,
                         int go_ld, float* gq, float* gk, float* gv, int gq_ld, int gk_ld, int gv_ld, float* workspace, int S,
                         int N, int nhead, int hd, int64_t seq_stride, int64_t batch_stride, const int32_t* n_valid, float scale,
                         const MhaDrop& dr, void* stream) {
  if (!q || !k || !v || !go || !gq || !gk || !gv || !workspace) return NBM_EINVAL;
  if (!mha_small_geometry_ok(S, N, nhead, hd, {q_ld, k_ld, v_ld, go_ld, gq_ld, gk_ld, gv_ld})) return NBM_EINVAL;
  if (S > MHA_SMAX) {
    hipLaunchKernelGGL(mha_long_bwd_rows_kernel<DROP>, dim3(N * nhead, (S + MHA_LBLOCK - 1) / MHA_LBLOCK), dim3(256), 0,
                       (hipStream_t)stream, q, k, v, go, q_ld, k_ld, v_ld, go_ld, gq, gq_ld, workspace, S, nhead, hd,
                       (long long)seq_stride, (long long)batch_stride, n_valid, scale, dr);
    hipLaunchKernelGGL(mha_long_bwd_keys_kernel, dim3(N * nhead, (hd + 63) / 64, (S + 4 * MHA_LKEYS - 1) / (4 * MHA_LKEYS)),
                       dim3(256), 0, (hipStream_t)stream, q, go, q_ld, go_ld, workspace, gk, gv, gk_ld, gv_ld, S, nhead, hd,
                       (long long)seq_stride, (long long)batch_stride, n_valid, scale);
  } else if (hd <= MHA_HDMAX) {
    hipLaunchKernelGGL(mha_bwd_rows_kernel<DROP>, dim3(N * nhead), dim3(256), 0, (hipStream_t)stream, q, k, v, go, q_ld, k_ld,
                       v_ld, go_ld, gq, gq_ld, workspace, S, nhead, hd, (long long)seq_stride, (long long)batch_stride, n_valid,
                       scale, dr);
    hipLaunchKernelGGL(mha_bwd_keys_kernel, dim3(N * nhead), dim3(256), 0, (hipStream_t)stream, q, go, q_ld, go_ld, workspace, gk,
                       gv, gk_ld, gv_ld, S, nhead, hd, (long long)seq_stride, (long long)batch_stride, n_valid, scale);
  } else {
    hipLaunchKernelGGL(mha_wide_bwd_rows_kernel<DROP>, dim3(N * nhead, (S + MHA_WBLOCK - 1) / MHA_WBLOCK), dim3(256), 0,
                       (hipStream_t)stream, q, k, v, go, q_ld, k_ld, v_ld, go_ld, gq, gq_ld, workspace, S, nhead, hd,
                       (long long)seq_stride, (long long)batch_stride, n_valid, scale, dr);
    hipLaunchKernelGGL(mha_wide_bwd_keys_kernel, dim3(N * nhead, (hd + 63) / 64, MHA_KEYBLOCKS), dim3(256), 0,
                       (hipStream_t)stream, q, go, q_ld, go_ld, workspace, gk, gv, gk_ld, gv_ld, S, nhead, hd,
                       (long long)seq_stride, (long long)batch_stride, n_valid, scale);
  }
  return nbm_launch_status();
}

// nbm_mha_segments (hd_max = MHA_HDMAX) and nbm_mha_segments_wide (hd_max = MHA_HDWIDE): one argument check, one dispatch.
int mha_segments_launch(const float* q, const float* k, const float* v, int q_ld, int k_ld, int v_ld, float* out, int out_ld,
                        int B, int R, int nhead, int hd, int hd_max, int mode, const int32_t* segments, const int32_t* n_roi,
                        int max_count, float scale, void* stream) {
  if (!q || !k || !v || !out || !n_roi || B <= 0 || R <= 0 || nhead <= 0 || hd <= 0 || hd > hd_max) return NBM_EINVAL;
  if (q_ld < nhead * hd || k_ld < nhead * hd || v_ld < nhead * hd || out_ld < nhead * hd) return NBM_EINVAL;
  if (mode == NBM_MHA_ACROSS_ROIS) {
    if (R > (hd_max == MHA_HDWIDE ? MHA_SLONG : MHA_SMAX)) return NBM_EINVAL;   // the older symbol keeps both its limits
  } else if (mode == NBM_MHA_ACROSS_IMAGES) {
    if (!segments || max_count < 1 || max_count > MHA_SMAX) return NBM_EINVAL;
  } else {
    return NBM_EINVAL;
  }
  if (mode == NBM_MHA_ACROSS_ROIS && R > MHA_SMAX)
    hipLaunchKernelGGL(mha_long_rois_kernel, dim3(B * nhead, (R + MHA_LBLOCK - 1) / MHA_LBLOCK), dim3(256), 0, (hipStream_t)stream,
                       q, k, v, q_ld, k_ld, v_ld, out, out_ld, R, nhead, hd, n_roi, scale);
  else if (hd <= MHA_HDMAX)
    hipLaunchKernelGGL(mha_segments_kernel, dim3(B * nhead), dim3(256), 0, (hipStream_t)stream, q, k, v, q_ld, k_ld, v_ld, out,
                       out_ld, B, R, nhead, hd, mode, segments, n_roi, max_count, scale);
  else
    hipLaunchKernelGGL(mha_wide_segments_kernel,
                       dim3(B * nhead, mode == NBM_MHA_ACROSS_ROIS ? (R + MHA_WBLOCK - 1) / MHA_WBLOCK : 1), dim3(256), 0,
                       (hipStream_t)stream, q, k, v, q_ld, k_ld, v_ld, out, out_ld, B, R, nhead, hd, mode, segments, n_roi,
                       max_count, scale);
  return nbm_launch_status();
}

}  // namespace

extern "C" int nbm_mha_plan(int S, int hd, int N, int nhead, nbm_mha_plan_t* out) {
  if (!out) return NBM_EINVAL;
  *out = nbm_mha_plan_t{};
  if (!mha_small_geometry_ok(S, N, nhead, hd, {})) return out->rc = NBM_EINVAL;
  if (S > MHA_SMAX) {
    out->family = NBM_MHA_LONG;
    out->lds_bytes = out->lds_bytes_bwd = (int)sizeof(MhaLongLds);
    out->rows = MHA_LBLOCK;
  } else if (hd > MHA_HDMAX) {
    out->family = NBM_MHA_WIDE;
    out->lds_bytes = out->lds_bytes_bwd = (int)sizeof(MhaWideLds);
    out->rows = MHA_WBLOCK;
  } else {
    out->family = NBM_MHA_NARROW;
    out->lds_bytes = MHA_NARROW_LDS;
    out->lds_bytes_bwd = MHA_NARROW_BWD_LDS;
    out->rows = S;
  }
  out->row_blocks = (S + out->rows - 1) / out->rows;
  out->workspace_bytes = (int64_t)sizeof(float) * 2 * N * nhead * S * S;
  return NBM_OK;
}

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
  return mha_segments_launch(q, k, v, q_ld, k_ld, v_ld, out, out_ld, B, R, nhead, hd, MHA_HDMAX, mode, segments, n_roi, max_count,
                             scale, stream);
}

extern "C" int nbm_mha_segments_wide(const float* q, const float* k, const float* v, int q_ld, int k_ld, int v_ld, float* out,
                                     int out_ld, int B, int R, int nhead, int hd, int mode, const int32_t* segments,
                                     const int32_t* n_roi, int max_count, float scale, void* stream) {
  return mha_segments_launch(q, k, v, q_ld, k_ld, v_ld, out, out_ld, B, R, nhead, hd, MHA_HDWIDE, mode, segments, n_roi, max_count,
                             scale, stream);
}
