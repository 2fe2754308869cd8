// Proposal / RoI / detection stages of the NBM detector on device: box decoding, top-N selection,
// greedy NMS, RoI pooling (+ separable positional encoding) and the FastRCNN eval post-processing.
// Integer / sort / index work: results are bit-exact against the oracle for identical inputs, so
// floating-point contraction is disabled wherever a value is rounded to a pixel coordinate or compared
// with a threshold (torch CPU evaluates a*b+c as two rounded operations).
#include "nbm_common.h"

#pragma clang fp contract(off)

namespace {

// bbox_reg_to_coord (reference nets_utils.py:169-186) + clip (layers.py:279-280)
__device__ __forceinline__ void decode_clip(const float* d, const float* a, int img_w, int img_h, float* o) {
  const float wa = (a[2] - a[0]) + 1.0f, ha = (a[3] - a[1]) + 1.0f;
  const float xa = a[0] + 0.5f * wa, ya = a[1] + 0.5f * ha;
  const float x = (d[0] * wa) + xa, y = (d[1] * ha) + ya;
  const float w = expf(d[2]) * wa, h = expf(d[3]) * ha;
  const float xm = (float)(img_w - 1), ym = (float)(img_h - 1);
  o[0] = fminf(fmaxf(rintf(x - 0.5f * w), 0.f), xm);
  o[1] = fminf(fmaxf(rintf(y - 0.5f * h), 0.f), ym);
  o[2] = fminf(fmaxf(rintf(x + 0.5f * w), 0.f), xm);
  o[3] = fminf(fmaxf(rintf(y + 0.5f * h), 0.f), ym);
}

// IoU with the inclusive-pixel convention (reference nets_utils.py:189-207)
__device__ __forceinline__ float iou_incl(const float* a, const float* b) {
  const float xi = fmaxf((fminf(a[2], b[2]) - fmaxf(a[0], b[0])) + 1.0f, 0.f);
  const float yi = fmaxf((fminf(a[3], b[3]) - fmaxf(a[1], b[1])) + 1.0f, 0.f);
  const float inter = xi * yi;
  const float aa = ((a[2] - a[0]) + 1.0f) * ((a[3] - a[1]) + 1.0f);
  const float ab = ((b[2] - b[0]) + 1.0f) * ((b[3] - b[1]) + 1.0f);
  return inter / ((aa + ab) - inter);
}

// ------------------------------------------------------------------ RPN decode
__global__ void rpn_decode_kernel(const float* __restrict__ cls, const float* __restrict__ reg,
                                  const float* __restrict__ anchors, int KA, int n_anchor, int img_w, int img_h,
                                  float min_size, float* __restrict__ boxes, uint32_t* __restrict__ keys,
                                  int* __restrict__ keep_count) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  int kept = 0;
  if (i < KA) {
    const int k = i / n_anchor, a = i - k * n_anchor;
    const long long pix = (long long)b * (KA / n_anchor) + k;
    const float score = cls[pix * (2 * n_anchor) + 2 * a + 1];
    float d[4], an[4], o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) { d[e] = reg[pix * (4 * n_anchor) + 4 * a + e]; an[e] = anchors[i * 4 + e]; }
    decode_clip(d, an, img_w, img_h, o);
    const bool keep = ((o[2] - o[0]) + 1.0f >= min_size) && ((o[3] - o[1]) + 1.0f >= min_size);
    float* ob = boxes + ((long long)b * KA + i) * 4;
    ob[0] = o[0]; ob[1] = o[1]; ob[2] = o[2]; ob[3] = o[3];
    keys[(long long)b * KA + i] = keep ? nbm_f2key(score) : 0u;
    kept = keep ? 1 : 0;
  }
  const unsigned long long m = __ballot(kept);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(keep_count + b, __popcll(m));
}

// An input image that holds a NaN keeps no anchor.  In the reference a NaN pixel spreads through every layer (relu(NaN) and
// max-pooling keep it; in the default configuration the attention levels and the top-down path carry it to every position:
// checked with one NaN pixel on the CPU oracle, tests/test_gpu_detect_edges.py), so every comparison of the
// size filter is false and the image's kept count is 0 ("RPN failed").  The epilogues here clamp with v_max, which drops a
// NaN, so the decision is taken from the image itself: launched after rpn_decode_kernel on the same stream.
__global__ void nan_images_kernel(const float* __restrict__ img, long long n, int* __restrict__ keep_count) {
  const int b = blockIdx.y;
  const float* p = img + (long long)b * n;
  bool bad = false;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float v = p[i];
    bad = bad || (v != v);
  }
  if (bad) keep_count[b] = 0;                    // benign race: every writer stores 0
}

// Segment of image b in a table of contiguous segments: seg[b] = first image, seg[B + b] = image count.  Clamped into
// [0, B) with b inside it, so that a malformed table can never make a kernel read past the batch.
__device__ __forceinline__ void seg_range(const int* __restrict__ seg, int B, int b, int& lo, int& hi) {
  lo = min(max(seg[b], 0), b);
  hi = max(min(lo + seg[B + b], B), b + 1);
}

// ------------------------------------------------------------------ top-N selection (radix select + bitonic sort)
// composite key = (score_key << 32) | ~index : unique, descending order == (score desc, index asc)
constexpr int SEL_THREADS = 1024;

// The N-th largest composite key of an image, N = *s_need on entry (1 <= N <= KA), left in *s_prefix: 8 passes of 8 bits, MSB
// first, each a histogram of the next byte over the keys that match the prefix found so far.  Whole workgroup; *s_prefix = 0
// on entry, hist = 256 LDS counters.
__device__ __forceinline__ void select_threshold(const uint32_t* __restrict__ kb, int KA, unsigned int* hist,
                                                 unsigned long long* s_prefix, int* s_need) {
  const int tid = threadIdx.x;
  for (int pass = 7; pass >= 0; --pass) {
    for (int i = tid; i < 256; i += SEL_THREADS) hist[i] = 0u;
    __syncthreads();
    const int shift = pass * 8;
    const unsigned long long prefix = *s_prefix;
    const unsigned long long himask = pass == 7 ? 0ull : (~0ull << (shift + 8));
    for (int i = tid; i < KA; i += SEL_THREADS) {
      const unsigned long long c = ((unsigned long long)kb[i] << 32) | (unsigned int)(~(unsigned int)i);
      if ((c & himask) == prefix) atomicAdd(&hist[(c >> shift) & 255ull], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      int need = *s_need, d = 255;
      for (; d > 0; --d) { if ((int)hist[d] >= need) break; need -= (int)hist[d]; }
      *s_need = need;
      *s_prefix = prefix | ((unsigned long long)d << shift);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(SEL_THREADS) void rpn_select_kernel(
    const float* __restrict__ boxes, const uint32_t* __restrict__ keys, const int* __restrict__ keep_count, int B,
    int KA, int top_n, int fail_below, int cap, float* __restrict__ sel_boxes, float* __restrict__ sel_scores,
    int* __restrict__ n_sel, const int* __restrict__ seg) {
  extern __shared__ unsigned long long sm[];  // [cap] sort buffer, then 256 histogram counters + scalars
  unsigned long long* buf = sm;
  unsigned int* hist = reinterpret_cast<unsigned int*>(sm + cap);
  __shared__ unsigned long long s_prefix;
  __shared__ int s_need, s_count, s_N;
  const int b = blockIdx.x, tid = threadIdx.x;
  const uint32_t* kb = keys + (long long)b * KA;

  if (tid == 0) {
    // layers.py:287: pre_nms_topN = min(topN, min over the BATCH of the kept-anchor counts); the images of b's segment
    // form one model call of their own
    int lo, hi, mn = 0x7fffffff;
    seg_range(seg, B, b, lo, hi);
    for (int i = lo; i < hi; ++i) mn = min(mn, keep_count[i]);
    int N = min(top_n, mn);
    if (N < fail_below) N = 0;
    s_N = N; s_need = N; s_prefix = 0ull; s_count = 0;
    n_sel[b] = N;
  }
  __syncthreads();
  const int N = s_N;
  for (int i = tid; i < cap; i += SEL_THREADS) buf[i] = 0ull;
  if (N > 0) {
    select_threshold(kb, KA, hist, &s_prefix, &s_need);
    const unsigned long long thr = s_prefix;  // exactly N composites are >= thr
    for (int i = tid; i < KA; i += SEL_THREADS) {
      const unsigned long long c = ((unsigned long long)kb[i] << 32) | (unsigned int)(~(unsigned int)i);
      if (c >= thr) { const int pos = atomicAdd(&s_count, 1); if (pos < cap) buf[pos] = c; }
    }
  }
  __syncthreads();
  // bitonic sort, descending
  for (int k = 2; k <= cap; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < cap; i += SEL_THREADS) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const unsigned long long x = buf[i], y = buf[ixj];
          const bool desc = (i & k) == 0;
          if (desc ? (x < y) : (x > y)) { buf[i] = y; buf[ixj] = x; }
        }
      }
      __syncthreads();
    }
  }
  for (int r = tid; r < cap; r += SEL_THREADS) {
    float* ob = sel_boxes + ((long long)b * cap + r) * 4;
    if (r < N) {
      const unsigned long long c = buf[r];
      const int idx = (int)(~(unsigned int)(c & 0xffffffffull));
      const float* ib = boxes + ((long long)b * KA + idx) * 4;
      ob[0] = ib[0]; ob[1] = ib[1]; ob[2] = ib[2]; ob[3] = ib[3];
      sel_scores[(long long)b * cap + r] = nbm_key2f((uint32_t)(c >> 32));
    } else {
      ob[0] = ob[1] = ob[2] = ob[3] = 0.f;
      sel_scores[(long long)b * cap + r] = 0.f;
    }
  }
}

// ------------------------------------------------------------------ NMS
__global__ void nms_mask_kernel(const float* __restrict__ boxes, const int* __restrict__ n_in, int cap, int words,
                                float thresh, unsigned long long* __restrict__ mask) {
  const int b = blockIdx.z, rb = blockIdx.y, cb = blockIdx.x;
  const int n = n_in[b];
  if (rb * 64 >= n || cb * 64 >= n || cb < rb) return;
  __shared__ float cbox[64][4];
  const int t = threadIdx.x;
  const float* bb = boxes + (long long)b * cap * 4;
  {
    const int j = cb * 64 + t;
#pragma unroll
    for (int e = 0; e < 4; ++e) cbox[t][e] = j < n ? bb[j * 4 + e] : 0.f;
  }
  __syncthreads();
  const int i = rb * 64 + t;
  if (i >= n) return;
  float me[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) me[e] = bb[i * 4 + e];
  unsigned long long bits = 0ull;
  const int jn = min(64, n - cb * 64);
  for (int jj = 0; jj < jn; ++jj) {
    const int j = cb * 64 + jj;
    if (j > i && iou_incl(me, cbox[jj]) >= thresh) bits |= 1ull << jj;
  }
  mask[((long long)b * cap + i) * words + cb] = bits;
}

// one wave per image: lane w owns removed-word w (cap <= 4096)
__global__ __launch_bounds__(64) void nms_scan_kernel(const unsigned long long* __restrict__ mask,
                                                      const int* __restrict__ n_in, int cap, int words,
                                                      int* __restrict__ keep_idx, int* __restrict__ keep_cnt) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n = n_in[b];
  const int nwords = (n + 63) >> 6;
  unsigned long long removed = 0ull;
  int cnt = 0;
  const unsigned long long* mb = mask + (long long)b * cap * words;
  for (int i = 0; i < n; ++i) {
    const int wi = i >> 6;
    const unsigned long long rw = __shfl(removed, wi);
    if (!((rw >> (i & 63)) & 1ull)) {
      if (lane == 0) keep_idx[(long long)b * cap + cnt] = i;
      ++cnt;
      // row i only has valid words for column blocks >= i/64 (upper triangle)
      if (lane < nwords && lane >= wi) removed |= mb[(long long)i * words + lane];
    }
  }
  if (lane == 0) keep_cnt[b] = cnt;
}

__global__ void nms_gather_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                  const int* __restrict__ keep_idx, const int* __restrict__ keep_cnt, int B, int cap,
                                  int post_n, float* __restrict__ rois, float* __restrict__ roi_scores,
                                  int* __restrict__ n_out, const int* __restrict__ seg) {
  const int b = blockIdx.x;
  // nets_utils.py:236: post_nms_topN = min(topN, min over the BATCH of the survivor counts), the batch being b's segment
  int lo, hi, mn = 0x7fffffff;
  seg_range(seg, B, b, lo, hi);
  for (int i = lo; i < hi; ++i) mn = min(mn, keep_cnt[i]);
  const int R = min(post_n, mn);
  if (threadIdx.x == 0) n_out[b] = R;
  for (int r = threadIdx.x; r < post_n; r += blockDim.x) {
    float* o = rois + ((long long)b * post_n + r) * 4;
    if (r < R) {
      const int idx = keep_idx[(long long)b * cap + r];
      const float* ib = boxes + ((long long)b * cap + idx) * 4;
      o[0] = ib[0]; o[1] = ib[1]; o[2] = ib[2]; o[3] = ib[3];
      roi_scores[(long long)b * post_n + r] = scores[(long long)b * cap + idx];
    } else {
      o[0] = o[1] = o[2] = o[3] = 0.f;
      roi_scores[(long long)b * post_n + r] = 0.f;
    }
  }
}

// ------------------------------------------------------------------ proposals beyond 4 096 boxes per image
// nbm_rpn_select_big / nbm_nms_big: the same contracts as nbm_rpn_select / nbm_nms_batched for cap up to BIG_CAP_MAX, with
// workspaces linear in B * cap (DESIGN "Proposals beyond 4 096").
constexpr int BIG_CAP_MAX = 65536;
constexpr int SORT_RUN = 4096;               // composite keys of one LDS-sorted run: 32 KiB

// One step (k, j) of the descending bitonic network on the run[0, len) that starts at element `base` of the whole sequence:
// a thread takes pairs (i, i + j), never an idle half.  Ends with a barrier.
__device__ __forceinline__ void bitonic_step(unsigned long long* run, int len, int base, int k, int j) {
  for (int t = threadIdx.x; t < (len >> 1); t += SEL_THREADS) {
    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
    const unsigned long long x = run[i], y = run[i + j];
    const bool desc = ((base + i) & k) == 0;
    if (desc ? (x < y) : (x > y)) { run[i] = y; run[i + j] = x; }
  }
  __syncthreads();
}

// One workgroup per image.  The radix search is rpn_select_kernel's; the N composites at or above the threshold go to the
// image's slice of sort_ws, padded with zeros to P = the power of two at or above N, and are sorted there: runs of
// min(P, SORT_RUN) keys in LDS, then for every longer stage k the steps j >= SORT_RUN in global memory and the steps below
// it run by run in LDS again.  sort_ws is written and read by this workgroup alone, between barriers.
__global__ __launch_bounds__(SEL_THREADS) void rpn_select_big_kernel(
    const float* __restrict__ boxes, const uint32_t* __restrict__ keys, const int* __restrict__ keep_count, int B,
    int KA, int top_n, int fail_below, int cap, unsigned long long* sort_ws, float* __restrict__ sel_boxes,
    float* __restrict__ sel_scores, int* __restrict__ n_sel, const int* __restrict__ seg) {
  __shared__ unsigned long long run[SORT_RUN];
  __shared__ unsigned int hist[256];
  __shared__ unsigned long long s_prefix;
  __shared__ int s_need, s_count, s_N;
  const int b = blockIdx.x, tid = threadIdx.x;
  const uint32_t* kb = keys + (long long)b * KA;
  unsigned long long* g = sort_ws + (long long)b * cap;

  if (tid == 0) {
    int lo, hi, mn = 0x7fffffff;
    seg_range(seg, B, b, lo, hi);
    for (int i = lo; i < hi; ++i) mn = min(mn, keep_count[i]);
    int N = min(min(top_n, mn), KA);               // a count above KA cannot be met: the search needs N existing keys
    if (N < fail_below || N < 0) N = 0;
    s_N = N; s_need = N; s_prefix = 0ull; s_count = 0;
    n_sel[b] = N;
  }
  __syncthreads();
  const int N = s_N;
  if (N > 0) {
    int P = 64;
    while (P < N) P <<= 1;                         // N <= top_n <= cap, a power of two: P <= cap
    const int len = min(P, SORT_RUN);
    select_threshold(kb, KA, hist, &s_prefix, &s_need);
    const unsigned long long thr = s_prefix;       // exactly N composites are >= thr
    for (int i = tid; i < KA; i += SEL_THREADS) {
      const unsigned long long c = ((unsigned long long)kb[i] << 32) | (unsigned int)(~(unsigned int)i);
      if (c >= thr) { const int pos = atomicAdd(&s_count, 1); if (pos < P) g[pos] = c; }
    }
    for (int i = N + tid; i < P; i += SEL_THREADS) g[i] = 0ull;
    __syncthreads();
    for (int base = 0; base < P; base += len) {
      for (int i = tid; i < len; i += SEL_THREADS) run[i] = g[base + i];
      __syncthreads();
      for (int k = 2; k <= len; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) bitonic_step(run, len, base, k, j);
      for (int i = tid; i < len; i += SEL_THREADS) g[base + i] = run[i];
      __syncthreads();
    }
    for (int k = len << 1; k <= P; k <<= 1) {
      for (int j = k >> 1; j >= len; j >>= 1) {
        for (int t = tid; t < (P >> 1); t += SEL_THREADS) {
          const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
          const unsigned long long x = g[i], y = g[i + j];
          const bool desc = (i & k) == 0;
          if (desc ? (x < y) : (x > y)) { g[i] = y; g[i + j] = x; }
        }
        __syncthreads();
      }
      for (int base = 0; base < P; base += len) {
        for (int i = tid; i < len; i += SEL_THREADS) run[i] = g[base + i];
        __syncthreads();
        for (int j = len >> 1; j > 0; j >>= 1) bitonic_step(run, len, base, k, j);
        for (int i = tid; i < len; i += SEL_THREADS) g[base + i] = run[i];
        __syncthreads();
      }
    }
  }
  for (int r = tid; r < cap; r += SEL_THREADS) {
    float* ob = sel_boxes + ((long long)b * cap + r) * 4;
    if (r < N) {
      const unsigned long long c = g[r];
      const int idx = (int)(~(unsigned int)(c & 0xffffffffull));
      const float* ib = boxes + ((long long)b * KA + idx) * 4;
      ob[0] = ib[0]; ob[1] = ib[1]; ob[2] = ib[2]; ob[3] = ib[3];
      sel_scores[(long long)b * cap + r] = nbm_key2f((uint32_t)(c >> 32));
    } else {
      ob[0] = ob[1] = ob[2] = ob[3] = 0.f;
      sel_scores[(long long)b * cap + r] = 0.f;
    }
  }
}

constexpr int NMSB_THREADS = 1024, NMSB_WAVES = NMSB_THREADS / 64;
constexpr int NMSB_KEPT_LDS = 2048;          // kept boxes held in LDS (32 KiB); later ones are read back from `rois`

__device__ __forceinline__ unsigned long long readlane64(unsigned long long v, int k) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, k);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), k);
  return ((unsigned long long)hi << 32) | lo;
}

// The greedy walk of one image in one workgroup, 64 boxes per step, without a mask: lane l of every wave holds box
// blk * 64 + l; wave w tests it against the kept boxes w, w + 16, ... found so far and against columns 4 w .. 4 w + 3 of
// the block's own 64 x 64 tile; wave 0 then ORs the 16 verdicts and resolves the tile in registers (64 dependent bit steps on
// the scalar unit, as merge.hip's scan).  A kept box goes straight to its output row, and to LDS while it fits: the walk
// stops at post_n kept boxes (a survivor count enters the result only through min(post_n, .)), so every kept box that a
// later step needs is an output row of this image.  `rois` is read back by the workgroup that wrote it, after a barrier.
__global__ __launch_bounds__(NMSB_THREADS) void nms_big_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                               const int* __restrict__ n_in, int cap, float thresh, int post_n,
                                                               float* rois, float* __restrict__ roi_scores,
                                                               int* __restrict__ keep_cnt) {
  __shared__ float kept[NMSB_KEPT_LDS][4];
  __shared__ unsigned long long sup_sh[NMSB_WAVES];
  __shared__ unsigned int diag_sh[NMSB_WAVES][64];
  __shared__ unsigned long long kp_sh;
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = min(max(n_in[b], 0), cap);
  const float* bb = boxes + (long long)b * cap * 4;
  float* out = rois + (long long)b * post_n * 4;
  const unsigned long long lt = (1ull << lane) - 1ull;
  int cnt = 0;
  for (int blk = 0; blk * 64 < n && cnt < post_n; ++blk) {
    const int i = blk * 64 + lane;
    float me[4] = {0.f, 0.f, 0.f, 0.f};
    if (i < n) {
#pragma unroll
      for (int e = 0; e < 4; ++e) me[e] = bb[(long long)i * 4 + e];
    }
    bool sup = false;
    const int c_lds = min(cnt, NMSB_KEPT_LDS);
    for (int k = wave; k < c_lds; k += NMSB_WAVES) sup |= iou_incl(kept[k], me) >= thresh;
    for (int k = NMSB_KEPT_LDS + wave; k < cnt; k += NMSB_WAVES) sup |= iou_incl(out + (long long)k * 4, me) >= thresh;
    const unsigned long long sm = __ballot(sup);
    if (lane == 0) sup_sh[wave] = sm;
    unsigned int d = 0u;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int jj = wave * 4 + q, j = blk * 64 + jj;
      if (jj > lane && j < n && iou_incl(me, bb + (long long)j * 4) >= thresh) d |= 1u << q;
    }
    diag_sh[wave][lane] = d;
    __syncthreads();
    if (wave == 0) {
      unsigned long long rem = 0ull, diag = 0ull;
#pragma unroll
      for (int w = 0; w < NMSB_WAVES; ++w) {
        rem |= sup_sh[w];
        diag |= (unsigned long long)diag_sh[w][lane] << (4 * w);
      }
      rem = readlane64(rem, 0);
      const int m = min(64, n - blk * 64);
      if (m < 64) rem |= ~0ull << m;
#pragma unroll
      for (int k = 0; k < 64; ++k) {
        const unsigned long long dk = readlane64(diag, k);
        rem |= ((rem >> k) & 1ull) ? 0ull : dk;
      }
      const unsigned long long kp = ~rem;
      if ((kp >> lane) & 1ull) {
        const int p = cnt + __popcll(kp & lt);
        if (p < post_n) {
#pragma unroll
          for (int e = 0; e < 4; ++e) out[(long long)p * 4 + e] = me[e];
          roi_scores[(long long)b * post_n + p] = scores[(long long)b * cap + i];
          if (p < NMSB_KEPT_LDS) {
#pragma unroll
            for (int e = 0; e < 4; ++e) kept[p][e] = me[e];
          }
        }
      }
      if (lane == 0) kp_sh = kp;
    }
    __syncthreads();
    cnt += __popcll(kp_sh);
  }
  if (threadIdx.x == 0) keep_cnt[b] = cnt;
}

// The coupled truncation: R_b = min(post_n, min over b's segment of the survivor counts); rows R_b .. post_n - 1 are zeroed
// (rows below R_b were written by the walk, which kept at least R_b boxes).
__global__ void nms_big_finish_kernel(const int* __restrict__ keep_cnt, int B, int post_n, float* __restrict__ rois,
                                      float* __restrict__ roi_scores, int* __restrict__ n_out, const int* __restrict__ seg) {
  const int b = blockIdx.x;
  int lo, hi, mn = 0x7fffffff;
  seg_range(seg, B, b, lo, hi);
  for (int i = lo; i < hi; ++i) mn = min(mn, keep_cnt[i]);
  const int R = max(min(post_n, mn), 0);
  if (threadIdx.x == 0) n_out[b] = R;
  for (int r = R + threadIdx.x; r < post_n; r += blockDim.x) {
    float* o = rois + ((long long)b * post_n + r) * 4;
    o[0] = o[1] = o[2] = o[3] = 0.f;
    roi_scores[(long long)b * post_n + r] = 0.f;
  }
}

size_t nms_big_ws_bytes(int B) { return 256 + ((size_t)B * sizeof(int) + 255) / 256 * 256; }

// ------------------------------------------------------------------ FastRCNN eval post-processing
constexpr int POST_MAX = 1024;

__global__ __launch_bounds__(256) void rcnn_post_kernel(const float* __restrict__ rois, const int* __restrict__ n_roi,
                                                        int roi_cap, const float* __restrict__ bbox_reg,
                                                        const float* __restrict__ bbox_cls, int n_cls1, int img_w,
                                                        int img_h, float nms_thresh, float min_score,
                                                        int proposal_number, float* __restrict__ det,
                                                        int* __restrict__ n_det) {
  __shared__ unsigned long long skey[POST_MAX];
  __shared__ float sbox[POST_MAX][4];
  __shared__ float sscore[POST_MAX];
  __shared__ int scls[POST_MAX];
  __shared__ unsigned char alive[POST_MAX];
  __shared__ int s_cnt;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int R = min(n_roi[b], roi_cap);
  int P = 1;
  while (P < R) P <<= 1;
  // 1. class arg-max (first maximum), score
  for (int r = tid; r < P; r += blockDim.x) {
    unsigned long long key = 0ull;
    if (r < R) {
      const float* pc = bbox_cls + ((long long)b * roi_cap + r) * n_cls1;
      float best = pc[0]; int bi = 0;
      for (int c = 1; c < n_cls1; ++c) { const float v = pc[c]; if (v > best) { best = v; bi = c; } }
      key = ((unsigned long long)nbm_f2key(best) << 32) | (unsigned int)(~(unsigned int)r);
      scls[r] = bi;  // temporarily indexed by roi
    }
    skey[r] = key;
  }
  __syncthreads();
  // 2. sort by (score desc, roi index asc)
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += blockDim.x) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const unsigned long long x = skey[i], y = skey[ixj];
          const bool desc = (i & k) == 0;
          if (desc ? (x < y) : (x > y)) { skey[i] = y; skey[ixj] = x; }
        }
      }
      __syncthreads();
    }
  // 3. decode the arg-max class deltas against the RoI, clip (sorted position s <- roi r)
  __shared__ int ocls[POST_MAX];
  for (int s = tid; s < R; s += blockDim.x) {
    const unsigned long long key = skey[s];
    const int r = (int)(~(unsigned int)(key & 0xffffffffull));
    const int c = scls[r];
    const float* pd = bbox_reg + ((long long)b * roi_cap + r) * (4 * n_cls1) + 4 * c;
    const float* pr = rois + ((long long)b * roi_cap + r) * 4;
    float d[4] = {pd[0], pd[1], pd[2], pd[3]}, a[4] = {pr[0], pr[1], pr[2], pr[3]};
    decode_clip(d, a, img_w, img_h, sbox[s]);
    sscore[s] = nbm_key2f((uint32_t)(key >> 32));
    ocls[s] = c;
    alive[s] = c > 0 ? 1 : 0;                      // background dropped before the first NMS (layers.py:734)
  }
  __syncthreads();
  // 4. class-agnostic greedy NMS in score order (layers.py:742)
  for (int i = 0; i < R; ++i) {
    if (alive[i]) {
      for (int j = i + 1 + tid; j < R; j += blockDim.x)
        if (alive[j] && iou_incl(sbox[i], sbox[j]) >= nms_thresh) alive[j] = 0;
    }
    __syncthreads();
  }
  // 5. per-class greedy NMS (layers.py:761).  After step 4 no surviving pair overlaps >= thresh, so this
  //    only reproduces the per-class truncation to `proposal_number`; kept for faithfulness.
  for (int i = 0; i < R; ++i) {
    if (alive[i]) {
      for (int j = i + 1 + tid; j < R; j += blockDim.x)
        if (alive[j] && ocls[j] == ocls[i] && iou_incl(sbox[i], sbox[j]) >= nms_thresh) alive[j] = 0;
    }
    __syncthreads();
  }
  // 6. rank inside class (truncate to proposal_number), min_score filter, emit sorted by (class, score desc)
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  __shared__ unsigned char emit[POST_MAX];
  for (int s = tid; s < R; s += blockDim.x) {
    int rank_in_class = 0;
    if (alive[s])
      for (int j = 0; j < s; ++j) rank_in_class += (alive[j] && ocls[j] == ocls[s]) ? 1 : 0;
    emit[s] = (alive[s] && rank_in_class < proposal_number && sscore[s] > min_score) ? 1 : 0;
  }
  __syncthreads();
  for (int s = tid; s < R; s += blockDim.x) {
    if (!emit[s]) continue;
    int pos = 0;
    for (int j = 0; j < R; ++j)
      if (emit[j] && (ocls[j] < ocls[s] || (ocls[j] == ocls[s] && j < s))) ++pos;
    float* o = det + ((long long)b * roi_cap + pos) * 6;
    o[0] = (float)ocls[s]; o[1] = sbox[s][0]; o[2] = sbox[s][1]; o[3] = sbox[s][2]; o[4] = sbox[s][3];
    o[5] = sscore[s];
    atomicAdd(&s_cnt, 1);
  }
  __syncthreads();
  if (tid == 0) n_det[b] = s_cnt;
}


// Proposal targets, the arithmetic half (layers.py:320-330 -> nets_utils.py:103-126): IoU with the inclusive-pixel (+1) convention
// of every proposal and every ground-truth box of an image against the image's ground-truth boxes, best overlap and FIRST best
// box per row.  One thread per row; the fp32 operations and their order are those of the reference's torch-CPU expressions (this
// file is compiled without contraction, the division is correctly rounded), so the thresholds the host applies afterwards
// resolve exactly as they do there.
__global__ void proposal_iou_kernel(const float* __restrict__ rois, const float* __restrict__ gt, const int* __restrict__ n_gt,
                                    int B, int R, int G, float* __restrict__ mx, int* __restrict__ asg) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (j >= R + G) return;
  const float* a = j < R ? rois + ((size_t)b * R + j) * 4 : gt + ((size_t)b * G + (j - R)) * 4;
  const float a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3];
  const float area_a = (a2 - a0 + 1.f) * (a3 - a1 + 1.f);
  const int ng = n_gt[b];
  float best = 0.f;
  int arg = 0;
  for (int g = 0; g < G; ++g) {
    float ov = -1.f;                                     // padded column: can never win
    if (g < ng) {
      const float* q = gt + ((size_t)b * G + g) * 4;
      const float g0 = q[0], g1 = q[1], g2 = q[2], g3 = q[3];
      float xi = fminf(a2, g2) - fmaxf(a0, g0) + 1.f;
      xi = fmaxf(xi, 0.f);
      float yi = fminf(a3, g3) - fmaxf(a1, g1) + 1.f;
      yi = fmaxf(yi, 0.f);
      const float inter = xi * yi;
      const float area_g = (g2 - g0 + 1.f) * (g3 - g1 + 1.f);
      const float den = (area_a + area_g) - inter;
      ov = __fdiv_rn(inter, den);
    }
    // numpy max / argmax: a NaN wins and stays, otherwise the first strictly greater value
    if (g == 0 || (!(best != best) && (ov > best || ov != ov))) { best = ov; arg = g; }
  }
  mx[(size_t)b * (R + G) + j] = best;
  asg[(size_t)b * (R + G) + j] = arg;
}

// AnchorTargetLayer, arithmetic half (reference layers.py:150-179, nets_utils.py:103-126): IoU of the image's ground-truth boxes with
// every anchor that lies inside the image, best overlap / first best box per anchor, best overlap per box, and the label each anchor
// has BEFORE the random subsampling: 0 if best < neg_t, 1 if best >= pos_t or the anchor is a best anchor (ties included) of a box
// whose best overlap is > 0, else -1.  One workgroup per image; the IoU uses the reference's fp32 operations in its order (no
// contraction in this file, correctly rounded division), evaluated twice with the same code, so `ov == gmx` means what it means on
// the host.  A NaN or negative overlap (degenerate box) raises the image's flag: the host then recomputes that image with NumPy.
constexpr int ANCHOR_MAXG = 256;
__device__ __forceinline__ float anchor_ov(const float* a, const float* q) {
  const float area_a = (a[2] - a[0] + 1.f) * (a[3] - a[1] + 1.f);
  float xi = fminf(a[2], q[2]) - fmaxf(a[0], q[0]) + 1.f;
  xi = fmaxf(xi, 0.f);
  float yi = fminf(a[3], q[3]) - fmaxf(a[1], q[1]) + 1.f;
  yi = fmaxf(yi, 0.f);
  const float inter = xi * yi;
  const float area_g = (q[2] - q[0] + 1.f) * (q[3] - q[1] + 1.f);
  const float den = (area_a + area_g) - inter;
  return __fdiv_rn(inter, den);
}

__global__ __launch_bounds__(1024) void anchor_targets_kernel(const float* __restrict__ anchors, int n_in, const float* __restrict__ gt,
                                                              const int* __restrict__ n_gt, int G, float neg_t, float pos_t,
                                                              signed char* __restrict__ lab, short* __restrict__ amx,
                                                              int* __restrict__ flag) {
  __shared__ float sg[ANCHOR_MAXG * 4];
  __shared__ int gmx[ANCHOR_MAXG];          // float bits of the best overlap of every box (overlaps are >= +0: integer order == float order)
  __shared__ int bad;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int ng = min(n_gt[b], G);
  for (int i = tid; i < ng * 4; i += 1024) sg[i] = gt[(size_t)b * G * 4 + i];
  for (int i = tid; i < ng; i += 1024) gmx[i] = 0;
  if (tid == 0) bad = 0;
  __syncthreads();
  for (int a = tid; a < n_in; a += 1024) {
    float an[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) an[e] = anchors[(size_t)a * 4 + e];
    for (int g = 0; g < ng; ++g) {
      const float ov = anchor_ov(an, sg + 4 * g);
      if (!(ov >= 0.f)) bad = 1;             // NaN or negative: benign race, every writer stores 1
      else if (ov > 0.f) atomicMax(&gmx[g], __float_as_int(ov));
    }
  }
  __syncthreads();
  for (int a = tid; a < n_in; a += 1024) {
    float an[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) an[e] = anchors[(size_t)a * 4 + e];
    float best = 0.f;
    int arg = 0;
    bool top = false;
    for (int g = 0; g < ng; ++g) {
      const float ov = anchor_ov(an, sg + 4 * g);
      if (g == 0 || ov > best) { best = ov; arg = g; }       // numpy max / argmax: the first strictly greater value
      const float gm = __int_as_float(gmx[g]);
      top = top || (gm > 0.f && ov == gm);
    }
    signed char l = -1;
    if (best < neg_t) l = 0;
    if (best >= pos_t) l = 1;
    if (top) l = 1;
    lab[(size_t)b * n_in + a] = l;
    amx[(size_t)b * n_in + a] = (short)arg;
  }
  if (tid == 0) flag[b] = bad;
}

}  // namespace

extern "C" int nbm_rpn_decode(const float* cls, const float* reg, const float* anchors, int B, int KA,
                                int n_anchor, int img_w, int img_h, int min_size, float* boxes, uint32_t* keys,
                                int* keep_count, void* stream) {
  if (!cls || !reg || !anchors || !boxes || !keys || !keep_count || B <= 0 || KA <= 0 || n_anchor <= 0 ||
      KA % n_anchor)
    return NBM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = nbm_zero_async(keep_count, sizeof(int) * B, st);
  if (e != hipSuccess) return (int)e;
  dim3 grid((KA + 255) / 256, B);
  hipLaunchKernelGGL(rpn_decode_kernel, grid, dim3(256), 0, st, cls, reg, anchors, KA, n_anchor, img_w, img_h,
                     (float)min_size, boxes, keys, keep_count);
  return nbm_launch_status();
}

extern "C" int nbm_nan_images(const float* img, int B, int64_t n, int* keep_count, void* stream) {
  if (!img || !keep_count || B <= 0 || B > 65535 || n <= 0) return NBM_EINVAL;
  const long long blocks = (n + 1023) / 1024;
  hipLaunchKernelGGL(nan_images_kernel, dim3((unsigned)(blocks < 128 ? blocks : 128), B), dim3(256), 0, (hipStream_t)stream, img,
                     (long long)n, keep_count);
  return nbm_launch_status();
}

extern "C" int nbm_rpn_select(const float* boxes, const uint32_t* keys, const int* keep_count, int B, int KA,
                              int top_n, int fail_below, int cap, float* sel_boxes, float* sel_scores, int* n_sel,
                              const int* seg, void* stream) {
  if (!boxes || !keys || !keep_count || !sel_boxes || !sel_scores || !n_sel || !seg || B <= 0 || KA <= 0) return NBM_EINVAL;
  if (cap < top_n || cap > 4096 || (cap & (cap - 1))) return NBM_EINVAL;
  const size_t shmem = (size_t)cap * 8 + 256 * 4;
  hipLaunchKernelGGL(rpn_select_kernel, dim3(B), dim3(SEL_THREADS), shmem, (hipStream_t)stream, boxes, keys,
                     keep_count, B, KA, top_n, fail_below, cap, sel_boxes, sel_scores, n_sel, seg);
  return nbm_launch_status();
}

extern "C" int nbm_nms_batched(const float* boxes, const float* scores, const int* n_in, int B, int cap,
                               float thresh, int post_n, uint64_t* mask_ws, int* keep_ws, float* rois,
                               float* roi_scores, int* n_out, const int* seg, void* stream) {
  if (!boxes || !scores || !n_in || !mask_ws || !keep_ws || !rois || !roi_scores || !n_out || !seg || B <= 0)
    return NBM_EINVAL;
  if (cap <= 0 || cap > 4096 || (cap & 63) || post_n <= 0 || post_n > cap) return NBM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int words = cap / 64;
  int* keep_idx = keep_ws;
  int* keep_cnt = keep_ws + (size_t)B * cap;
  hipLaunchKernelGGL(nms_mask_kernel, dim3(words, words, B), dim3(64), 0, st, boxes, n_in, cap, words, thresh,
                     reinterpret_cast<unsigned long long*>(mask_ws));
  hipLaunchKernelGGL(nms_scan_kernel, dim3(B), dim3(64), 0, st, reinterpret_cast<const unsigned long long*>(mask_ws),
                     n_in, cap, words, keep_idx, keep_cnt);
  hipLaunchKernelGGL(nms_gather_kernel, dim3(B), dim3(256), 0, st, boxes, scores, keep_idx, keep_cnt, B, cap, post_n,
                     rois, roi_scores, n_out, seg);
  return nbm_launch_status();
}

extern "C" int nbm_rpn_select_big_workspace(int B, int cap, int64_t* bytes) {
  if (!bytes || B <= 0 || cap < 64 || cap > BIG_CAP_MAX || (cap & (cap - 1))) return NBM_EINVAL;
  *bytes = (int64_t)B * cap * 8;
  return NBM_OK;
}

extern "C" int nbm_rpn_select_big(const float* boxes, const uint32_t* keys, const int* keep_count, int B, int KA,
                                  int top_n, int fail_below, int cap, void* ws, int64_t ws_bytes, float* sel_boxes,
                                  float* sel_scores, int* n_sel, const int* seg, void* stream) {
  if (!boxes || !keys || !keep_count || !ws || !sel_boxes || !sel_scores || !n_sel || !seg || B <= 0 || KA <= 0)
    return NBM_EINVAL;
  if (cap < top_n || cap < 64 || cap > BIG_CAP_MAX || (cap & (cap - 1)) || (((uintptr_t)ws) & 7u) ||
      ws_bytes < (int64_t)B * cap * 8)
    return NBM_EINVAL;
  hipLaunchKernelGGL(rpn_select_big_kernel, dim3(B), dim3(SEL_THREADS), 0, (hipStream_t)stream, boxes, keys, keep_count, B,
                     KA, top_n, fail_below, cap, static_cast<unsigned long long*>(ws), sel_boxes, sel_scores, n_sel, seg);
  return nbm_launch_status();
}

extern "C" int nbm_nms_big_workspace(int B, int cap, int64_t* bytes) {
  if (!bytes || B <= 0 || cap <= 0 || cap > BIG_CAP_MAX || (cap & 63)) return NBM_EINVAL;
  *bytes = (int64_t)nms_big_ws_bytes(B);
  return NBM_OK;
}

extern "C" int nbm_nms_big(const float* boxes, const float* scores, const int* n_in, int B, int cap, float thresh,
                           int post_n, void* ws, int64_t ws_bytes, float* rois, float* roi_scores, int* n_out,
                           const int* seg, void* stream) {
  if (!boxes || !scores || !n_in || !ws || !rois || !roi_scores || !n_out || !seg || B <= 0) return NBM_EINVAL;
  if (cap <= 0 || cap > BIG_CAP_MAX || (cap & 63) || post_n <= 0 || post_n > cap || (((uintptr_t)ws) & 3u) ||
      ws_bytes < (int64_t)nms_big_ws_bytes(B))
    return NBM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  int* keep_cnt = static_cast<int*>(ws);
  hipLaunchKernelGGL(nms_big_kernel, dim3(B), dim3(NMSB_THREADS), 0, st, boxes, scores, n_in, cap, thresh, post_n, rois,
                     roi_scores, keep_cnt);
  hipLaunchKernelGGL(nms_big_finish_kernel, dim3(B), dim3(256), 0, st, keep_cnt, B, post_n, rois, roi_scores, n_out, seg);
  return nbm_launch_status();
}

extern "C" int nbm_rcnn_post(const float* rois, const int* n_roi, int B, int roi_cap, const float* bbox_reg,
                             const float* bbox_cls, int n_cls1, int img_w, int img_h, float nms_thresh,
                             float min_score, int proposal_number, float* det, int* n_det, void* stream) {
  if (!rois || !n_roi || !bbox_reg || !bbox_cls || !det || !n_det || B <= 0 || roi_cap <= 0 || roi_cap > POST_MAX ||
      n_cls1 < 2)
    return NBM_EINVAL;
  hipLaunchKernelGGL(rcnn_post_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, rois, n_roi, roi_cap, bbox_reg,
                     bbox_cls, n_cls1, img_w, img_h, nms_thresh, min_score, proposal_number, det, n_det);
  return nbm_launch_status();
}

// IoU / best ground-truth box of the proposal target layer -- see nbm_hip.h.
extern "C" int nbm_proposal_iou(const float* rois, const float* gt, const int* n_gt, int B, int R, int G, float* mx, int* asg,
                                void* stream) {
  if (!rois || !gt || !n_gt || !mx || !asg || B <= 0 || R < 0 || G <= 0 || B > 65535) return NBM_EINVAL;
  hipLaunchKernelGGL(proposal_iou_kernel, dim3((R + G + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, rois, gt, n_gt, B, R, G,
                     mx, asg);
  return nbm_launch_status();
}

// AnchorTargetLayer: labels before subsampling + first best box of every inside anchor -- see nbm_hip.h.
extern "C" int nbm_anchor_targets(const float* anchors, int n_in, const float* gt, const int* n_gt, int B, int G, float neg_t,
                                  float pos_t, signed char* lab, short* amx, int* flag, void* stream) {
  if (!anchors || !gt || !n_gt || !lab || !amx || !flag || n_in <= 0 || B <= 0 || G <= 0) return NBM_EINVAL;
  if (G > ANCHOR_MAXG) return NBM_EUNSUPPORTED;
  hipLaunchKernelGGL(anchor_targets_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, anchors, n_in, gt, n_gt, G, neg_t, pos_t, lab,
                     amx, flag);
  return nbm_launch_status();
}
