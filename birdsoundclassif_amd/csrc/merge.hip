// Per-file merge of the detector's window outputs on device (reference run_detection.py:163-249):
// collect (border rules, shift, end-of-file drop, class-major compaction), greedy NMS over the whole file in
// the collected order for up to NBM_MERGE_MAX_N boxes, and the gather of the kept rows.
// Every compared value is computed with the reference's fp32 operations in its order, so contraction is off.
#include "nbm_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAX_BLOCKS = NBM_MERGE_MAX_N / 64;     // 64-box blocks of the NMS at its limit
constexpr int SCAN_THREADS = 1024;

// --------------------------------------------------------------------------------------------- collect
struct MergeRule {
  int n_img;
  float w_edge;       // w_pix - 5
  float min_border;   // float32(0.9 * (w_pix - hop)): torch compares an fp32 tensor with a Python float in fp32
  int hop;
  float spec_len;
};

// run_detection.py:190-209 / oracle/nets_ref.py:577-602 for one row of window i: the if/elif chain of the border rules
// (a single-window file takes the first-window rule only), the shift by hop * i (one fp32 add), the end-of-file drop.
__device__ __forceinline__ bool merge_row(const MergeRule& m, int i, const float* r, float* x1s, float* x2s) {
  const float x1 = r[1], x2 = r[3];
  const float wd = x2 - x1;
  bool drop;
  if (i == 0) drop = (x2 >= m.w_edge) && (wd < m.min_border);
  else if (i == m.n_img - 1) drop = (x1 <= 4.f) && (wd < m.min_border);
  else drop = ((x1 <= 4.f) || (x2 >= m.w_edge)) && (wd < m.min_border);
  if (drop) return false;
  const float sh = (float)(m.hop * i);
  *x1s = x1 + sh;
  *x2s = x2 + sh;
  return !(*x2s >= m.spec_len);
}

__device__ __forceinline__ int row_class(const float* r, int num_classes) {
  const float c = r[0];
  return (c >= 1.f && c <= (float)num_classes) ? (int)c : 0;
}

// one wave per window: surviving rows per (class, window) cell
__global__ __launch_bounds__(64) void collect_count_kernel(const float* __restrict__ det, const int* __restrict__ n_det,
                                                           int cap, int num_classes, MergeRule m, int* __restrict__ cell) {
  const int i = blockIdx.x;
  const int n = min(max(n_det[i], 0), cap);
  for (int r = threadIdx.x; r < n; r += 64) {
    const float* row = det + ((long long)i * cap + r) * 6;
    const int c = row_class(row, num_classes);
    float x1, x2;
    if (c && merge_row(m, i, row, &x1, &x2)) atomicAdd(&cell[(long long)(c - 1) * m.n_img + i], 1);
  }
}

// exclusive scan of the cells in class-major order (class 1..num_classes, then window), total -> *n_out
__global__ __launch_bounds__(SCAN_THREADS) void collect_scan_kernel(int* __restrict__ cell, int M, int* __restrict__ n_out) {
  __shared__ int part[SCAN_THREADS];
  const int t = threadIdx.x;
  const int per = (M + SCAN_THREADS - 1) / SCAN_THREADS;
  const int b = min(t * per, M), e = min(b + per, M);
  int s = 0;
  for (int k = b; k < e; ++k) s += cell[k];
  part[t] = s;
  __syncthreads();
  for (int d = 1; d < SCAN_THREADS; d <<= 1) {       // inclusive Hillis-Steele scan of the per-thread sums
    const int v = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = part[t] - s;
  for (int k = b; k < e; ++k) {
    const int c = cell[k];
    cell[k] = run;
    run += c;
  }
  if (t == SCAN_THREADS - 1) *n_out = part[t];
}

// one wave per window: every surviving row goes to its cell's offset + its rank among the cell's survivors.  The rows of a
// window are sorted by class, so a cell is one contiguous slice and the rank is (survivors before the row) - (survivors
// before the slice's first row).
__global__ __launch_bounds__(64) void collect_scatter_kernel(const float* __restrict__ det, const int* __restrict__ n_det,
                                                             int cap, int num_classes, MergeRule m, const int* __restrict__ off,
                                                             float* __restrict__ boxes, float* __restrict__ scores,
                                                             int* __restrict__ species) {
  const int i = blockIdx.x, lane = threadIdx.x;
  const int n = min(max(n_det[i], 0), cap);
  const long long out_cap = (long long)m.n_img * cap;
  const unsigned long long lt = (1ull << lane) - 1ull;
  const unsigned long long le = lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1ull;
  int carry_rank = 0, carry_start = 0;
  for (int base = 0; base < n; base += 64) {
    const int r = base + lane;
    const bool valid = r < n;
    const float* row = det + ((long long)i * cap + (valid ? r : 0)) * 6;
    int c = 0, pc = -1;
    float x1 = 0.f, x2 = 0.f;
    bool s = false;
    if (valid) {
      c = row_class(row, num_classes);
      pc = r > 0 ? row_class(row - 6, num_classes) : -1;
      s = c && merge_row(m, i, row, &x1, &x2);
    }
    const unsigned long long ms = __ballot(s);
    const unsigned long long mstart = __ballot(valid && c != pc);
    const int rank = carry_rank + __popcll(ms & lt);
    const unsigned long long st = mstart & le;
    int start_rank = carry_start;
    if (st) {
      const int L = 63 - __clzll((long long)st);
      start_rank = carry_rank + __popcll(ms & ((1ull << L) - 1ull));
    }
    if (s) {
      const long long pos = (long long)off[(long long)(c - 1) * m.n_img + i] + (rank - start_rank);
      if (pos >= 0 && pos < out_cap) {
        float* ob = boxes + pos * 4;
        ob[0] = x1; ob[1] = row[2]; ob[2] = x2; ob[3] = row[4];
        scores[pos] = row[5];
        species[pos] = c;
      }
    }
    carry_start = __shfl(start_rank, 63);
    carry_rank += __popcll(ms);
  }
}

// --------------------------------------------------------------------------------------------- greedy NMS
// IoU with the inclusive-pixel convention in the association order of oracle/nets_ref.py:284-294
__device__ __forceinline__ float iou_incl(const float* a, const float* b) {
  const float xi = fmaxf((fminf(a[2], b[2]) - fmaxf(a[0], b[0])) + 1.0f, 0.f);
  const float yi = fmaxf((fminf(a[3], b[3]) - fmaxf(a[1], b[1])) + 1.0f, 0.f);
  const float inter = xi * yi;
  const float aa = ((a[2] - a[0]) + 1.0f) * ((a[3] - a[1]) + 1.0f);
  const float ab = ((b[2] - b[0]) + 1.0f) * ((b[3] - b[1]) + 1.0f);
  return inter / ((aa + ab) - inter);
}

// Can a box of block a reach IoU >= thresh with a box of block b?  r = {min x1, max x2} of a block.  The x overlap of any pair
// is at most (min(max x2) - max(min x1)) + 1 with the same fp32 operations (they are monotone), and a pair without x overlap
// has IoU 0 (or NaN), which no positive threshold reaches.  NaN anywhere => "maybe".
__device__ __forceinline__ bool tile_may_hit(float2 a, float2 b, float thresh) {
  if (!(thresh > 0.f)) return true;
  const float xi = (fminf(a.y, b.y) - fmaxf(a.x, b.x)) + 1.0f;
  return !(xi <= 0.f);
}

// first word of row block rb in the packed upper triangle: tiles (rb, cb >= rb), 64 words each, cb-major within rb
__device__ __forceinline__ size_t tile_base(int rb, int nb) {
  return (size_t)64 * ((size_t)rb * nb - (size_t)rb * (rb - 1) / 2);
}

__device__ __forceinline__ int clamp_count(const int* n_in, int cap) { return min(max(*n_in, 0), cap); }

// one wave per 64-box block: its x-range (NaN coordinates widen it to everything)
__global__ __launch_bounds__(64) void nms_range_kernel(const float* __restrict__ boxes, const int* __restrict__ n_in, int cap,
                                                       float2* __restrict__ rng) {
  const int n = clamp_count(n_in, cap);
  const int rb = blockIdx.x, i = rb * 64 + threadIdx.x;
  if (rb * 64 >= n) return;
  float lo = INFINITY, hi = -INFINITY;
  if (i < n) {
    const float x1 = boxes[(long long)i * 4], x2 = boxes[(long long)i * 4 + 2];
    if (x1 != x1 || x2 != x2) { lo = -INFINITY; hi = INFINITY; }
    else { lo = x1; hi = x2; }
  }
  for (int d = 32; d > 0; d >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, d));
    hi = fmaxf(hi, __shfl_xor(hi, d));
  }
  if (threadIdx.x == 0) rng[rb] = make_float2(lo, hi);
}

constexpr int MASK_CB = 8;     // column blocks per workgroup of the mask kernel

// bits of row i in tile (rb, cb): bit jj <=> box cb*64+jj comes after i and has IoU >= thresh with it.  Tiles that cannot
// hold a bit (tile_may_hit) are neither computed nor written: the scan skips them by the same test.
__global__ __launch_bounds__(64) void nms_mask_kernel(const float* __restrict__ boxes, const int* __restrict__ n_in, int cap,
                                                      float thresh, const float2* __restrict__ rng,
                                                      unsigned long long* __restrict__ mask) {
  const int n = clamp_count(n_in, cap);
  const int nb = (n + 63) >> 6;
  const int rb = blockIdx.y, lane = threadIdx.x;
  if (rb >= nb) return;
  __shared__ float cbox[64][4];
  const int i = rb * 64 + lane;
  float me[4] = {0.f, 0.f, 0.f, 0.f};
  if (i < n) {
#pragma unroll
    for (int e = 0; e < 4; ++e) me[e] = boxes[(long long)i * 4 + e];
  }
  const float2 rr = rng[rb];
  const size_t base = tile_base(rb, nb);
  for (int k = 0; k < MASK_CB; ++k) {
    const int cb = blockIdx.x * MASK_CB + k;
    if (cb < rb || cb >= nb) continue;
    if (cb != rb && !tile_may_hit(rr, rng[cb], thresh)) continue;
    __syncthreads();
    const int j = cb * 64 + lane;
#pragma unroll
    for (int e = 0; e < 4; ++e) cbox[lane][e] = j < n ? boxes[(long long)j * 4 + e] : 0.f;
    __syncthreads();
    unsigned long long bits = 0ull;
    const int jn = min(64, n - cb * 64);
    if (i < n) {
      for (int jj = 0; jj < jn; ++jj)
        if (cb * 64 + jj > i && iou_incl(me, cbox[jj]) >= thresh) bits |= 1ull << jj;
    }
    mask[base + (size_t)(cb - rb) * 64 + lane] = bits;
  }
}

__device__ __forceinline__ unsigned long long readlane64(unsigned long long v, int k) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, k);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), k);
  return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ unsigned long long wave_or(unsigned long long v) {
  for (int d = 32; d > 0; d >>= 1) v |= __shfl_xor(v, d);
  return v;
}

// The greedy walk in one workgroup, one 64-box block per step, the removed bits of every box in LDS.  Wave 0 resolves the
// diagonal tile in registers (64 dependent bit steps, no global load in the chain); then the 16 waves OR the kept rows'
// off-diagonal tiles into the removed words of the later blocks (each later block is owned by one wave).
__global__ __launch_bounds__(SCAN_THREADS) void nms_scan_kernel(const int* __restrict__ n_in, int cap, float thresh,
                                                                const float2* __restrict__ rng,
                                                                const unsigned long long* __restrict__ mask,
                                                                int* __restrict__ keep, int* __restrict__ n_keep) {
  __shared__ unsigned long long removed[MAX_BLOCKS];
  __shared__ float2 srng[MAX_BLOCKS];
  __shared__ unsigned long long keep_sh;
  const int n = clamp_count(n_in, cap);
  const int nb = (n + 63) >> 6;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (int w = t; w < nb; w += SCAN_THREADS) { removed[w] = 0ull; srng[w] = rng[w]; }
  __syncthreads();
  const unsigned long long lt = (1ull << lane) - 1ull;
  int cnt = 0;
  for (int rb = 0; rb < nb; ++rb) {
    const size_t base = tile_base(rb, nb);
    if (wave == 0) {
      const int m = min(64, n - rb * 64);
      const unsigned long long diag = mask[base + lane];
      unsigned long long rem = readlane64(removed[rb], 0);
      if (m < 64) rem |= ~0ull << m;
#pragma unroll
      for (int k = 0; k < 64; ++k) {
        const unsigned long long d = readlane64(diag, k);
        rem |= ((rem >> k) & 1ull) ? 0ull : d;
      }
      const unsigned long long kp = ~rem;
      if ((kp >> lane) & 1ull) keep[cnt + __popcll(kp & lt)] = rb * 64 + lane;
      if (lane == 0) keep_sh = kp;
    }
    __syncthreads();
    const unsigned long long kp = keep_sh;
    cnt += __popcll(kp);
    if (kp) {
      const float2 rr = srng[rb];
      const bool mine = (kp >> lane) & 1ull;
      for (int c0 = rb + 1 + wave * 64; c0 < nb; c0 += SCAN_THREADS) {
        const int cb = c0 + lane;
        unsigned long long hits = __ballot(cb < nb && tile_may_hit(rr, srng[min(cb, nb - 1)], thresh));
        while (hits) {
          const int h = __ffsll((long long)hits) - 1;
          hits &= hits - 1ull;
          const int c = c0 + h;
          unsigned long long v = mine ? mask[base + (size_t)(c - rb) * 64 + lane] : 0ull;
          v = wave_or(v);
          if (lane == 0 && v) removed[c] |= v;
        }
      }
    }
    __syncthreads();
  }
  if (t == 0) *n_keep = cnt;
}

// --------------------------------------------------------------------------------------------- gather
__global__ void gather_kernel(const float* __restrict__ boxes, const float* __restrict__ scores, const int* __restrict__ species,
                              const int* __restrict__ keep, const int* __restrict__ n_keep, int cap, float* __restrict__ rows,
                              int* __restrict__ n_rows) {
  const int cnt = clamp_count(n_keep, cap);
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r == 0) *n_rows = cnt;
  if (r >= cnt) return;
  const int k = keep[r];
  if (k < 0 || k >= cap) return;
  float* o = rows + (long long)r * 6;
  o[0] = (float)species[k];
  o[1] = boxes[(long long)k * 4]; o[2] = boxes[(long long)k * 4 + 1];
  o[3] = boxes[(long long)k * 4 + 2]; o[4] = boxes[(long long)k * 4 + 3];
  o[5] = scores[k];
}

size_t nms_ws_bytes(int cap) {
  const size_t nb = (size_t)(cap + 63) / 64;
  return 256 + (nb * sizeof(float2) + 255) / 256 * 256 + nb * (nb + 1) / 2 * 64 * sizeof(unsigned long long);
}

}  // namespace

extern "C" int nbm_merge_collect(const float* det, const int* n_det, int n_img, int cap, int num_classes, int w_pix, int hop,
                                 int64_t spectrogram_length, int* cell_ws, float* boxes, float* scores, int* species,
                                 int* n_out, void* stream) {
  if (!det || !n_det || !cell_ws || !boxes || !scores || !species || !n_out) return NBM_EINVAL;
  if (n_img <= 0 || cap <= 0 || num_classes <= 0 || (long long)n_img * cap > (1ll << 30) ||
      (long long)n_img * num_classes > (1ll << 30))
    return NBM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  MergeRule m;
  m.n_img = n_img;
  m.w_edge = (float)(w_pix - 5);
  m.min_border = (float)(0.9 * (double)(w_pix - hop));
  m.hop = hop;
  m.spec_len = (float)spectrogram_length;
  const int M = n_img * num_classes;
  const hipError_t e = nbm_zero_async(cell_ws, (size_t)M * sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(collect_count_kernel, dim3(n_img), dim3(64), 0, st, det, n_det, cap, num_classes, m, cell_ws);
  hipLaunchKernelGGL(collect_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, cell_ws, M, n_out);
  hipLaunchKernelGGL(collect_scatter_kernel, dim3(n_img), dim3(64), 0, st, det, n_det, cap, num_classes, m, cell_ws, boxes,
                     scores, species);
  return nbm_launch_status();
}

extern "C" int nbm_merge_nms_workspace(int cap, int64_t* bytes) {
  if (!bytes || cap < 0 || cap > NBM_MERGE_MAX_N) return NBM_EINVAL;
  *bytes = (int64_t)nms_ws_bytes(cap);
  return NBM_OK;
}

extern "C" int nbm_merge_nms(const float* boxes, const int* n_in, int cap, float thresh, void* ws, int64_t ws_bytes,
                             int* keep, int* n_keep, void* stream) {
  if (!boxes || !n_in || !ws || !keep || !n_keep || cap < 0 || cap > NBM_MERGE_MAX_N) return NBM_EINVAL;
  if (ws_bytes < (int64_t)nms_ws_bytes(cap)) return NBM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int nb = (cap + 63) / 64;
  float2* rng = reinterpret_cast<float2*>(static_cast<char*>(ws) + 256);
  unsigned long long* mask = reinterpret_cast<unsigned long long*>(
      static_cast<char*>(ws) + 256 + ((size_t)nb * sizeof(float2) + 255) / 256 * 256);
  if (nb > 0) {
    hipLaunchKernelGGL(nms_range_kernel, dim3(nb), dim3(64), 0, st, boxes, n_in, cap, rng);
    hipLaunchKernelGGL(nms_mask_kernel, dim3((nb + MASK_CB - 1) / MASK_CB, nb), dim3(64), 0, st, boxes, n_in, cap, thresh,
                       rng, mask);
  }
  hipLaunchKernelGGL(nms_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, n_in, cap, thresh, rng, mask, keep, n_keep);
  return nbm_launch_status();
}

extern "C" int nbm_merge_gather(const float* boxes, const float* scores, const int* species, const int* keep,
                                const int* n_keep, int cap, float* rows, int* n_rows, void* stream) {
  if (!boxes || !scores || !species || !keep || !n_keep || !rows || !n_rows || cap < 0 || cap > NBM_MERGE_MAX_N)
    return NBM_EINVAL;
  hipLaunchKernelGGL(gather_kernel, dim3(max(1, (cap + 255) / 256)), dim3(256), 0, (hipStream_t)stream, boxes, scores,
                     species, keep, n_keep, cap, rows, n_rows);
  return nbm_launch_status();
}
