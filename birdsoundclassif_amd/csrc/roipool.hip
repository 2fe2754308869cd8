// Everything that depends on the RoI window (include/nbm_hip.h): RoI pooling at any pool size and its gradient
// (nbm_roi_pool_hw / nbm_roi_pool_hw_bwd; nbm_roi_pool / nbm_roi_pool_bwd forward to them with a 2 x 2 pool), the tile lists
// under the 2 x 2 windows of a demand-driven level (nbm_roi_tiles) and the re-zeroing of those windows in a persistent
// gradient map (nbm_zero_roi_windows).  roi_level and roi_window below are the only statement of the window: the tile lists,
// the footprint re-zeroing and the pooling agree because they call them.
#include "nbm_common.h"
#include <cstddef>
#include <cstring>

namespace {

struct RoiHwParams {
  const float* fmap[5]; int fh[5], fw[5]; int n_levels, C;
  const float* rois; const int* n_roi; int B, roi_cap;
  const float* pe_f; const float* pe_t; int img_h, img_w;
  float* pool; float* pe; int* level;
  int ph, pw, vec;
};

struct RoiHwBwdParams {
  float* gfmap[5]; int fh[5], fw[5]; int n_levels, C;
  const float* rois; const int* level; int B, n_roi; const float* gpool;
  int ph, pw;
};

// Pyramid level of a RoI, layers.py:408-417 (sizes WITHOUT the +1).
__device__ __forceinline__ int roi_level(const float* roi, int n_levels) {
  const float size = sqrtf((roi[2] - roi[0]) * (roi[3] - roi[1]));
  const float lf = logf(size * 0.1f) / 0.6931471805599453f;
  int lvl = (lf != lf) ? (int)0x80000000 : (lf <= -2147483648.f ? (int)0x80000000 : (lf >= 2147483648.f ? (int)0x80000000 : (int)lf));
  return min(max(lvl, 0), n_levels - 1);
}

// Feature-map window of a RoI on level `lvl`, layers.py:424-427 (round), :450-465 (y2 clamp, growth to at least ph x pw).
// The reference grows with `while size < pool: ...`, which never ends when the pool exceeds the map; here the pool fits every
// map (checked on the host) and the loop is bounded by the pool size: a RoI inside the image starts at a height >= 0 and a
// width >= 1 and gains at least one row / column per round from the second round on, so the bound is never what ends it.
// Rows read: y1..y2, columns: x1..min(x2, W-1); x2 itself stays unclamped for the positional encoding.
// -> false for a window with no pixel in the map (coordinates outside the image: nothing is read or written for it).
__device__ __forceinline__ bool roi_window(const float* roi, int lvl, int H, int W, int ph, int pw, int& x1, int& y1, int& x2,
                                           int& y2) {
  const float stride = (float)(2 << lvl);
  x1 = (int)rintf(roi[0] / stride); y1 = (int)rintf(roi[1] / stride);
  x2 = (int)rintf(roi[2] / stride); y2 = (int)rintf(roi[3] / stride);
  y2 = min(y2, H - 1);
  const int rounds = max(ph, pw);
  for (int k = 0; k < rounds && y2 - y1 + 1 < ph; ++k) { y1 = max(0, y1 - 1); y2 = min(H - 1, y2 + 1); }
  for (int k = 0; k < rounds && x2 - x1 + 1 < pw; ++k) { x1 = max(0, x1 - 1); x2 = min(W - 1, x2 + 1); }
  // (x2 == W with x2 - x1 + 1 == pw is not grown and reads pw - 1 columns: the bins below take any window of >= 1 pixel)
  return x1 >= 0 && y1 >= 0 && y2 <= H - 1 && y2 >= y1 && min(x2, W - 1) >= x1;
}

// One workgroup per RoI slot; work items are (bin, channel quad) for the map and (bin row | bin column, channel) for the
// separable positional encoding.
__global__ __launch_bounds__(256) void roi_pool_hw_kernel(const RoiHwParams p) {
  const int slot = blockIdx.x;                 // b * roi_cap + r
  const int b = slot / p.roi_cap, r = slot - b * p.roi_cap;
  if (r >= p.n_roi[b]) return;
  const float* roi = p.rois + (long long)slot * 4;
  const int lvl = roi_level(roi, p.n_levels);
  const int H = p.fh[lvl], W = p.fw[lvl], ph = p.ph, pw = p.pw;
  int x1, y1, x2, y2;
  const bool inside = roi_window(roi, lvl, H, W, ph, pw, x1, y1, x2, y2);
  if (threadIdx.x == 0) p.level[slot] = lvl;
  if (!inside) return;
  const int C = p.C, half = C >> 1, nbin = ph * pw;
  const float* fm = p.fmap[lvl] + ((long long)b * H + y1) * W * C + (long long)x1 * C;
  float* out = p.pool + (long long)slot * nbin * C;
  const int h = y2 - y1 + 1, w = min(x2, W - 1) - x1 + 1;
  if (p.vec) {
    const int C4 = C >> 2;
    for (int it = threadIdx.x; it < nbin * C4; it += blockDim.x) {
      const int bin = it / C4, q = it - bin * C4;
      const int i = bin / pw, j = bin - i * pw;
      const int ya = (i * h) / ph, yb = ((i + 1) * h + ph - 1) / ph;
      const int xa = (j * w) / pw, xb = ((j + 1) * w + pw - 1) / pw;
      f32x4 sum = {0.f, 0.f, 0.f, 0.f};
      for (int yy = ya; yy < yb; ++yy) {
        const f32x4* row = reinterpret_cast<const f32x4*>(fm + (long long)yy * W * C) + q;
        for (int xx = xa; xx < xb; ++xx) sum += row[xx * C4];
      }
      const float area = (float)((yb - ya) * (xb - xa));
      f32x4 o = {sum.x / area, sum.y / area, sum.z / area, sum.w / area};
      reinterpret_cast<f32x4*>(out + (long long)bin * C)[q] = o;
    }
  } else {
    for (int it = threadIdx.x; it < nbin * C; it += blockDim.x) {
      const int bin = it / C, c = it - bin * C;
      const int i = bin / pw, j = bin - i * pw;
      const int ya = (i * h) / ph, yb = ((i + 1) * h + ph - 1) / ph;
      const int xa = (j * w) / pw, xb = ((j + 1) * w + pw - 1) / pw;
      float sum = 0.f;
      for (int yy = ya; yy < yb; ++yy)
        for (int xx = xa; xx < xb; ++xx) sum += fm[((long long)yy * W + xx) * C + c];
      out[(long long)bin * C + c] = sum / (float)((yb - ya) * (xb - xa));
    }
  }
  // positional encoding: channels [0, C/2) are bin means of pe_frequency[s*y1 : s*y2] (rows only), [C/2, C) of
  // pe_time[: s*(x2-x1)] (columns only, x2 unclamped), layers.py:484-489; summed in double, rounded once
  const int s = 2 << lvl;
  const int f0 = s * y1, f1 = min(s * y2, p.img_h), hf = f1 - f0;
  const int wt = min(s * (x2 - x1), p.img_w);
  if (hf < 1 || wt < 1) return;                // maps that are not this image's pyramid: no table row to read
  float* pe = p.pe + (long long)slot * nbin * C;
  for (int it = threadIdx.x; it < (ph + pw) * half; it += blockDim.x) {
    const int k = it / half, c = it - k * half;
    if (k < ph) {
      const int ra = (k * hf) / ph, rb = ((k + 1) * hf + ph - 1) / ph;
      double acc = 0.0;
      for (int q = ra; q < rb; ++q) acc += (double)p.pe_f[(long long)(f0 + q) * half + c];
      const float v = (float)(acc / (double)(rb - ra));
      for (int j = 0; j < pw; ++j) pe[(long long)(k * pw + j) * C + c] = v;
    } else {
      const int j = k - ph;
      const int ca = (j * wt) / pw, cb = ((j + 1) * wt + pw - 1) / pw;
      double acc = 0.0;
      for (int q = ca; q < cb; ++q) acc += (double)p.pe_t[(long long)q * half + c];
      const float v = (float)(acc / (double)(cb - ca));
      for (int i = 0; i < ph; ++i) pe[(long long)(i * pw + j) * C + half + c] = v;
    }
  }
}

// Scatter-add with fp32 atomics: RoI windows overlap, so the order of the sums (and the last bits of the result) is not fixed.
__global__ __launch_bounds__(256) void roi_pool_hw_bwd_kernel(const RoiHwBwdParams p) {
  const int slot = blockIdx.x;
  const int b = slot / p.n_roi;
  const float* roi = p.rois + (long long)slot * 4;
  const int lvl = min(max(p.level[slot], 0), p.n_levels - 1);
  const int H = p.fh[lvl], W = p.fw[lvl], ph = p.ph, pw = p.pw;
  int x1, y1, x2, y2;
  if (!roi_window(roi, lvl, H, W, ph, pw, x1, y1, x2, y2)) return;
  const int C = p.C, nbin = ph * pw;
  float* gf = p.gfmap[lvl] + ((long long)b * H + y1) * W * C + (long long)x1 * C;
  const float* g = p.gpool + (long long)slot * nbin * C;
  const int h = y2 - y1 + 1, w = min(x2, W - 1) - x1 + 1;
  // work items are (bin, channel): neighbouring lanes add to neighbouring floats (a lane per channel quad spreads each atomic
  // instruction over four times the cache lines: 4.2 x slower at 2 x 2, measured)
  for (int it = threadIdx.x; it < nbin * C; it += blockDim.x) {
    const int bin = it / C, c = it - bin * C;
    const int i = bin / pw, j = bin - i * pw;
    const int ya = (i * h) / ph, yb = ((i + 1) * h + ph - 1) / ph;
    const int xa = (j * w) / pw, xb = ((j + 1) * w + pw - 1) / pw;
    const float gv = g[(long long)bin * C + c] / (float)((yb - ya) * (xb - xa));
    for (int yy = ya; yy < yb; ++yy)
      for (int xx = xa; xx < xb; ++xx) atomicAdd(gf + ((long long)yy * W + xx) * C + c, gv);
  }
}

// The deterministic twin (nbm_roi_pool_hw_bwd_det): the same sums in GATHER form.  A workgroup owns a 16 x 16 pixel tile of one level and
// one image (blockIdx = tile, image; one launch per level).  It walks the image's RoIs in index order, 256 at a time: thread r works out
// RoI r's window once (roi_window, the one statement of it) into LDS, then every (pixel, channel) work item of the tile adds, RoI by RoI
// and bin by bin in ascending order, the shares of the bins that contain its pixel, and adds the total to the map once.  No atomic, one
// fixed order per element.  A pixel outside every window is not written, so the kernel stays inside the footprint that
// nbm_zero_roi_windows restores (the persistent demand-driven maps keep working), and a tile that no window touches costs its
// workgroup the window pass only.  Cost: the window pass is B x tiles x n_roi roi_window calls, the gather loop visits n_roi LDS records
// per work item -- linear in n_roi where the scatter form is constant; 16 RoIs per image in training, 1 000 at the evaluation geometry.
struct RoiWin { int x1, y1, w, h; };      // w = 0: not on this level / no pixel in the map

__global__ __launch_bounds__(256) void roi_pool_hw_bwd_gather_kernel(const RoiHwBwdParams p, int lvl) {
  __shared__ RoiWin win[256];
  __shared__ int any_s;
  const int H = p.fh[lvl], W = p.fw[lvl], ph = p.ph, pw = p.pw, C = p.C, nbin = ph * pw;
  const int tiles_x = (W + 15) >> 4;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x, b = blockIdx.y;
  const int py0 = ty * 16, px0 = tx * 16;
  const int th = min(16, H - py0), tw = min(16, W - px0);
  float* gmap = p.gfmap[lvl] + (long long)b * H * W * C;
  for (int r0 = 0; r0 < p.n_roi; r0 += 256) {
    __syncthreads();                                    // the previous chunk's records are consumed
    if (threadIdx.x == 0) any_s = 0;
    __syncthreads();
    const int r = r0 + threadIdx.x;
    RoiWin wn = {0, 0, 0, 0};
    if (r < p.n_roi) {
      const long long slot = (long long)b * p.n_roi + r;
      if (min(max(p.level[slot], 0), p.n_levels - 1) == lvl) {
        int x1, y1, x2, y2;
        if (roi_window(p.rois + slot * 4, lvl, H, W, ph, pw, x1, y1, x2, y2)) {
          const int w = min(x2, W - 1) - x1 + 1, h = y2 - y1 + 1;
          if (x1 < px0 + tw && x1 + w > px0 && y1 < py0 + th && y1 + h > py0) { wn = {x1, y1, w, h}; any_s = 1; }   // (benign: all store 1)
        }
      }
    }
    win[threadIdx.x] = wn;
    __syncthreads();
    if (!any_s) continue;                               // uniform
    const int nr = min(256, p.n_roi - r0);
    for (int it = threadIdx.x; it < th * tw * C; it += 256) {
      const int c = it % C, px = it / C;
      const int yy = py0 + px / tw, xx = px0 + px % tw;
      float acc = 0.f;
      bool hit = false;
      for (int k = 0; k < nr; ++k) {
        const RoiWin q = win[k];
        const int dy = yy - q.y1, dx = xx - q.x1;
        if (q.w == 0 || (unsigned)dy >= (unsigned)q.h || (unsigned)dx >= (unsigned)q.w) continue;
        hit = true;
        const float* g = p.gpool + ((long long)b * p.n_roi + r0 + k) * nbin * C + c;
        for (int i = 0; i < ph; ++i) {
          const int ya = (i * q.h) / ph, yb = ((i + 1) * q.h + ph - 1) / ph;
          if (dy < ya || dy >= yb) continue;
          for (int j = 0; j < pw; ++j) {
            const int xa = (j * q.w) / pw, xb = ((j + 1) * q.w + pw - 1) / pw;
            if (dx < xa || dx >= xb) continue;
            acc += g[(long long)(i * pw + j) * C] / (float)((yb - ya) * (xb - xa));
          }
        }
      }
      if (hit) { float* o = gmap + ((long long)yy * W + xx) * C + c; *o = *o + acc; }
    }
  }
}

// ------------------------------------------------------------------ demand-driven pyramid level: tiles under the RoIs
// The finest FPN output map is read by two consumers only: the RPN's stride-8 depthwise convolution (a fixed pixel pattern)
// and the RoI pooling of the RoIs assigned to that level.  This kernel lists the 2 x 2 Winograd output tiles of level `level`
// that the 2 x 2 pool's RoI windows touch (minus the tiles in `skip`, which the fixed pattern has computed already): one
// workgroup per image, an LDS bitmap, then an ordered compaction into 128-entry blocks (entries = b * TH * TW + ty * TW + tx,
// ascending, -1 padded, a block never mixes images); blocks are handed out by an atomic counter, so the filled blocks are the
// leading *n_blocks ones of `tiles` (capacity B * ceil(TH * TW / 128) blocks: cannot overflow).
struct RoiTilesParams {
  const float* rois; const int* n_roi; int B, roi_cap, n_levels, level, H, W;
  const unsigned char* skip; int* tiles; int* n_blocks; int dilate;
  int* counts;           // deterministic twin: [B] blocks of every image (pass 1), placed by their exclusive prefix (pass 2); else null
};

// PASS 0: the default (blocks handed out by the atomic counter).  Deterministic twin: PASS 1 only counts (counts[b] = blocks of image b),
// PASS 2 places image b's blocks at the exclusive prefix of counts -- the list is then ascending in (image, tile id) whatever the order the
// workgroups run in -- and image 0's workgroup stores the total into *n_blocks.
template <int PASS>
__global__ __launch_bounds__(256) void roi_tiles_kernel(const RoiTilesParams p) {
  extern __shared__ unsigned bits[];
  __shared__ int part[256];
  __shared__ int base_s;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int H = p.H, W = p.W;
  const int TH = (H + 1) >> 1, TW = (W + 1) >> 1, THW = TH * TW;
  const int n_words = (THW + 31) >> 5;
  for (int i = tid; i < n_words; i += 256) bits[i] = 0u;
  __syncthreads();
  const int n = min(p.n_roi[b], p.roi_cap);
  for (int r = tid; r < n; r += 256) {
    const float* roi = p.rois + ((long long)b * p.roi_cap + r) * 4;
    int x1, y1, x2, y2;
    if (roi_level(roi, p.n_levels) != p.level || !roi_window(roi, p.level, H, W, 2, 2, x1, y1, x2, y2)) continue;
    const int dl = p.dilate;           // > 0: the tiles within `dilate` pixels of the window (support of a 3x3 data gradient)
    const int ty0 = max(y1 - dl, 0) >> 1, ty1 = min(y2 + dl, H - 1) >> 1, tx0 = max(x1 - dl, 0) >> 1, tx1 = min(min(x2, W - 1) + dl, W - 1) >> 1;
    for (int ty = ty0; ty <= ty1; ++ty)
      for (int tx = tx0; tx <= tx1; ++tx) {
        const int id = ty * TW + tx;
        if (p.skip && p.skip[id]) continue;
        atomicOr(&bits[id >> 5], 1u << (id & 31));
      }
  }
  __syncthreads();
  // ordered compaction: thread t owns the words [t * wpt, (t + 1) * wpt)
  const int wpt = (n_words + 255) / 256;
  int cnt = 0;
  for (int i = tid * wpt; i < min((tid + 1) * wpt, n_words); ++i) cnt += __popc(bits[i]);
  part[tid] = cnt;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int i = 0; i < 256; ++i) { const int c = part[i]; part[i] = run; run += c; }
    if (PASS == 0) base_s = run ? atomicAdd(p.n_blocks, (run + 127) >> 7) : 0;
    else if (PASS == 1) p.counts[b] = (run + 127) >> 7;
    else {
      int before = 0, all = 0;
      for (int i = 0; i < p.B; ++i) { if (i < b) before += p.counts[i]; all += p.counts[i]; }
      base_s = before;
      if (b == 0) *p.n_blocks = all;
    }
    part[0] = 0;
    bits[n_words] = (unsigned)run;                               // total, one spare word
  }
  __syncthreads();
  const int total = (int)bits[n_words];
  if (!total || PASS == 1) return;
  int* out = p.tiles + (long long)base_s * 128;
  int o = part[tid];
  for (int i = tid * wpt; i < min((tid + 1) * wpt, n_words); ++i) {
    unsigned wbits = bits[i];
    while (wbits) {
      const int bit = __ffs(wbits) - 1;
      wbits &= wbits - 1;
      out[o++] = b * THW + (i << 5) + bit;
    }
  }
  const int padded = ((total + 127) >> 7) << 7;
  for (int i = total + tid; i < padded; i += 256) out[i] = -1;
}

// Targeted re-zeroing of the persistent gradient map of a demand-driven FPN level (nbm_hip.h: nbm_zero_*): the map is zero
// everywhere except where its writers left something, so restoring it costs their footprint, not a fill of the whole map.
// This one undoes roi_pool_hw_bwd_kernel's scatter of a 2 x 2 pool on level `lvl`.
__global__ void zero_roi_windows_kernel(float* __restrict__ g, int H, int W, int C4, const float* __restrict__ rois,
                                        const int* __restrict__ level, int n_roi, int lvl) {
  const int slot = blockIdx.x;
  if (level[slot] != lvl) return;
  const int b = slot / n_roi;
  int x1, y1, x2, y2;
  if (!roi_window(rois + (long long)slot * 4, lvl, H, W, 2, 2, x1, y1, x2, y2)) return;
  const int h = y2 - y1 + 1, w = min(x2, W - 1) - x1 + 1;
  f32x4* g4 = reinterpret_cast<f32x4*>(g);
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  for (int i = threadIdx.x; i < h * w * C4; i += blockDim.x) {
    const int c = i % C4, px = i / C4;
    const int yy = px / w, xx = px - yy * w;
    g4[(((long long)b * H + y1 + yy) * W + x1 + xx) * C4 + c] = z;
  }
}

// Shared argument rule of both entry points: the pool must fit the smallest map (the growth loop needs it to end) and have
// at least two rows and columns (a one-row window has an empty positional-encoding slice).
int roi_hw_check(int n_levels, int C, const int* fh, const int* fw, int ph, int pw) {
  if (n_levels < 1 || n_levels > 5 || C <= 0 || (C & 1) || !fh || !fw) return NBM_EINVAL;
  if (ph < 2 || pw < 2) return NBM_EUNSUPPORTED;
  for (int i = 0; i < n_levels; ++i) {
    if (fh[i] < 2 || fw[i] < 2) return NBM_EINVAL;
    if (ph > fh[i] || pw > fw[i]) return NBM_EUNSUPPORTED;
  }
  return NBM_OK;
}

}  // namespace

extern "C" int nbm_roi_pool_hw(const nbm_roi_hw_desc* d, void* stream) {
  if (!d || !d->rois || !d->n_roi || !d->pool || !d->pe || !d->level || !d->pe_f || !d->pe_t) return NBM_EINVAL;
  if (d->B <= 0 || d->roi_cap <= 0 || d->img_h <= 0 || d->img_w <= 0) return NBM_EINVAL;
  const int rc = roi_hw_check(d->n_levels, d->C, d->fh, d->fw, d->pool_h, d->pool_w);
  if (rc) return rc;
  if ((long long)d->B * d->roi_cap > 0x7fffffffLL) return NBM_EINVAL;
  RoiHwParams p;
  bool vec = (d->C & 3) == 0 && nbm_aligned16(d->pool);
  for (int i = 0; i < 5; ++i) {
    const bool on = i < d->n_levels;
    if (on && !d->fmap[i]) return NBM_EINVAL;
    p.fmap[i] = on ? d->fmap[i] : nullptr; p.fh[i] = on ? d->fh[i] : 0; p.fw[i] = on ? d->fw[i] : 0;
    if (on) vec = vec && nbm_aligned16(d->fmap[i]);
  }
  p.n_levels = d->n_levels; p.C = d->C; p.rois = d->rois; p.n_roi = d->n_roi; p.B = d->B; p.roi_cap = d->roi_cap;
  p.pe_f = d->pe_f; p.pe_t = d->pe_t; p.img_h = d->img_h; p.img_w = d->img_w;
  p.pool = d->pool; p.pe = d->pe; p.level = d->level;
  p.ph = d->pool_h; p.pw = d->pool_w; p.vec = vec ? 1 : 0;
  hipLaunchKernelGGL(roi_pool_hw_kernel, dim3(d->B * d->roi_cap), dim3(256), 0, (hipStream_t)stream, p);
  return nbm_launch_status();
}

static int roi_pool_hw_bwd_impl(float* const* gfmap, const int* fh, const int* fw, int n_levels, int C, const float* rois,
                                const int* level, int B, int n_roi, int pool_h, int pool_w, const float* gpool,
                                int deterministic, void* stream) {
  if (!gfmap || !rois || !level || !gpool || B <= 0 || n_roi <= 0) return NBM_EINVAL;
  const int rc = roi_hw_check(n_levels, C, fh, fw, pool_h, pool_w);
  if (rc) return rc;
  if ((long long)B * n_roi > 0x7fffffffLL) return NBM_EINVAL;
  RoiHwBwdParams p;
  for (int i = 0; i < 5; ++i) {
    const bool on = i < n_levels;
    if (on && !gfmap[i]) return NBM_EINVAL;
    p.gfmap[i] = on ? gfmap[i] : nullptr; p.fh[i] = on ? fh[i] : 0; p.fw[i] = on ? fw[i] : 0;
  }
  p.n_levels = n_levels; p.C = C; p.rois = rois; p.level = level; p.B = B; p.n_roi = n_roi; p.gpool = gpool;
  p.ph = pool_h; p.pw = pool_w;
  if (deterministic) {
    if (B > 65535) return NBM_EUNSUPPORTED;
    for (int l = 0; l < n_levels; ++l)
      hipLaunchKernelGGL(roi_pool_hw_bwd_gather_kernel, dim3(((fh[l] + 15) / 16) * ((fw[l] + 15) / 16), B), dim3(256), 0,
                         (hipStream_t)stream, p, l);
    return nbm_launch_status();
  }
  hipLaunchKernelGGL(roi_pool_hw_bwd_kernel, dim3(B * n_roi), dim3(256), 0, (hipStream_t)stream, p);
  return nbm_launch_status();
}
extern "C" int nbm_roi_pool_hw_bwd(float* const* gfmap, const int* fh, const int* fw, int n_levels, int C, const float* rois,
                                   const int* level, int B, int n_roi, int pool_h, int pool_w, const float* gpool,
                                   void* stream) {
  return roi_pool_hw_bwd_impl(gfmap, fh, fw, n_levels, C, rois, level, B, n_roi, pool_h, pool_w, gpool, 0, stream);
}
extern "C" int nbm_roi_pool_hw_bwd_det(float* const* gfmap, const int* fh, const int* fw, int n_levels, int C, const float* rois,
                                       const int* level, int B, int n_roi, int pool_h, int pool_w, const float* gpool,
                                       void* stream) {
  return roi_pool_hw_bwd_impl(gfmap, fh, fw, n_levels, C, rois, level, B, n_roi, pool_h, pool_w, gpool, 1, stream);
}

// The 2 x 2 entries of the ABI: the same checks and kernels with the pool size filled in.
static_assert(offsetof(nbm_roi_hw_desc, pool_h) == sizeof(nbm_roi_desc), "nbm_roi_hw_desc is nbm_roi_desc plus the pool size");

extern "C" int nbm_roi_pool(const nbm_roi_desc* d, void* stream) {
  if (!d) return NBM_EINVAL;
  nbm_roi_hw_desc h;
  memcpy(&h, d, sizeof(*d));
  h.pool_h = h.pool_w = 2;
  return nbm_roi_pool_hw(&h, stream);
}

extern "C" int nbm_roi_pool_bwd(float* const* gfmap, const int* fh, const int* fw, int n_levels, int C, const float* rois,
                                const int* level, int B, int n_roi, const float* gpool, void* stream) {
  return nbm_roi_pool_hw_bwd(gfmap, fh, fw, n_levels, C, rois, level, B, n_roi, 2, 2, gpool, stream);
}

// RoI windows of pyramid level `level` -> list of the 2 x 2 output tiles they touch -- see nbm_hip.h.
// `counts` NULL: the default placement (atomic counter); else [B] ints of scratch for the deterministic placement
static int roi_tiles_impl(const float* rois, const int* n_roi, int B, int roi_cap, int n_levels, int level,
                          const int* fh, const int* fw, const unsigned char* skip, int dilate, int* tiles, int* n_blocks,
                          int* counts, void* stream) {
  if (!rois || !n_roi || !fh || !fw || !tiles || !n_blocks || B <= 0 || roi_cap <= 0 || n_levels < 1 || n_levels > 5 ||
      level < 0 || level >= n_levels || dilate < 0 || dilate > 2)
    return NBM_EINVAL;
  for (int i = 0; i < n_levels; ++i)
    if (fh[i] < 2 || fw[i] < 2) return NBM_EINVAL;
  RoiTilesParams p{};
  p.rois = rois; p.n_roi = n_roi; p.B = B; p.roi_cap = roi_cap; p.n_levels = n_levels; p.level = level;
  p.H = fh[level]; p.W = fw[level];
  p.skip = skip; p.tiles = tiles; p.n_blocks = n_blocks; p.dilate = dilate;
  const int thw = ((p.H + 1) >> 1) * ((p.W + 1) >> 1);
  const size_t lds = (size_t)(((thw + 31) >> 5) + 1) * 4;
  if (lds > 60000) return NBM_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (counts) {
    p.counts = counts;
    hipLaunchKernelGGL(roi_tiles_kernel<1>, dim3(B), dim3(256), lds, st, p);
    hipLaunchKernelGGL(roi_tiles_kernel<2>, dim3(B), dim3(256), lds, st, p);
    return nbm_launch_status();
  }
  hipError_t e = nbm_zero_async(n_blocks, sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(roi_tiles_kernel<0>, dim3(B), dim3(256), lds, st, p);
  return nbm_launch_status();
}
extern "C" int nbm_roi_tiles(const float* rois, const int* n_roi, int B, int roi_cap, int n_levels, int level,
                             const int* fh, const int* fw, const unsigned char* skip, int dilate, int* tiles, int* n_blocks,
                             void* stream) {
  return roi_tiles_impl(rois, n_roi, B, roi_cap, n_levels, level, fh, fw, skip, dilate, tiles, n_blocks, nullptr, stream);
}
extern "C" int nbm_roi_tiles_det(const float* rois, const int* n_roi, int B, int roi_cap, int n_levels, int level,
                                 const int* fh, const int* fw, const unsigned char* skip, int dilate, int* tiles, int* n_blocks,
                                 int* counts, void* stream) {
  if (!counts) return NBM_EINVAL;
  return roi_tiles_impl(rois, n_roi, B, roi_cap, n_levels, level, fh, fw, skip, dilate, tiles, n_blocks, counts, stream);
}

extern "C" int nbm_zero_roi_windows(float* g, int H, int W, int C, const float* rois, const int* level, int B, int n_roi, int lvl,
                                    void* stream) {
  if (!g || !rois || !level || B <= 0 || n_roi <= 0 || H < 2 || W < 2 || C <= 0 || (C & 3) || lvl < 0 || lvl > 4) return NBM_EINVAL;
  if (!nbm_aligned16(g)) return NBM_EALIGN;
  hipLaunchKernelGGL(zero_roi_windows_kernel, dim3(B * n_roi), dim3(256), 0, (hipStream_t)stream, g, H, W, C / 4, rois, level,
                     n_roi, lvl);
  return nbm_launch_status();
}
