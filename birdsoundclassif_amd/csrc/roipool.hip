// RoI pooling at any pool size (--roi_pool_h / --roi_pool_w): nbm_roi_pool_hw / nbm_roi_pool_hw_bwd (include/nbm_hip.h).
// The 2 x 2 default keeps its own kernels (detect.hip: roi_pool_kernel, pointwise_bwd.hip: roi_pool_bwd_kernel); these read and
// write dense FPN maps only.  With pool_h = pool_w = 2 every operation below is the one roi_pool_kernel performs, in its order,
// so the outputs are its bits.
#include "nbm_common.h"

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

// Pyramid level of a RoI, layers.py:408-417 (sizes WITHOUT the +1): roi_window of detect.hip.
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
__device__ __forceinline__ bool roi_window_hw(const float* roi, int lvl, int H, int W, int ph, int pw, int& x1, int& y1, int& x2,
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
  const bool inside = roi_window_hw(roi, lvl, H, W, ph, pw, x1, y1, x2, y2);
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
  if (!roi_window_hw(roi, lvl, H, W, ph, pw, x1, y1, x2, y2)) return;
  const int C = p.C, nbin = ph * pw;
  float* gf = p.gfmap[lvl] + ((long long)b * H + y1) * W * C + (long long)x1 * C;
  const float* g = p.gpool + (long long)slot * nbin * C;
  const int h = y2 - y1 + 1, w = min(x2, W - 1) - x1 + 1;
  // work items are (bin, channel): neighbouring lanes add to neighbouring floats, as in roi_pool_bwd_kernel (a lane per channel
  // quad spreads each atomic instruction over four times the cache lines: 4.2 x slower at 2 x 2, measured)
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

extern "C" int nbm_roi_pool_hw_bwd(float* const* gfmap, const int* fh, const int* fw, int n_levels, int C, const float* rois,
                                   const int* level, int B, int n_roi, int pool_h, int pool_w, const float* gpool,
                                   void* stream) {
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
  hipLaunchKernelGGL(roi_pool_hw_bwd_kernel, dim3(B * n_roi), dim3(256), 0, (hipStream_t)stream, p);
  return nbm_launch_status();
}
