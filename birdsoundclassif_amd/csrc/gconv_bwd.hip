// Gradients of the grouped 3x3 convolution of the ResNeXt bottleneck (include/nbm_hip.h: nbm_gconv3x3_dgrad, nbm_gconv3x3_wgrad,
// nbm_gconv3x3_wgrad_workspace) on the fp32 matrix instruction v_mfma_f32_16x16x4_f32.  DESIGN 4k.
//
// Both kernels stage dz = g * (y > 0) (the ReLU of the layer; y optional) in LDS, four channels of a pixel per 16-byte slot, 16 planes
// of four channels each -- the layout of csrc/gconv.hip.
//
// DATA GRADIENT.  With the weights transposed inside their group, rotated by 180 degrees and scaled (`gconv_dgrad` in nets/_prep.py,
// the fragment order of the forward kernel) the data gradient is the forward convolution of the zero-upsampled dz:
//   gx[iy][ix] = sum_{r', s'} dzup[iy - 1 + r'][ix - 1 + s'] W'[r'][s'],   dzup[S oy][S ox] = dz[oy][ox], 0 elsewhere.
// Stride 1: dzup = dz, the forward kernel's loop with a patch of dz.  Stride 2: a tap contributes only where iy - 1 + r' is even, so the
// four parity classes (iy & 1, ix & 1) of gx see 1 / 2 / 2 / 4 of the nine taps; a workgroup takes TH x 16 pixels of dz (+ one halo
// row and column) and produces the 2 TH x 32 pixels of gx above them, one accumulator per class: the 16 columns of one class read 16
// CONSECUTIVE columns of dz, so every tap is the forward's one ds_read_b128 -> four MFMAs, and no product with an upsampling zero is
// issued (nine tap-MFMAs per dz pixel, as the forward has per output pixel).
//
// WEIGHT GRADIENT.  dW[n][c][tap] = sum over pixels dz[pixel][n] x[pixel shifted by the tap][c]: the pixel is the K index.
//   MFMA operand A (16 x 4): dz[k = pixel lane >> 4][n = lane & 15]        -> D row    = output channel n
//   MFMA operand B (4 x 16): x [k = pixel lane >> 4][c = lane & 15]        -> D column = input channel c of a 16-channel slab
// A wave owns 16 output channels and keeps the 9 x NSLAB fragments of its group in registers while its workgroup walks a contiguous
// range of pixel tiles (TH rows x 16 columns of dz and the input patch under them); MFMA e of a row sums the pixels {4 e + q}.  The
// operands are scalar LDS reads (ds_read_b32: 32 banks, two 32-lane halves): a plane pitch of 2 (mod 8) slots puts the 32 lanes of a
// half -- 16 channels = 4 planes x 4 elements, 2 consecutive pixels -- on 32 different banks.  One dz read feeds 9 NSLAB MFMAs.
// The pixel tiles are SPLIT over blockIdx.x; every split stores its fragments to the workspace with plain stores, and a second kernel
// sums the splits in ascending order, applies scale[n], drops the block-diagonal zeros (Cg < 16) and is the only writer of dW: no
// atomics, the same bits every run.
#include "nbm_common.h"

namespace {

constexpr int GB_CB = 64;             // channels of a workgroup: 4 waves x 16 channels
constexpr int GB_QUADS = GB_CB / 4;   // LDS planes

// ------------------------------------------------------------------------------------------------ data gradient
template <int S>
struct gd_geom {
  static constexpr int TH = S == 1 ? 8 : 4;            // rows of dz per tile (stride 2: 2 TH rows of gx)
  static constexpr int NCLS = S == 1 ? 1 : 4;          // parity classes of gx
  static constexpr int OFF = S == 1 ? -1 : 0;          // patch origin relative to the tile's first dz pixel
  static constexpr int PH = S == 1 ? TH + 2 : TH + 1;
  static constexpr int PW = S == 1 ? 18 : 17;
  static constexpr int PLANE = (PH * PW + 7 + 15) / 16 * 16;   // csrc/gconv.hip: pitch a multiple of 16 slots, plane Q starts Q >> 1 late
};

struct gd_params {
  const float* g;
  const float* y;
  const f32x4* w;
  float* out;
  int H, W, Ho, Wo, g_ld, y_ld, out_ld;
  unsigned tiles_x, tiles_per_image;
  nbm_fastdiv div_tx, div_tpi;
};

// dz of four channels of one pixel
__device__ __forceinline__ f32x4 gb_load_dz(const float* g, const float* y, size_t pix, int g_ld, int y_ld, int ch) {
  f32x4 v = *reinterpret_cast<const f32x4*>(g + pix * g_ld + ch);
  if (y) {
    const f32x4 m = *reinterpret_cast<const f32x4*>(y + pix * y_ld + ch);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = m[e] > 0.f ? v[e] : 0.f;
  }
  return v;
}

template <int S, int NSLAB>
__global__ __launch_bounds__(256, 2) void gconv3x3_dgrad_kernel(const gd_params p) {
  using G = gd_geom<S>;
  __shared__ f32x4 patch[GB_QUADS * G::PLANE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned t = blockIdx.x;
  const unsigned b = nbm_fdiv(t, p.div_tpi);
  t -= b * p.tiles_per_image;
  const unsigned ty = nbm_fdiv(t, p.div_tx), tx = t - ty * p.tiles_x;
  const int c0 = blockIdx.y * GB_CB;
  const int oy0 = (int)ty * G::TH, ox0 = (int)tx * 16;

  // ---- the patch of dz (zeros outside the map): 16 consecutive threads read the 256 contiguous bytes of one pixel
  for (int i = tid; i < G::PH * G::PW * GB_QUADS; i += 256) {
    const int Q = i & (GB_QUADS - 1), pix = i >> 4;
    const int py = pix / G::PW, px = pix - py * G::PW;
    const int oy = oy0 + G::OFF + py, ox = ox0 + G::OFF + px;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if ((unsigned)oy < (unsigned)p.Ho && (unsigned)ox < (unsigned)p.Wo)
      v = gb_load_dz(p.g, p.y, ((size_t)b * p.Ho + oy) * p.Wo + ox, p.g_ld, p.y_ld, c0 + 4 * Q);
    patch[Q * G::PLANE + (Q >> 1) + py * G::PW + px] = v;
  }
  __syncthreads();

  const int m = lane & 15, q = lane >> 4;
  const int tile = blockIdx.y * 4 + wave;                      // 16 channels of gx
  const int slab0 = (wave / NSLAB) * NSLAB;
  const f32x4* wp = p.w + (size_t)tile * (9 * NSLAB * 64) + lane;
  const f32x4* pa0 = patch + (slab0 * 4 + q) * G::PLANE + ((slab0 * 4 + q) >> 1) + m;
  f32x4 acc[G::NCLS][G::TH];
#pragma unroll
  for (int c = 0; c < G::NCLS; ++c)
#pragma unroll
    for (int i = 0; i < G::TH; ++i) acc[c][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  // the taps are unrolled (each has its own class = its own accumulators), the slabs of a tap are not
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int r = tap / 3, s = tap - 3 * r;
    const int cls = S == 1 ? 0 : (r != 1) * 2 + (s != 1);
    const int dy = S == 1 ? r : (r == 2), dx = S == 1 ? s : (s == 2);
#pragma unroll 1
    for (int j = 0; j < NSLAB; ++j) {
      const f32x4 w = wp[(tap * NSLAB + j) * 64];
      const f32x4* pa = pa0 + j * (4 * G::PLANE + 2) + dy * G::PW + dx;
      f32x4 a[G::TH];
#pragma unroll
      for (int i = 0; i < G::TH; ++i) a[i] = pa[i * G::PW];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int i = 0; i < G::TH; ++i) acc[cls][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[e], a[i][e], acc[cls][i], 0, 0, 0);
      }
    }
  }

  // ---- four channels of one pixel per lane and accumulator
  const int ch = c0 + wave * 16 + 4 * q;
#pragma unroll
  for (int c = 0; c < G::NCLS; ++c) {
    const int ix = S == 1 ? ox0 + m : 2 * (ox0 + m) + (c & 1);
    if (ix >= p.W) continue;
#pragma unroll
    for (int i = 0; i < G::TH; ++i) {
      const int iy = S == 1 ? oy0 + i : 2 * (oy0 + i) + (c >> 1);
      if (iy >= p.H) continue;
      *reinterpret_cast<f32x4*>(p.out + (((size_t)b * p.H + iy) * p.W + ix) * p.out_ld + ch) = acc[c][i];
    }
  }
}

template <int S, int NSLAB>
int gd_launch(const gd_params& p, unsigned n_tiles, int chunks, hipStream_t st) {
  hipLaunchKernelGGL((gconv3x3_dgrad_kernel<S, NSLAB>), dim3(n_tiles, chunks), dim3(256), 0, st, p);
  return nbm_launch_status();
}

// ------------------------------------------------------------------------------------------------ weight gradient
constexpr int gw_pitch(int slots) { return (slots - 2 + 7) / 8 * 8 + 2; }   // the next pitch that is 2 (mod 8)

template <int S>
struct gw_geom {
  static constexpr int TH = S == 1 ? 4 : 2;              // rows of dz per tile
  static constexpr int PH = (TH - 1) * S + 3;            // input patch rows    6 / 5
  static constexpr int PW = 15 * S + 3;                  // input patch columns 18 / 33
  static constexpr int HALF = (PW + 1) / 2;              // S == 2: a patch row keeps its even columns first, then the odd ones
  static constexpr int PLX = gw_pitch(PH * PW);          // 114 / 170 slots
  static constexpr int PLG = gw_pitch(TH * 16);          // 66 / 34 slots
  static constexpr int LDS_BYTES = GB_QUADS * (PLX + PLG) * 16;   // 45 KiB / 51 KiB
};

struct gw_params {
  const float* g;
  const float* y;
  const float* x;
  f32x4* ws;
  int H, W, Ho, Wo, g_ld, y_ld, x_ld;
  unsigned tiles_x, tiles_per_image, n_tiles;
  nbm_fastdiv div_tx, div_tpi;
};

template <int S, int NSLAB>
__global__ __launch_bounds__(256, 2) void gconv3x3_wgrad_kernel(const gw_params p) {
  using G = gw_geom<S>;
  __shared__ f32x4 xs[GB_QUADS * G::PLX];
  __shared__ f32x4 gs[GB_QUADS * G::PLG];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c0 = blockIdx.y * GB_CB;
  const unsigned t_begin = (unsigned)((unsigned long long)blockIdx.x * p.n_tiles / gridDim.x);
  const unsigned t_end = (unsigned)((unsigned long long)(blockIdx.x + 1) * p.n_tiles / gridDim.x);

  const int cl = lane & 15, q = lane >> 4;
  const int slab0 = (wave / NSLAB) * NSLAB;
  // scalar views: float index = 4 * slot + element
  const float* a_base = reinterpret_cast<const float*>(gs) + ((wave * 4 + (cl >> 2)) * G::PLG + q) * 4 + (cl & 3);
  const float* b_base = reinterpret_cast<const float*>(xs) + ((slab0 * 4 + (cl >> 2)) * G::PLX + q) * 4 + (cl & 3);
  f32x4 acc[NSLAB][9];
#pragma unroll
  for (int j = 0; j < NSLAB; ++j)
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) acc[j][tap] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (unsigned tt = t_begin; tt < t_end; ++tt) {
    unsigned t = tt;
    const unsigned b = nbm_fdiv(t, p.div_tpi);
    t -= b * p.tiles_per_image;
    const unsigned ty = nbm_fdiv(t, p.div_tx), tx = t - ty * p.tiles_x;
    const int oy0 = (int)ty * G::TH, ox0 = (int)tx * 16;
    if (tt != t_begin) __syncthreads();                  // every wave is done with the previous tile
    {
      const int iy0 = oy0 * S - 1, ix0 = ox0 * S - 1;
      const float* xb = p.x + (size_t)b * p.H * p.W * p.x_ld + c0;
      for (int i = tid; i < G::PH * G::PW * GB_QUADS; i += 256) {
        const int Q = i & (GB_QUADS - 1), pix = i >> 4;
        const int py = pix / G::PW, px = pix - py * G::PW;
        const int iy = iy0 + py, ix = ix0 + px;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W)
          v = *reinterpret_cast<const f32x4*>(xb + ((size_t)iy * p.W + ix) * p.x_ld + 4 * Q);
        xs[Q * G::PLX + py * G::PW + (S == 1 ? px : (px & 1) * G::HALF + (px >> 1))] = v;
      }
      for (int i = tid; i < G::TH * 16 * GB_QUADS; i += 256) {
        const int Q = i & (GB_QUADS - 1), pix = i >> 4;
        const int oy = oy0 + (pix >> 4), ox = ox0 + (pix & 15);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (oy < p.Ho && ox < p.Wo) v = gb_load_dz(p.g, p.y, ((size_t)b * p.Ho + oy) * p.Wo + ox, p.g_ld, p.y_ld, c0 + 4 * Q);
        gs[Q * G::PLG + pix] = v;
      }
    }
    __syncthreads();
#pragma unroll 1
    for (int row = 0; row < G::TH; ++row) {
      const float* pa = a_base + row * 16 * 4;
      const float* pb = b_base + row * S * G::PW * 4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float a = pa[4 * e * 4];                   // dz of pixel 4 e + q of the row
#pragma unroll
        for (int j = 0; j < NSLAB; ++j) {
#pragma unroll
          for (int tap = 0; tap < 9; ++tap) {
            const int r = tap / 3, s = tap - 3 * r;
            const int pos = r * G::PW + 4 * e + (S == 1 ? s : (s & 1) * G::HALF + (s >> 1));
            acc[j][tap] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, pb[(j * 4 * G::PLX + pos) * 4], acc[j][tap], 0, 0, 0);
          }
        }
      }
    }
  }

  // ---- this split's fragments: [split][C / 16][9][NSLAB][64 lanes] x 16 bytes; a split without tiles stores zeros
  f32x4* o = p.ws + (((size_t)blockIdx.x * gridDim.y * 4 + blockIdx.y * 4 + wave) * 9 * NSLAB) * 64 + lane;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap)
#pragma unroll
    for (int j = 0; j < NSLAB; ++j) o[(tap * NSLAB + j) * 64] = acc[j][tap];
}

// dW[n][c][tap] (+)= scale[n] * sum over the splits, in ascending order.  Fragment element: lane = 16 (n % 16 / 4) + column, e = n % 4.
__global__ __launch_bounds__(256) void gconv3x3_wgrad_reduce_kernel(const float* __restrict__ ws, const float* __restrict__ scale,
                                                                    float* __restrict__ out, int C, int Cg, int splits,
                                                                    int accumulate) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)C * Cg * 9) return;
  const int n = (int)(idx / (9 * Cg)), rem = (int)(idx - (long long)n * 9 * Cg);
  const int c = rem / 9, tap = rem - 9 * c;
  const int nslab = Cg <= 16 ? 1 : Cg / 16;
  const int t = n >> 4, nl = n & 15;
  const int j = Cg <= 16 ? 0 : c >> 4;
  const int col = Cg <= 16 ? (nl / Cg) * Cg + c : c & 15;   // Cg < 16: the group's block on the diagonal of the 16 x 16 fragment
  const size_t frag = (size_t)9 * nslab * 256, per_split = (size_t)(C / 16) * frag;
  const float* src = ws + (size_t)t * frag + (size_t)(tap * nslab + j) * 256 + ((nl >> 2) * 16 + col) * 4 + (nl & 3);
  float sum = 0.f;
  for (int s = 0; s < splits; ++s) sum += src[(size_t)s * per_split];
  if (scale) sum *= scale[n];
  out[idx] = accumulate ? out[idx] + sum : sum;
}

template <int S, int NSLAB>
int gw_launch(const gw_params& p, int splits, int chunks, hipStream_t st) {
  hipLaunchKernelGGL((gconv3x3_wgrad_kernel<S, NSLAB>), dim3(splits, chunks), dim3(256), 0, st, p);
  return nbm_launch_status();
}

// ------------------------------------------------------------------------------------------------ host
constexpr int GW_MAX_SPLITS = 4096;
constexpr int GW_TARGET_WORKGROUPS = 512;                // two per CU

// the geometry all three entry points accept; C = groups * Cg
int gb_check_geometry(const nbm_gconv_bwd_desc* d) {
  if (!d) return NBM_EINVAL;
  if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->groups <= 0 || d->Cg <= 0) return NBM_EINVAL;
  if (d->kh != 3 || d->kw != 3 || d->pad != 1 || (d->stride != 1 && d->stride != 2)) return NBM_EUNSUPPORTED;
  const int Cg = d->Cg;
  if (Cg != 4 && Cg != 8 && Cg != 16 && Cg != 32 && Cg != 64) return NBM_EUNSUPPORTED;
  const long long C = (long long)d->groups * Cg;
  if (C % GB_CB || C > (1 << 20)) return NBM_EUNSUPPORTED;
  if (d->Ho != (d->H - 1) / d->stride + 1 || d->Wo != (d->W - 1) / d->stride + 1) return NBM_EINVAL;
  return NBM_OK;
}

long long gw_tiles(const nbm_gconv_bwd_desc* d, long long* tiles_x, long long* tiles_y) {
  const int TH = d->stride == 1 ? gw_geom<1>::TH : gw_geom<2>::TH;
  *tiles_x = (d->Wo + 15) / 16, *tiles_y = (d->Ho + TH - 1) / TH;
  return *tiles_x * *tiles_y * d->B;
}

long long gw_split_floats(const nbm_gconv_bwd_desc* d) {   // one split's fragments
  return (long long)d->groups * d->Cg * 9 * (d->Cg < 16 ? 16 : d->Cg);
}

// d->splits > 0: taken as it is (up to GW_MAX_SPLITS).  0: enough splits for two workgroups per CU, but no more than there are pixel
// tiles and no more than keep the workspace within the size of the two operands the launch reads (x counted with the pixels of g, which
// it has at least: the choice then depends on the gradient map alone)
int gw_splits(const nbm_gconv_bwd_desc* d) {
  if (d->splits > 0) return d->splits;
  long long tx, ty;
  const long long n_tiles = gw_tiles(d, &tx, &ty);
  const long long chunks = (long long)d->groups * d->Cg / GB_CB;
  const long long operands = 2LL * d->B * d->Ho * d->Wo * d->groups * d->Cg;
  long long s = (GW_TARGET_WORKGROUPS + chunks - 1) / chunks;
  if (s > n_tiles) s = n_tiles;
  if (s > operands / gw_split_floats(d)) s = operands / gw_split_floats(d);
  if (s > GW_MAX_SPLITS) s = GW_MAX_SPLITS;
  return s < 1 ? 1 : (int)s;
}

}  // namespace

extern "C" int nbm_gconv3x3_dgrad(const nbm_gconv_bwd_desc* d, void* stream) {
  const int rc = gb_check_geometry(d);
  if (rc != NBM_OK) return rc;
  if (!d->g || !d->w || !d->out) return NBM_EINVAL;
  const long long C = (long long)d->groups * d->Cg;
  if (d->g_ld < C || d->out_ld < C || (d->y && d->y_ld < C)) return NBM_EINVAL;
  // every access is a 16-byte one
  if (!nbm_aligned16(d->g) || !nbm_aligned16(d->w) || !nbm_aligned16(d->out) || (d->g_ld & 3) || (d->out_ld & 3) ||
      (d->y && (!nbm_aligned16(d->y) || (d->y_ld & 3))))
    return NBM_EUNSUPPORTED;
  const int S = d->stride;
  const int TH = S == 1 ? gd_geom<1>::TH : gd_geom<2>::TH;
  const long long tiles_x = (d->Wo + 15) / 16, tiles_y = (d->Ho + TH - 1) / TH;
  const long long n_tiles = tiles_x * tiles_y * d->B;
  if (n_tiles > 0x7fffffffLL) return NBM_EUNSUPPORTED;
  gd_params p;
  p.g = d->g, p.y = d->y, p.w = reinterpret_cast<const f32x4*>(d->w), p.out = d->out;
  p.H = d->H, p.W = d->W, p.Ho = d->Ho, p.Wo = d->Wo, p.g_ld = d->g_ld, p.y_ld = d->y_ld, p.out_ld = d->out_ld;
  p.tiles_x = (unsigned)tiles_x;
  p.tiles_per_image = (unsigned)(tiles_x * tiles_y);
  p.div_tx = nbm_fastdiv_make(p.tiles_x);
  p.div_tpi = nbm_fastdiv_make(p.tiles_per_image);
  hipStream_t st = (hipStream_t)stream;
  const int chunks = (int)(C / GB_CB);
  const int nslab = d->Cg <= 16 ? 1 : d->Cg / 16;
  if (S == 1) {
    if (nslab == 1) return gd_launch<1, 1>(p, (unsigned)n_tiles, chunks, st);
    if (nslab == 2) return gd_launch<1, 2>(p, (unsigned)n_tiles, chunks, st);
    return gd_launch<1, 4>(p, (unsigned)n_tiles, chunks, st);
  }
  if (nslab == 1) return gd_launch<2, 1>(p, (unsigned)n_tiles, chunks, st);
  if (nslab == 2) return gd_launch<2, 2>(p, (unsigned)n_tiles, chunks, st);
  return gd_launch<2, 4>(p, (unsigned)n_tiles, chunks, st);
}

extern "C" int nbm_gconv3x3_wgrad_workspace(const nbm_gconv_bwd_desc* d, long long* bytes) {
  if (!bytes) return NBM_EINVAL;
  const int rc = gb_check_geometry(d);
  if (rc != NBM_OK) return rc;
  if (d->splits < 0 || d->splits > GW_MAX_SPLITS) return NBM_EINVAL;
  *bytes = (long long)gw_splits(d) * gw_split_floats(d) * 4;
  return NBM_OK;
}

extern "C" int nbm_gconv3x3_wgrad(const nbm_gconv_bwd_desc* d, void* stream) {
  long long need = 0;
  const int rc = nbm_gconv3x3_wgrad_workspace(d, &need);
  if (rc != NBM_OK) return rc;
  if (!d->g || !d->x || !d->out || !d->workspace || d->workspace_bytes < need) return NBM_EINVAL;
  const long long C = (long long)d->groups * d->Cg;
  if (d->g_ld < C || d->x_ld < C || (d->y && d->y_ld < C)) return NBM_EINVAL;
  if (!nbm_aligned16(d->g) || !nbm_aligned16(d->x) || !nbm_aligned16(d->workspace) || (d->g_ld & 3) || (d->x_ld & 3) ||
      (d->y && (!nbm_aligned16(d->y) || (d->y_ld & 3))))
    return NBM_EUNSUPPORTED;
  long long tiles_x, tiles_y;
  const long long n_tiles = gw_tiles(d, &tiles_x, &tiles_y);
  if (n_tiles > 0x7fffffffLL) return NBM_EUNSUPPORTED;
  const int splits = gw_splits(d);
  gw_params p;
  p.g = d->g, p.y = d->y, p.x = d->x, p.ws = reinterpret_cast<f32x4*>(d->workspace);
  p.H = d->H, p.W = d->W, p.Ho = d->Ho, p.Wo = d->Wo, p.g_ld = d->g_ld, p.y_ld = d->y_ld, p.x_ld = d->x_ld;
  p.tiles_x = (unsigned)tiles_x;
  p.tiles_per_image = (unsigned)(tiles_x * tiles_y);
  p.n_tiles = (unsigned)n_tiles;
  p.div_tx = nbm_fastdiv_make(p.tiles_x);
  p.div_tpi = nbm_fastdiv_make(p.tiles_per_image);
  hipStream_t st = (hipStream_t)stream;
  const int chunks = (int)(C / GB_CB);
  const int nslab = d->Cg <= 16 ? 1 : d->Cg / 16;
  const int S = d->stride;
  int lrc;
  if (S == 1)
    lrc = nslab == 1 ? gw_launch<1, 1>(p, splits, chunks, st) : nslab == 2 ? gw_launch<1, 2>(p, splits, chunks, st)
                                                                           : gw_launch<1, 4>(p, splits, chunks, st);
  else
    lrc = nslab == 1 ? gw_launch<2, 1>(p, splits, chunks, st) : nslab == 2 ? gw_launch<2, 2>(p, splits, chunks, st)
                                                                           : gw_launch<2, 4>(p, splits, chunks, st);
  if (lrc != NBM_OK) return lrc;
  const long long n_out = C * d->Cg * 9;
  hipLaunchKernelGGL(gconv3x3_wgrad_reduce_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, st,
                     reinterpret_cast<const float*>(d->workspace), d->scale, d->out, (int)C, d->Cg, splits, d->accumulate != 0);
  return nbm_launch_status();
}
