// Grouped 3x3 convolution of the ResNeXt bottleneck (include/nbm_hip.h: nbm_gconv3x3) on the fp32 matrix instruction
// v_mfma_f32_16x16x4_f32.  DESIGN 4k.
//
// One workgroup = one tile of output pixels (TH rows x 16 columns of one image) x 64 consecutive channels; its four waves take 16 output
// channels each.  The input patch of the tile (halo included, zeros outside the image) is staged in LDS once, as 16 planes of four
// channels each; every tap of every output row is then ONE ds_read_b128 per lane, which is the x operand of four MFMAs:
//
//   MFMA operand A (16 x 4): the weights  w[n = lane & 15][k = lane >> 4]   -> D row    = output channel
//   MFMA operand B (4 x 16): the pixels   x[k = lane >> 4][m = lane & 15]   -> D column = output pixel (16 neighbours of one row)
//
// so a lane ends up with FOUR CONSECUTIVE CHANNELS of one pixel and stores them with one 16-byte store.  The k index of an instruction
// is free as long as both operands agree: lane group q = lane >> 4 reads channels 4q .. 4q+3 of a 16-channel slab with one 16-byte load
// and feeds element e to MFMA e, so instruction e sums over the channels {e, 4 + e, 8 + e, 12 + e}.
//
// Groups narrower than the instruction (Cg = 4, 8) are packed 4 / 2 to a slab with a block-diagonal weight fragment (3/4 and 1/2 of the
// issued products are structural zeros); Cg = 16 fills it; Cg = 32 / 64 sum over 2 / 4 slabs.  The weight fragments come from global
// memory in exactly the lane order (`gconv` in nets/_prep.py), 1 KiB per wave-instruction, one tap ahead of their use: a group's
// weights never have to fit LDS.
#include "nbm_common.h"

namespace {

constexpr int GC_TW = 16;            // output columns of a tile: the 16 pixels of one MFMA
constexpr int GC_CB = 64;            // channels of a workgroup: 4 waves x 16 output channels
constexpr int GC_QUADS = GC_CB / 4;  // LDS planes, four channels (16 bytes) per pixel each

template <int S>
struct gc_geom {
  static constexpr int TH = S == 1 ? 8 : 4;               // output rows of a tile
  static constexpr int PH = (TH - 1) * S + 3;             // patch rows    10 / 9
  static constexpr int PW = (GC_TW - 1) * S + 3;          // patch columns 18 / 33
  static constexpr int HALF = (PW + 1) / 2;               // S == 2: a patch row keeps its even columns first, then the odd ones
  // plane pitch in 16-byte slots: a multiple of 16, so that the two planes a 16-lane read group of ds_read_b128 touches (lanes m of
  // plane q, lanes m' of plane q + 1) fall on the banks their pixel index alone decides; + 7: plane Q starts Q >> 1 slots late, which
  // spreads the 8 planes that one ds_write_b128 lane group stores over 4 bank slots instead of 1
  static constexpr int PLANE = (PH * PW + 7 + 15) / 16 * 16;        // 192 / 304
  static constexpr int LDS_BYTES = GC_QUADS * PLANE * 16;           // 48 KiB (3 workgroups per CU) / 76 KiB (2 per CU)
};

struct gc_params {
  const float* x;
  const f32x4* w;
  float* y;
  const float* scale;
  const float* shift;
  int H, W, Ho, Wo, x_ld, y_ld, relu;
  unsigned tiles_x, tiles_per_image;
  nbm_fastdiv div_tx, div_tpi;
};

template <int S>
__device__ __forceinline__ int gc_pos(int px) {
  return S == 1 ? px : (px & 1) * gc_geom<S>::HALF + (px >> 1);
}

template <int S, int NSLAB>
__global__ __launch_bounds__(256, 2) void gconv3x3_kernel(const gc_params p) {
  using G = gc_geom<S>;
  __shared__ f32x4 patch[GC_QUADS * G::PLANE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned t = blockIdx.x;
  const unsigned b = nbm_fdiv(t, p.div_tpi);
  t -= b * p.tiles_per_image;
  const unsigned ty = nbm_fdiv(t, p.div_tx), tx = t - ty * p.tiles_x;
  const int c0 = blockIdx.y * GC_CB;

  // ---- the input patch: 16 consecutive threads read the 256 contiguous bytes of one pixel
  {
    const int iy0 = (int)ty * G::TH * S - 1, ix0 = (int)tx * GC_TW * S - 1;
    const float* xb = p.x + (size_t)b * p.H * p.W * p.x_ld + c0;
#pragma unroll 4
    for (int i = tid; i < G::PH * G::PW * GC_QUADS; i += 256) {
      const int Q = i & (GC_QUADS - 1), pix = i >> 4;
      const int py = pix / G::PW, px = pix - py * G::PW;
      const int iy = iy0 + py, ix = ix0 + px;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W)
        v = *reinterpret_cast<const f32x4*>(xb + ((size_t)iy * p.W + ix) * p.x_ld + 4 * Q);
      patch[Q * G::PLANE + (Q >> 1) + py * G::PW + gc_pos<S>(px)] = v;
    }
  }
  __syncthreads();

  // ---- 9 taps x NSLAB slabs x TH rows: one 16-byte LDS read -> four MFMAs
  const int m = lane & 15, q = lane >> 4;
  const int tile = blockIdx.y * 4 + wave;                       // 16 output channels
  const int slab0 = (wave / NSLAB) * NSLAB;                     // first 16-channel slab of this wave's group(s) within the 64
  const f32x4* wp = p.w + (size_t)tile * (9 * NSLAB * 64) + lane;
  f32x4 acc[G::TH];
#pragma unroll
  for (int i = 0; i < G::TH; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  // one step = one (tap, slab): TH LDS reads and 4 TH MFMAs; the next step's operands are fetched while this step's MFMAs run (a rolled
  // loop: fully unrolled, the compiler hoists every LDS read of the kernel and runs out of registers at 4 slabs)
  const int plane0 = (slab0 * 4 + q) * G::PLANE + ((slab0 * 4 + q) >> 1) + m;
  auto a_ptr = [&](int step) {
    const int tap = step / NSLAB, j = step % NSLAB;
    const int r = tap / 3, s = tap - 3 * r;
    return patch + plane0 + j * (4 * G::PLANE + 2) + r * G::PW + (S == 1 ? s : (s & 1) * G::HALF + (s >> 1));
  };
  f32x4 a_cur[G::TH], a_nxt[G::TH], w_cur = wp[0], w_nxt = w_cur;
  {
    const f32x4* pa = a_ptr(0);
#pragma unroll
    for (int i = 0; i < G::TH; ++i) a_cur[i] = pa[i * S * G::PW];
  }
#pragma unroll 1
  for (int step = 0; step < 9 * NSLAB; ++step) {
    if (step + 1 < 9 * NSLAB) {
      const f32x4* pa = a_ptr(step + 1);
      w_nxt = wp[(step + 1) * 64];
#pragma unroll
      for (int i = 0; i < G::TH; ++i) a_nxt[i] = pa[i * S * G::PW];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
#pragma unroll
      for (int i = 0; i < G::TH; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(w_cur[e], a_cur[i][e], acc[i], 0, 0, 0);
    }
    w_cur = w_nxt;
#pragma unroll
    for (int i = 0; i < G::TH; ++i) a_cur[i] = a_nxt[i];
  }

  // ---- epilogue: folded FrozenBatchNorm + ReLU, four channels of one pixel per lane
  const int ch = c0 + wave * 16 + 4 * q;
  f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
  if (p.scale) sc = *reinterpret_cast<const f32x4*>(p.scale + ch);
  if (p.shift) sh = *reinterpret_cast<const f32x4*>(p.shift + ch);
  const int ox = (int)tx * GC_TW + m;
  if (ox >= p.Wo) return;
#pragma unroll
  for (int i = 0; i < G::TH; ++i) {
    const int oy = (int)ty * G::TH + i;
    if (oy >= p.Ho) break;
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = fmaf(acc[i][e], sc[e], sh[e]);
      if (p.relu) v[e] = fmaxf(v[e], 0.f);
    }
    *reinterpret_cast<f32x4*>(p.y + (((size_t)b * p.Ho + oy) * p.Wo + ox) * p.y_ld + ch) = v;
  }
}

template <int S, int NSLAB>
int gc_launch(const gc_params& p, unsigned n_tiles, int chunks, hipStream_t st) {
  hipLaunchKernelGGL((gconv3x3_kernel<S, NSLAB>), dim3(n_tiles, chunks), dim3(256), 0, st, p);
  return nbm_launch_status();
}

}  // namespace

extern "C" int nbm_gconv3x3(const nbm_gconv_desc* d, void* stream) {
  if (!d || !d->x || !d->w || !d->y) return NBM_EINVAL;
  if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->groups <= 0 || d->Cg <= 0) return NBM_EINVAL;
  if (d->kh != 3 || d->kw != 3 || d->pad != 1 || (d->stride != 1 && d->stride != 2)) return NBM_EUNSUPPORTED;
  const int Cg = d->Cg;
  if (Cg != 4 && Cg != 8 && Cg != 16 && Cg != 32 && Cg != 64) return NBM_EUNSUPPORTED;
  const long long C = (long long)d->groups * Cg;
  if (C % GC_CB || C > (1 << 20)) return NBM_EUNSUPPORTED;      // a workgroup takes 64 consecutive channels (whole groups)
  if (d->x_ld < C || d->y_ld < C) return NBM_EINVAL;
  const int S = d->stride;
  if (d->Ho != (d->H - 1) / S + 1 || d->Wo != (d->W - 1) / S + 1) return NBM_EINVAL;
  // every access is a 16-byte one
  if (!nbm_aligned16(d->x) || !nbm_aligned16(d->w) || !nbm_aligned16(d->y) || (d->x_ld & 3) || (d->y_ld & 3) ||
      (d->scale && !nbm_aligned16(d->scale)) || (d->shift && !nbm_aligned16(d->shift)))
    return NBM_EUNSUPPORTED;
  const int TH = S == 1 ? gc_geom<1>::TH : gc_geom<2>::TH;
  const long long tiles_x = (d->Wo + GC_TW - 1) / GC_TW, tiles_y = (d->Ho + TH - 1) / TH;
  const long long n_tiles = tiles_x * tiles_y * d->B;
  if (n_tiles > 0x7fffffffLL) return NBM_EUNSUPPORTED;
  gc_params p;
  p.x = d->x;
  p.w = reinterpret_cast<const f32x4*>(d->w);
  p.y = d->y;
  p.scale = d->scale;
  p.shift = d->shift;
  p.H = d->H, p.W = d->W, p.Ho = d->Ho, p.Wo = d->Wo, p.x_ld = d->x_ld, p.y_ld = d->y_ld, p.relu = d->relu != 0;
  p.tiles_x = (unsigned)tiles_x;
  p.tiles_per_image = (unsigned)(tiles_x * tiles_y);
  p.div_tx = nbm_fastdiv_make(p.tiles_x);
  p.div_tpi = nbm_fastdiv_make(p.tiles_per_image);
  hipStream_t st = (hipStream_t)stream;
  const int chunks = (int)(C / GC_CB);
  const int nslab = Cg <= 16 ? 1 : Cg / 16;
  if (S == 1) {
    if (nslab == 1) return gc_launch<1, 1>(p, (unsigned)n_tiles, chunks, st);
    if (nslab == 2) return gc_launch<1, 2>(p, (unsigned)n_tiles, chunks, st);
    return gc_launch<1, 4>(p, (unsigned)n_tiles, chunks, st);
  }
  if (nslab == 1) return gc_launch<2, 1>(p, (unsigned)n_tiles, chunks, st);
  if (nslab == 2) return gc_launch<2, 2>(p, (unsigned)n_tiles, chunks, st);
  return gc_launch<2, 4>(p, (unsigned)n_tiles, chunks, st);
}
