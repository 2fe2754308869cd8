// Device-side pieces shared by the implicit-GEMM kernels (igemm.hip, igemm_h16.hip, igemm_split.hip, igemm_split_tn.hip, igemm_bwd.hip)
// and wino_fused.hip: the workgroup -> tile map, the buffer resource, the A-row decode of the fast gather and the forward epilogue.
// The forward kernels give the same bits as each other BECAUSE they finish a tile through the functions below: an epilogue operand is
// added here, once, and the compiler reports every kernel it reaches.
#pragma once
#include "nbm_common.h"      // f32x4 / f32x16, nbm_fdiv, NBM_ACT_* (nbm_hip.h)
#include "igemm_params.h"

namespace {

enum { EPI_STD = 0 };      // igemm_kernel's reserved EPI parameter (the only epilogue there is; part of the instantiation names)

// XCD-aware tile id (bijective for any grid size): consecutive tile ids, e.g. the N tiles of one M tile, run on the same XCD / L2
__device__ __forceinline__ int xcd_tile(int nwg, int bid) {
  const int q8 = nwg >> 3, r8 = nwg & 7, xcd = bid & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
}

// raw buffer resource (stride 0): base = block-uniform pointer, a per-lane offset >= bytes reads zeros
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const float* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, bytes, 0x00020000);
}

// ---- fast gather: rows as 32-bit byte offsets relative to a block-uniform base, and one bit per filter tap that lands inside the image
// -- the K loop then needs one add and one bit test per row instead of re-deriving coordinates (the address / validity VALU work sat in
// front of every MFMA burst: 15 % of the kernel).
// base of the tile whose first GEMM row is bm0: the first tap of that row's pixel
__device__ __forceinline__ long long gather_base(const nbm_igemm::IgemmParams& p, int bm0) {
  const int m0 = bm0 < p.M ? bm0 : 0;
  const int b = (int)nbm_fdiv((unsigned)m0, p.fd_howo), rem = m0 - b * p.HoWo;
  const int oy = (int)nbm_fdiv((unsigned)rem, p.fd_wo), ox = rem - oy * p.Wo;
  return ((long long)(b * p.H + oy * p.stride - p.pad) * p.W + (ox * p.stride - p.pad)) * p.x_ld;
}
// rows and columns of the filter that land inside the image, then their product -- selects only: as a kh x kw nest of data-dependent
// branches this loop was the longest part of the tile prologue (cycle counters of the data-gradient twin, round 5)
__device__ __forceinline__ unsigned long long tap_mask(const nbm_igemm::IgemmParams& p, int iy0, int ix0) {
  unsigned rowm = 0u, colm = 0u;
  unsigned long long mk = 0ull;
  for (int r = 0; r < p.kh; ++r) rowm |= ((unsigned)(iy0 + r) < (unsigned)p.H ? 1u : 0u) << r;
  for (int s2 = 0; s2 < p.kw; ++s2) colm |= ((unsigned)(ix0 + s2) < (unsigned)p.W ? 1u : 0u) << s2;
  for (int r = 0; r < p.kh; ++r) mk |= ((rowm >> r) & 1u) ? (unsigned long long)colm << (r * p.kw) : 0ull;
  return mk;
}
struct GatherRow { unsigned rel; unsigned long long taps; };
// GEMM row m = output pixel m (ok: m < M): byte offset of float `koff` of its first tap relative to blk_base, and its tap mask
__device__ __forceinline__ GatherRow gather_row(const nbm_igemm::IgemmParams& p, int m, bool ok, long long blk_base, int koff) {
  const int mm = ok ? m : 0;
  // (pixel indices fit 31 bits: M is an int; a 64-bit division here was ~150 instructions per row)
  const int b = (int)nbm_fdiv((unsigned)mm, p.fd_howo), rem = mm - b * p.HoWo;
  const int oy = (int)nbm_fdiv((unsigned)rem, p.fd_wo), ox = rem - oy * p.Wo;
  const int iy0 = oy * p.stride - p.pad, ix0 = ox * p.stride - p.pad;
  const long long base = ((long long)(b * p.H + iy0) * p.W + ix0) * p.x_ld;
  const unsigned long long mk = tap_mask(p, iy0, ix0);      // (unconditionally: a select, no branch around the loops)
  return {((unsigned)(base - blk_base) + koff) * 4u,        // bytes; rows ascend with m: never negative
          ok ? mk : 0ull};
}

// ---- the finish of an output value.  These are the only places where it is written.
__device__ __forceinline__ float epi_act(float v, int act) {
  if (act == NBM_ACT_RELU) return fmaxf(v, 0.0f);
  if (act == NBM_ACT_SILU) return v / (1.0f + expf(-v));
  if (act == NBM_ACT_LEAKY) return v > 0.f ? v : 0.01f * v;
  return v;
}
__device__ __forceinline__ f32x4 epi_act4(f32x4 v, int act) {      // (the branch on the uniform `act` outside the element loops)
  if (act == NBM_ACT_RELU) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = epi_act(v[e], NBM_ACT_RELU);
  } else if (act == NBM_ACT_SILU) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = epi_act(v[e], NBM_ACT_SILU);
  } else if (act == NBM_ACT_LEAKY) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = epi_act(v[e], NBM_ACT_LEAKY);
  }
  return v;
}
// the one expression whose association and contraction decide the bits (rs: the per-row shift, 0.f without one -- it IS added)
__device__ __forceinline__ f32x4 epi_affine4(f32x4 v, float alpha, f32x4 sc, f32x4 sh, float rs) {
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = (v[e] * alpha) * sc[e] + sh[e] + rs;
  return v;
}
// (value > 0) of a lane's four channels as its row's 32-channel word.  The 8 consecutive lanes grp8 .. grp8 + 7 of the wave hold the row's
// 32 channels and read their byte of the four wave-wide comparison masks: bit 8 e + q of the word <-> channel 4 q + e of the 32
// (nbm_hip.h) -- no cross-lane traffic
__device__ __forceinline__ unsigned epi_relu_bits(f32x4 v, int grp8) {
  return ((unsigned)(__builtin_amdgcn_ballot_w64(v[0] > 0.f) >> grp8) & 0xffu) |
         (((unsigned)(__builtin_amdgcn_ballot_w64(v[1] > 0.f) >> grp8) & 0xffu) << 8) |
         (((unsigned)(__builtin_amdgcn_ballot_w64(v[2] > 0.f) >> grp8) & 0xffu) << 16) |
         (((unsigned)(__builtin_amdgcn_ballot_w64(v[3] > 0.f) >> grp8) & 0xffu) << 24);
}

// ---- epilogue of the forward kernels: the BM x BN accumulator tile of a workgroup of 4 waves (WM x WN per wave) -> y.
// C/D layout: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  lds: the kernel's operand buffers (LDS_FLOATS floats), free
// after the barrier behind the K loop.  STAGES == 1 (or a 256-row tile): the tile goes out WM rows at a time.  ROWS: GEMM row m is pixel
// row_pixel(m) (or none: < 0) of the dense maps; every other form passes no row_pixel.
template <int BM, int BN, int WM, int WN, int STAGES, bool ROWS, int LDS_FLOATS, class RowPixel = int>
__device__ __forceinline__ void igemm_store_tile(const nbm_igemm::IgemmParams& p, int g, float* lds, f32x16 (&acc)[WM / 32][WN / 32],
                                                 int bm0, int bn0, int wm0, int wn0, int lrow, int lh, int tid,
                                                 RowPixel row_pixel = RowPixel()) {
  constexpr int MT = WM / 32, NT = WN / 32;
  float* __restrict__ yg = p.y + (long long)g * p.y_gs;
  const float* __restrict__ rg = p.residual ? p.residual + (long long)g * p.res_gs : nullptr;
  if (p.vec_epi) {
    // Stage the accumulator tile through LDS so that every lane finishes 4 consecutive channels: 16-byte residual / scale / shift loads
    // and 16-byte stores instead of 64 dword stores per lane (store-issue bound on the short-K 1x1 layers).
    constexpr int CP = BN + 4;
    constexpr int HALVES = (STAGES == 1 || BM > 128) ? BM / WM : 1;   // single-stage LDS (or a 256-row tile) holds WM rows of the tile at a time
    constexpr int HROWS = BM / HALVES;
    static_assert(HROWS * CP <= LDS_FLOATS, "epilogue tile must fit the operand buffers");
    float* Cs = lds;
    constexpr int CH = BN / 4;                 // 16-byte chunks per tile row
    constexpr int RPP = 256 / CH;              // rows per pass
    const int cc = tid % CH, rr = tid / CH;
    const int n = bn0 + cc * 4;
    f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
    if (n < p.N) {
      if (p.scale) sc = *reinterpret_cast<const f32x4*>(p.scale + n);
      if (p.shift && !p.shift_per_row) sh = *reinterpret_cast<const f32x4*>(p.shift + n);
    }
    constexpr int NR = (HROWS + RPP - 1) / RPP;      // tile rows a thread finishes
#pragma unroll
    for (int half = 0; half < HALVES; ++half) {
      if (half) __syncthreads();
      // the residual values of this thread's rows are requested before the accumulators go through LDS: loaded inside the row loop
      // (behind its `m >= M` exit) they were NR dependent round trips at the end of every tile
      f32x4 rq[NR];
      const bool pre = !ROWS && rg && n < p.N;
      if (pre) {
#pragma unroll
        for (int k = 0; k < NR; ++k) {
          long long m = bm0 + half * HROWS + rr + k * RPP;
          m = m < p.M ? m : p.M - 1;
          rq[k] = *reinterpret_cast<const f32x4*>(rg + m * p.res_ld + n);
        }
      }
      if (HALVES == 1 || wm0 == half * HROWS) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e)
              Cs[((HALVES == 1 ? wm0 : 0) + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh) * CP + wn0 + j * 32 + lrow] = acc[i][j][e];
      }
      // fused top-down merge: the interpolation set-up of a tile ROW (source pixels, weights) is the same for all its channel chunks -- one
      // thread per row computes it once into LDS (round 5: in the row loop it was ~45 vector instructions per row and thread, repeated by the
      // BN / 4 threads of the row, issued between the other workgroups' MFMAs); same expressions, same values
      static_assert(HROWS * CP + 8 * HROWS <= LDS_FLOATS, "epilogue tile + merge table must fit the operand buffers");
      int* const Ut = reinterpret_cast<int*>(lds + HROWS * CP);          // [HROWS][8]: p00, p01, p10, p11, ly, lx, hy, hx
      if constexpr (!ROWS) {
        if (p.up && tid < HROWS) {
#pragma clang fp contract(off)   // like torch's CPU upsample_bilinear2d: no fused multiply-adds in the coordinates or the blend
          long long m = bm0 + half * HROWS + tid;
          m = m < p.M ? m : p.M - 1;
          const int b = (int)nbm_fdiv((unsigned)m, p.fd_howo), rem = (int)(m - (long long)b * p.HoWo);
          const int oy = (int)nbm_fdiv((unsigned)rem, p.fd_wo), ox = rem - oy * p.Wo;
          const float fy = p.up_sh * oy, fx = p.up_sw * ox;
          const int y0 = (int)fy, x0 = (int)fx;
          const int y1 = y0 + (y0 < p.up_H - 1 ? 1 : 0), x1 = x0 + (x0 < p.up_W - 1 ? 1 : 0);
          const float ly = fminf(fmaxf(fy - y0, 0.f), 1.f), lx = fminf(fmaxf(fx - x0, 0.f), 1.f);
          const float hy = 1.f - ly, hx = 1.f - lx;
          const int rb = b * p.up_H;
          int* u = Ut + 8 * tid;
          u[0] = (rb + y0) * p.up_W + x0; u[1] = (rb + y0) * p.up_W + x1; u[2] = (rb + y1) * p.up_W + x0; u[3] = (rb + y1) * p.up_W + x1;
          u[4] = __float_as_int(ly); u[5] = __float_as_int(lx); u[6] = __float_as_int(hy); u[7] = __float_as_int(hx);
        }
      }
      __syncthreads();
      if (n < p.N) {
#pragma unroll
        for (int k = 0; k < NR; ++k) {
          const int r = rr + k * RPP;
          if (r >= HROWS) break;
          long long m = bm0 + half * HROWS + r;
          if (m >= p.M) break;
          if constexpr (ROWS) {
            m = row_pixel((int)m);
            if (m < 0) continue;
          }
          const float rs = (p.shift_per_row && p.shift) ? p.shift[m] : 0.f;
          f32x4 v = epi_affine4(*reinterpret_cast<const f32x4*>(Cs + r * CP + cc * 4), p.alpha, sc, sh, rs);
          if (rg) {
            const f32x4 q = pre ? rq[k] : *reinterpret_cast<const f32x4*>(rg + (long long)m * p.res_ld + n);
            v[0] += q[0]; v[1] += q[1]; v[2] += q[2]; v[3] += q[3];
          }
          // (NEGATIVE: the rows in groups of 2 / 4 with the four gathered vectors of a whole group requested first -- 4: spills at the
          // 256-register cap; 2: 242 registers, the merge laterals 3.039 / 1.376 / 0.621 ms against 3.042 / 1.364 / 0.621: what these
          // launches wait for is not the gather's latency)
          if (p.up) {       // same arithmetic as upsample_add_kernel (pointwise.hip): interp first, then + lateral
#pragma clang fp contract(off)   // like torch's CPU upsample_bilinear2d: no fused multiply-adds in the coordinates or the
                                 // blend (the compiler fused `scale * o - floor` in one instantiation of this kernel and not in
                                 // another: 5e-6 apart)
            const float* ub = p.up + n;
            f32x4 v00, v01, v10, v11;
            float ly, lx, hy, hx;
            if constexpr (!ROWS) {                       // the row's table entry (above)
              const int* u = Ut + 8 * r;
              v00 = *reinterpret_cast<const f32x4*>(ub + (long long)u[0] * p.N);
              v01 = *reinterpret_cast<const f32x4*>(ub + (long long)u[1] * p.N);
              v10 = *reinterpret_cast<const f32x4*>(ub + (long long)u[2] * p.N);
              v11 = *reinterpret_cast<const f32x4*>(ub + (long long)u[3] * p.N);
              ly = __int_as_float(u[4]); lx = __int_as_float(u[5]); hy = __int_as_float(u[6]); hx = __int_as_float(u[7]);
            } else {
              const int b = (int)nbm_fdiv((unsigned)m, p.fd_howo), rem = (int)(m - (long long)b * p.HoWo);
              const int oy = (int)nbm_fdiv((unsigned)rem, p.fd_wo), ox = rem - oy * p.Wo;
              const float fy = p.up_sh * oy, fx = p.up_sw * ox;
              const int y0 = (int)fy, x0 = (int)fx;
              const int y1 = y0 + (y0 < p.up_H - 1 ? 1 : 0), x1 = x0 + (x0 < p.up_W - 1 ? 1 : 0);
              ly = fminf(fmaxf(fy - y0, 0.f), 1.f); lx = fminf(fmaxf(fx - x0, 0.f), 1.f);
              hy = 1.f - ly; hx = 1.f - lx;
              const long long rb = (long long)b * p.up_H;
              v00 = *reinterpret_cast<const f32x4*>(ub + ((rb + y0) * p.up_W + x0) * p.N);
              v01 = *reinterpret_cast<const f32x4*>(ub + ((rb + y0) * p.up_W + x1) * p.N);
              v10 = *reinterpret_cast<const f32x4*>(ub + ((rb + y1) * p.up_W + x0) * p.N);
              v11 = *reinterpret_cast<const f32x4*>(ub + ((rb + y1) * p.up_W + x1) * p.N);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
              v[e] = (hy * (hx * v00[e] + lx * v01[e]) + ly * (hx * v10[e] + lx * v11[e])) + v[e];
          }
          v = epi_act4(v, p.act);
          if (!ROWS && p.mask) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(p.mask + (long long)m * p.mask_ld + n);
#pragma unroll
            for (int e = 0; e < 4; ++e) if (!(q[e] > 0.f)) v[e] = 0.f;
          }
          if (!ROWS && p.bits_out) {
            // the 8 consecutive lanes that share a row's 32-channel word (bn0 % 32 == 0, N % 32 == 0: rows and column range are uniform
            // over the group)
            const unsigned wb = epi_relu_bits(v, 8 * ((tid & 63) >> 3));
            if ((cc & 7) == 0) p.bits_out[(long long)m * (p.N >> 5) + (n >> 5)] = wb;
          }
          *reinterpret_cast<f32x4*>(yg + (long long)m * p.y_ld + n) = v;
        }
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int n = bn0 + wn0 + j * 32 + lrow;
      if (n >= p.N) continue;
      const float sc = p.scale ? p.scale[n] : 1.0f;
      const float sh = (p.shift && !p.shift_per_row) ? p.shift[n] : 0.0f;
#pragma unroll
      for (int i = 0; i < MT; ++i) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int m = bm0 + wm0 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
          if (m >= p.M) continue;
          // not epi_affine4's expression: without a per-row shift nothing is added here, where the vector path adds 0.f (-0.f -> +0.f)
          float v = acc[i][j][e] * p.alpha;
          v = v * sc + sh;
          if (p.shift_per_row && p.shift) v += p.shift[m];
          if (rg) v += rg[(long long)m * p.res_ld + n];
          v = epi_act(v, p.act);
          if (p.mask && !(p.mask[(long long)m * p.mask_ld + n] > 0.f)) v = 0.f;
          yg[(long long)m * p.y_ld + n] = v;
        }
      }
    }
  }
}

}  // namespace
