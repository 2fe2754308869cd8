// Backward implicit GEMMs on the gfx950 fp32 matrix core (v_mfma_f32_32x32x2_f32).
//
//   NN  (data gradient):   dX[m][c] = sum_{r,s,n} G[pix(m,r,s)][n] * a_scale[n] * W[n][r][s][c]
//        m enumerates the INPUT pixels of the forward convolution; a forward stride > 1 is handled as a dilated gather
//        of G (only taps with (iy+pad-r) % stride == 0 contribute).  A operand: gathered G rows, n contiguous;
//        B operand "K-major": the KRSC weight rows W[n][r][s][:] are already contiguous along c, no transposed copy
//        of the weights is ever made.  Also serves plain C = A * B ("NN") GEMMs (attention dQ, P.V, dX of linears).
//   TN  (weight gradient): dW[n][r][s][c] += row_scale[n] * sum_m G[m][n] * X[pix(m,r,s)][c]
//        reduction over the output pixels, split over gridDim.y chunks, fp32 atomics into a zeroed dW (KRSC).  Both
//        operands are K-major (pixel-major, exactly as they lie in HBM), so neither is transposed: the MFMA fragments
//        are read from LDS with 16 ds_read_b32 (conflict-free: 32 consecutive floats per half-wave).
//
// Same structure as igemm.hip: 128 x BN x 32 tiles, 4 waves, double-buffered LDS with one barrier per K-step, operands
// fetched with branch-free raw buffer loads (invalid taps / rows get an out-of-range offset and read zeros), global
// loads issued two tiles ahead and, like the LDS writes, scheduled between the MFMAs of the running K-step.
#include <stdlib.h>
#include "nbm_common.h"
#include "igemm_split_tn.h"
#include "igemm_device.h"
#include <type_traits>
#include "nbm_ordered_sum.h"

namespace {

constexpr int BK = 32;
constexpr int PITCH = 36;     // row-major-K tile: [rows][32 + 4]
constexpr unsigned OOB = 0x80000000u;

struct BwdParams {
  const float* g; const float* w; const float* x; float* out;
  const float* a_scale;      // NN: per-n multiplier of G (FrozenBN scale) or null
  const float* row_scale;    // TN: per-n multiplier of dW rows or null
  const float* residual;     // NN: added to dX (gradient accumulation) or null
  const float* mask;         // NN: forward output of the producer; dX is zeroed where mask <= 0 (ReLU) or null
  const unsigned* mask_bits; // NN: the same mask as bits, [M][Cin / 32] words (nbm_gemm_desc.bits_out of the producer), or null
  const float* residual2;    // NN: a HALF-resolution map [B][ceil(H/2)][ceil(W/2)][Cin] added at the pixels with even iy and ix, or null
  int res2_ld;
  long long g_gs, w_gs, x_gs, out_gs, res_gs;
  int B, H, W, Cin, N, kh, kw, stride, pad, Ho, Wo;
  int g_ld, w_ld, x_ld, out_ld, res_ld, mask_ld;
  int M;                     // NN: B*H*W input pixels; TN: B*Ho*Wo output pixels
  int m_tiles, n_tiles;
  int k_chunk;               // TN: pixels per split
  float alpha;
  int b_generic;             // TN: gather the X tile element-wise (Cin % 4 != 0)
  int w_row;                 // NN: floats between W[n] and W[n+1] (= taps*Cin, or the padded pitch)
  int vec_epi;               // NN: 16-byte epilogue accesses are legal
  float* bias_grad;          // TN: += sum_m g[m][n] (added by the workgroups of the first N-tile) or null
  int plain;                 // TN: 1x1 / stride 1 / pad 0 -- im2col row m IS input pixel m, no bounds to track
  int phased;                // NN, stride 2: M tiles are grouped by the parity class of (iy + pad, ix + pad)
  int ph_tiles[4];           //   M tiles of each class; tile_m = 4 * (tile within class) + class, so the four classes of
                             //   one image region run side by side and fill the same DRAM pages together
  // NN: launch-invariant divisors of the row decode (nbm_fastdiv, nbm_common.h): pixels per image and row width of the (parity class's)
  // pixel grid, the stride, and the full grid again for the half-resolution residual
  nbm_fastdiv fd_hw[4], fd_w[4], fd_st, fd_HW, fd_W;
  nbm_fastdiv fd_howo, fd_wo;   // TN: output pixels per image, output row width
  // TN, deterministic twin (DET instantiations only): split s STORES its scaled tile at ws + s * ws_stride + grp * N * ws_ld + n * ws_ld
  // + col and its bias partial at ws + s * ws_stride + groups * N * ws_ld + grp * N + n; nbm_ordered_sum_launch adds the slices in split order
  float* ws; long long ws_stride; int groups, ws_ld;
};

__device__ __forceinline__ f32x4 buf_load4(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}

// ---------------------------------------------------------------------------------------------------- NN
// STAGES = 2: the deep-K pipeline.  STAGES = 1 (round 3): short-K layers (N * taps <= 256: the 1x1 data gradients of the ResNet
// bottlenecks, whose time is the dX / shortcut-gradient / ReLU-mask traffic of the epilogue, not MFMA): one LDS buffer (35 KB)
// and an epilogue staged in two halves, so THREE workgroups fit a CU and their load / compute / store phases overlap -- the same
// trade as igemm.hip's STAGES = 1 forward variant.
// HS (round 5, STAGES = 2 only): HALF-STEP LDS stages like igemm_h16.hip -- a stage holds 16 of the 32 K values of a step (A rows of 20
// floats, 16 B rows), the epilogue goes out in two halves like the single-stage form's, and THREE workgroups share a CU.  Half-step h
// holds k = 8h .. 8h + 7 (A columns / B rows 0..7, fed by lanes 0..31) and k = 16 + 8h .. (columns / rows 8..15, lanes 32..63): its two
// MFMA groups are groups 2h, 2h + 1 of the full step -- the same products in the same order, the same bits.
template <int BN, int STAGES = 2, bool HS = false>
__global__ __launch_bounds__(256, (STAGES == 1 || HS) ? 3 : 2) void igemm_nn_kernel(const BwdParams p) {
  static_assert(!HS || STAGES == 2, "half-step stages are a form of the two-stage pipeline");
  constexpr int BM = 128, WM = 64, WN = BN / 2, MT = 2, NT = WN / 32;
  constexpr int BP = BN + 4;                                   // K-major B tile pitch
  constexpr int KS = HS ? 16 : BK;                             // K values per LDS stage
  constexpr int AP = HS ? 20 : PITCH;                          // A tile pitch (16 + 4 / 32 + 4 floats)
  constexpr int NG = KS / 8;                                   // MFMA groups (4 k-pairs each) per stage
  __shared__ __attribute__((aligned(16))) float lds[STAGES * (BM * AP + KS * BP)];
  float* As = lds;
  float* Bs = lds + STAGES * BM * AP;
  if constexpr (STAGES == 2) nbm_stagger_priority();

  const int wg = xcd_tile(gridDim.x, blockIdx.x);
  const int tile_m = wg / p.n_tiles, tile_n = wg - tile_m * p.n_tiles;
  const int bm0 = tile_m * BM, bn0 = tile_n * BN;
  const int grp = blockIdx.z;
  const float* __restrict__ gg = p.g + (long long)grp * p.g_gs;
  const float* __restrict__ wg_ = p.w + (long long)grp * p.w_gs;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm0 = (wave >> 1) * WM, wn0 = (wave & 1) * WN;
  const int lrow = lane & 31, lh = lane >> 5;
  const int st = p.stride;
  // v / stride for v >= 0 through a host-prepared multiplier: a 32-bit division by a run-time value is ~35 vector instructions, and the
  // tap loop of the prologue did 4 of them per (row, tap) (144 per thread for a 3x3), `load_tiles` 2 per K-step, the row decode 2 per row
  auto divst = [&](int v) -> int { return (int)nbm_fdiv((unsigned)v, p.fd_st); };
  const int frm = divst(p.kh - 1), fsm = divst(p.kw - 1);      // largest tap shift in G rows / columns

  // Row -> input pixel.  Plain: row q = bm0 + r enumerates (b, iy, ix) row-major.  Phased (stride 2): a pixel only
  // receives the taps with r = (iy + pad) mod 2, s = (ix + pad) mod 2, so the M tiles are grouped by that parity class;
  // a tile enumerates its class's sub-grid (b, u, v) -> (2u + y0, 2v + x0) and its K loop visits the class's taps only
  // (1, 2, 2 or 4 of the 9 taps of a 3x3 instead of all 9 with 3/4 of the loads masked to zero).
  int y0 = 0, x0 = 0, Hp = p.H, Wp = p.W, rows_here = p.M, q0 = bm0, r_begin = 0, s_begin = 0, t_step = 1;
  if (p.phased) {
    const int ph = tile_m & 3;
    if ((tile_m >> 2) >= p.ph_tiles[ph]) return;               // classes differ by at most a row / column of tiles
    q0 = (tile_m >> 2) * BM;
    r_begin = ph >> 1; s_begin = ph & 1; t_step = 2;
    y0 = (r_begin + p.pad) & 1; x0 = (s_begin + p.pad) & 1;
    Hp = (p.H - y0 + 1) >> 1; Wp = (p.W - x0 + 1) >> 1;
    rows_here = p.B * Hp * Wp;
  }
  const nbm_fastdiv dv_hw = p.fd_hw[p.phased ? (tile_m & 3) : 0], dv_w = p.fd_w[p.phased ? (tile_m & 3) : 0];
  auto decode = [&](int q, int& b, int& iy, int& ix) -> bool {
    const bool ok = q < rows_here;
    const int qq = ok ? q : 0, hw = Hp * Wp;
    b = (int)nbm_fdiv((unsigned)qq, dv_hw);
    const int rem = qq - b * hw, u = (int)nbm_fdiv((unsigned)rem, dv_w), v = rem - u * Wp;
    iy = p.phased ? 2 * u + y0 : u;
    ix = p.phased ? 2 * v + x0 : v;
    return ok;
  };

  // A staging: 128 rows x 8 (half-step: 4) chunks of 16 B.  Row i gathers G at (b, fy - r/st, fx - s/st) for the taps whose parity
  // matches; offsets are relative to a block-uniform base shifted by the largest tap so that they stay non-negative.
  constexpr int ACH = KS / 4, ARPP = 256 / ACH, AR = BM / ARPP;      // chunks per row, rows per pass, rows per thread
  const int c4 = tid % ACH, r0 = tid / ACH;
  // first K value (of the 32 of a step) of this thread's chunk: 4 c4, or -- half-step -- 0, 4, 16, 20 (+ 8 h)
  const int koff = HS ? (c4 < 2 ? 4 * c4 : 16 + 4 * (c4 - 2)) : 4 * c4;
  unsigned a_rel[AR];
  unsigned long long a_taps[AR];
  long long blk_base;
  {
    int b, iy, ix;
    decode(q0, b, iy, ix);
    // column 0 of the first row's G row: with stride > 1 two consecutive input rows can map to the SAME G row, so the
    // first pixel of the tile is not necessarily the smallest address (offsets must stay non-negative)
    (void)ix;
    blk_base = ((long long)(b * p.Ho + divst(iy + p.pad)) * p.Wo) * p.g_ld;
  }
#pragma unroll
  for (int i = 0; i < AR; ++i) {
    int b, iy, ix;
    const bool ok = decode(q0 + r0 + ARPP * i, b, iy, ix);
    const int fy = divst(iy + p.pad), fx = divst(ix + p.pad);
    const int py = (iy + p.pad) - fy * st, px = (ix + p.pad) - fx * st;
    const long long base = ((long long)(b * p.Ho + fy) * p.Wo + fx) * p.g_ld;
    a_rel[i] = ((unsigned)(base - blk_base) + koff) * 4u;
    // taps that reach this pixel: filter rows r with r = py (mod stride) whose G row fy - r / stride exists, likewise columns, then their
    // product -- selects only (as a kh x kw nest of data-dependent branches this was the longest part of the tile prologue: 28 k of the
    // 37 k cycles in front of the first load of a 3x3 tile, cycle counters of a timing-only attribution build, round 5)
    unsigned long long mk = 0ull;
    unsigned rowm = 0u, colm = 0u;
    for (int r = 0; r < p.kh; ++r) {
      const int rq = divst(r);
      rowm |= ((r - rq * st == py && (unsigned)(fy - rq) < (unsigned)p.Ho) ? 1u : 0u) << r;
    }
    for (int s = 0; s < p.kw; ++s) {
      const int sq = divst(s);
      colm |= ((s - sq * st == px && (unsigned)(fx - sq) < (unsigned)p.Wo) ? 1u : 0u) << s;
    }
    for (int r = 0; r < p.kh; ++r) mk |= ((rowm >> r) & 1u) ? (unsigned long long)colm << (r * p.kw) : 0ull;
    a_taps[i] = ok ? mk : 0ull;
  }
  const long long maxoff = ((long long)frm * p.Wo + fsm) * p.g_ld;
  const __amdgpu_buffer_rsrc_t rsrc_a = make_rsrc(gg + blk_base - maxoff, 0x7ffffff0u);

  // B staging (K-major): 32 rows x BN/4 chunks; thread -> rows rk0 + (256/(BN/4)) * i
  constexpr int BCH = BN / 4, BROWS = 256 / BCH, BPASS = KS / BROWS;
  const int bc = tid % BCH, rk0 = tid / BCH;
  unsigned b_rel[BPASS];
#pragma unroll
  for (int i = 0; i < BPASS; ++i) {
    const int j = rk0 + BROWS * i;                               // LDS row; half-step: rows 8..15 hold k = 16 + (row - 8) (+ 8 h)
    const int kk = HS ? (j < 8 ? j : j + 8) : j;
    b_rel[i] = (bn0 + bc * 4 < p.Cin) ? (unsigned)(kk * p.w_row + bn0 + bc * 4) * 4u : OOB;
  }
  // rows n >= N fall outside the resource and read zeros
  const long long wbytes = (long long)p.N * p.w_row * 4;
  const __amdgpu_buffer_rsrc_t rsrc_b = make_rsrc(wg_, (unsigned)(wbytes < 0x7ffffff0ll ? wbytes : 0x7ffffff0ll));

  f32x4 ra[AR], rb[BPASS], rsc = {1.f, 1.f, 1.f, 1.f};
  int cur_r = r_begin, cur_s = s_begin, cur_n0 = 0, cur_h = 0;

  auto load_tiles = [&]() {
    const int tap = cur_r * p.kw + cur_s;
    const int n0h = cur_n0 + 8 * cur_h;                                    // (half-step: the second half starts 8 K values further)
    const unsigned a_soff = (unsigned)((maxoff - ((long long)divst(cur_r) * p.Wo + divst(cur_s)) * p.g_ld + n0h) * 4);
    const unsigned b_soff = (unsigned)(((long long)n0h * p.w_row + (long long)tap * p.Cin) * 4);
#pragma unroll
    for (int i = 0; i < AR; ++i) ra[i] = buf_load4(rsrc_a, ((a_taps[i] >> tap) & 1ull) ? a_rel[i] : OOB, a_soff);
#pragma unroll
    for (int i = 0; i < BPASS; ++i) rb[i] = buf_load4(rsrc_b, b_rel[i], b_soff);
    if (p.a_scale) rsc = *reinterpret_cast<const f32x4*>(p.a_scale + n0h + koff);
    if (HS && (cur_h ^= 1) != 0) return;                                   // the other half of the same (tap, 32-wide K) step comes next
    cur_s += t_step;
    if (cur_s >= p.kw) { cur_s = s_begin; cur_r += t_step; if (cur_r >= p.kh) { cur_r = r_begin; cur_n0 += BK; } }
  };
  auto store_lds = [&](int buf) {
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      f32x4 v = ra[i];
      v[0] *= rsc[0]; v[1] *= rsc[1]; v[2] *= rsc[2]; v[3] *= rsc[3];
      *reinterpret_cast<f32x4*>(As + (buf * BM + r0 + ARPP * i) * AP + c4 * 4) = v;
    }
#pragma unroll
    for (int i = 0; i < BPASS; ++i)
      *reinterpret_cast<f32x4*>(Bs + (buf * KS + rk0 + BROWS * i) * BP + bc * 4) = rb[i];
  };

  f32x16 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  auto mfma_group = [&](const float* Ab, const float* Bb, int q) {
    f32x4 a[MT];
    float b[NT][4];
#pragma unroll
    for (int i = 0; i < MT; ++i) a[i] = *reinterpret_cast<const f32x4*>(Ab + i * 32 * AP + q * 4);
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) b[j][e] = Bb[(q * 4 + e) * BP + j * 32];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][e], b[j][e], acc[i][j], 0, 0, 0);
  };

  const int n_r = r_begin < p.kh ? (p.kh - r_begin + t_step - 1) / t_step : 0;
  const int n_s = s_begin < p.kw ? (p.kw - s_begin + t_step - 1) / t_step : 0;
  const int nk = ((p.N + BK - 1) / BK) * n_r * n_s;          // 0: no tap reaches this parity class, dX = residual
  const int n_st = HS ? 2 * nk : nk;                             // LDS stages of the K loop
  if constexpr (STAGES == 2) {
    if (n_st > 0) {
      load_tiles();
      store_lds(0);
    }
    if (n_st > 1) load_tiles();
  }

  auto k_step = [&](int kt, auto store_c, auto load_c) {
    constexpr bool STORE = decltype(store_c)::value, LOAD = decltype(load_c)::value;
    const int cur = kt & 1;
    __syncthreads();
    const float* Ab = As + (cur * BM + wm0 + lrow) * AP + lh * (KS / 2);
    const float* Bb = Bs + (cur * KS + lh * (KS / 2)) * BP + wn0 + lrow;
    mfma_group(Ab, Bb, 0);
    if constexpr (STORE) {
      store_lds(cur ^ 1);
      __builtin_amdgcn_sched_group_barrier(0x100, MT + 4 * NT, 0);
#pragma unroll
      for (int z = 0; z < AR + BPASS; ++z) {
        __builtin_amdgcn_sched_group_barrier(0x008, (4 * MT * NT) / (AR + BPASS), 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
        __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    mfma_group(Ab, Bb, 1);
    if constexpr (LOAD) {
      load_tiles();
      __builtin_amdgcn_sched_group_barrier(0x100, MT + 4 * NT, 0);
#pragma unroll
      for (int z = 0; z < AR + BPASS; ++z) {
        __builtin_amdgcn_sched_group_barrier(0x008, (4 * MT * NT) / (AR + BPASS), 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (NG == 4) {
      mfma_group(Ab, Bb, 2);
      mfma_group(Ab, Bb, 3);
    }
  };
  if constexpr (STAGES == 2) {
    using T = std::true_type;
    using F = std::false_type;
    int kt = 0;
    for (; kt + 2 < n_st; ++kt) k_step(kt, T{}, T{});
    if (n_st >= 2) { k_step(kt, T{}, F{}); ++kt; }
    if (n_st >= 1) k_step(kt, F{}, F{});
  } else {
    // short K: load -> LDS -> MFMA, the next tile's loads in flight during the MFMAs; the other two workgroups of the CU cover
    // the barriers
    if (nk > 0) load_tiles();
    for (int kt = 0; kt < nk; ++kt) {
      if (kt) __syncthreads();                       // everyone finished reading the previous tile
      store_lds(0);
      if (kt + 1 < nk) load_tiles();
      __syncthreads();
      const float* Ab = As + (wm0 + lrow) * PITCH + lh * 16;
      const float* Bb = Bs + (lh * 16) * BP + wn0 + lrow;
#pragma unroll
      for (int q = 0; q < 4; ++q) mfma_group(Ab, Bb, q);
    }
  }
  __syncthreads();

  float* __restrict__ og = p.out + (long long)grp * p.out_gs;
  const float* __restrict__ rg = p.residual ? p.residual + (long long)grp * p.res_gs : nullptr;
  const unsigned* __restrict__ mb_ = p.mask_bits;     // the mask as bits takes precedence
  const float* __restrict__ mk_ = mb_ ? nullptr : p.mask;
  const float* __restrict__ r2_ = p.residual2;
  auto out_pixel = [&](int q) -> long long {                  // output row of tile row q (q < rows_here)
    if (!p.phased) return q;
    int b, iy, ix;
    decode(q, b, iy, ix);
    return ((long long)b * p.H + iy) * p.W + ix;
  };
  if (p.vec_epi) {
    // accumulator tile -> LDS -> 16-byte residual / mask loads and stores (see igemm.hip)
    constexpr int CP = BN + 4;
    constexpr int HALVES = (STAGES == 1 || HS) ? BM / WM : 1;  // the single-stage / half-step LDS holds WM rows of the tile at a time
    constexpr int HROWS = BM / HALVES;
    static_assert(HROWS * CP + 2 * HROWS <= STAGES * (BM * AP + KS * BP), "epilogue tile + row table must fit the operand buffers");
    float* Cs = lds;
    // stride 2: the output pixel of a tile row (parity-class sub-grid -> image) is decoded ONCE per row into LDS, not by each of the row's
    // BN / 4 threads in the prefetch AND in the store loop (two fast divisions + the parity arithmetic per call; round 5)
    long long* const Rm = reinterpret_cast<long long*>(lds + HROWS * CP);     // [HROWS]; HROWS * CP is even
    constexpr int CH = BN / 4, RPP = 256 / CH;
    const int cc = tid % CH, rr = tid / CH;
    const int c = bn0 + cc * 4;
    constexpr int NR = (HROWS + RPP - 1) / RPP;                 // tile rows a thread finishes
#pragma unroll
    for (int half = 0; half < HALVES; ++half) {
      if (HALVES > 1 && half) __syncthreads();                  // the previous half has been read
      if (p.phased) {
        if (tid < HROWS) Rm[tid] = out_pixel(min(q0 + half * HROWS + tid, rows_here - 1));
        __syncthreads();
      }
      auto row_out = [&](int rl) -> long long {                 // output pixel of row rl of this half (clamped to the last row of the class)
        return p.phased ? Rm[rl] : (long long)min(q0 + half * HROWS + rl, rows_here - 1);
      };
      // residual / mask values of this thread's rows: requested before the accumulators go through LDS (inside the row loop, behind
      // its exit test, they were 2 NR dependent round trips at the end of every tile -- igemm.hip)
      f32x4 rq[NR], mq[NR];
      unsigned mw[NR];                                          // mask words (Cin % 32 == 0: the word of channels c .. c + 3 of the row)
      const bool pre = c < p.Cin && (rg || mk_ || mb_);
      if (pre) {
#pragma unroll
        for (int k = 0; k < NR; ++k) {
          const long long m = row_out(min(rr + k * RPP, HROWS - 1));
          if (rg) rq[k] = *reinterpret_cast<const f32x4*>(rg + m * p.res_ld + c);
          if (mk_) mq[k] = *reinterpret_cast<const f32x4*>(mk_ + m * p.mask_ld + c);
          if (mb_) mw[k] = mb_[m * (p.Cin >> 5) + (c >> 5)];
        }
      }
      if (HALVES == 1 || wm0 == half * HROWS) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e)
              Cs[(wm0 - half * HROWS + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh) * CP + wn0 + j * 32 + lrow] = acc[i][j][e];
      }
      __syncthreads();
      if (c >= p.Cin) continue;
#pragma unroll
      for (int k = 0; k < NR; ++k) {
        const int rl = rr + k * RPP;
        if (rl >= HROWS) break;
        const int r = half * HROWS + rl;
        if (q0 + r >= rows_here) break;
        const long long m = row_out(rl);
        f32x4 v = *reinterpret_cast<const f32x4*>(Cs + rl * CP + cc * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] *= p.alpha;
        if (rg) {
          const f32x4 q = rq[k];
          v[0] += q[0]; v[1] += q[1]; v[2] += q[2]; v[3] += q[3];
        }
        if (r2_) {          // the data gradient of a 1x1 / stride-2 shortcut, kept at its own (half) resolution
          const int hw = p.H * p.W, b_ = (int)nbm_fdiv((unsigned)m, p.fd_HW), rem_ = (int)(m - (long long)b_ * hw);
          const int iy_ = (int)nbm_fdiv((unsigned)rem_, p.fd_W), ix_ = rem_ - iy_ * p.W;
          if (!((iy_ | ix_) & 1)) {
            const long long m2 = ((long long)b_ * ((p.H + 1) >> 1) + (iy_ >> 1)) * ((p.W + 1) >> 1) + (ix_ >> 1);
            const f32x4 q = *reinterpret_cast<const f32x4*>(r2_ + m2 * p.res2_ld + c);
            v[0] += q[0]; v[1] += q[1]; v[2] += q[2]; v[3] += q[3];
          }
        }
        if (mk_) {
          const f32x4 q = mq[k];
#pragma unroll
          for (int e = 0; e < 4; ++e) if (!(q[e] > 0.f)) v[e] = 0.f;
        }
        if (mb_) {
          const unsigned by = mw[k] >> ((c >> 2) & 7);        // bit 8 e + q of the word <-> channel 4 q + e (nbm_hip.h)
#pragma unroll
          for (int e = 0; e < 4; ++e) if (!((by >> (8 * e)) & 1u)) v[e] = 0.f;
        }
        *reinterpret_cast<f32x4*>(og + (long long)m * p.out_ld + c) = v;
      }
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int c = bn0 + wn0 + j * 32 + lrow;
    if (c >= p.Cin) continue;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int q = q0 + wm0 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        if (q >= rows_here) continue;
        const long long m = out_pixel(q);
        float v = acc[i][j][e] * p.alpha;
        if (rg) v += rg[(long long)m * p.res_ld + c];
        if (r2_) {
          const int hw = p.H * p.W, b_ = (int)nbm_fdiv((unsigned)m, p.fd_HW), rem_ = (int)(m - (long long)b_ * hw);
          const int iy_ = (int)nbm_fdiv((unsigned)rem_, p.fd_W), ix_ = rem_ - iy_ * p.W;
          if (!((iy_ | ix_) & 1))
            v += r2_[(((long long)b_ * ((p.H + 1) >> 1) + (iy_ >> 1)) * ((p.W + 1) >> 1) + (ix_ >> 1)) * p.res2_ld + c];
        }
        if (mk_ && !(mk_[(long long)m * p.mask_ld + c] > 0.f)) v = 0.f;
        if (mb_ && !((mb_[m * (p.Cin >> 5) + (c >> 5)] >> (8 * (c & 3) + ((c >> 2) & 7))) & 1u)) v = 0.f;
        og[(long long)m * p.out_ld + c] = v;
      }
  }
}

// ---------------------------------------------------------------------------------------------------- TN
// BMODE: how the X tile (im2col rows of one tap) is fetched
//   B_SAME    stride-1 'same' convolution with Wo >= 32: input pixel = output pixel + constant, so every row has a
//             constant byte offset from a per-K-step scalar base -> raw buffer loads, padding / tail rows read zeros
//   B_STRIDED any stride / small maps, 16-byte channel chunks through pointers
//   B_GENERIC unaligned or Cin % 4 != 0: scalar gather over the flattened (tap, c) axis
enum { B_SAME = 0, B_STRIDED = 1, B_GENERIC = 2 };

// BM: rows of the dW tile = output channels n of the convolution.  128 by default; 64 for layers with N <= 64 (ResNet layer1:
// with the 128-row tile half of every MFMA multiplied the zero padding of the G tile -- 59 TF/s "executed" on 3x3 64 -> 64).
// DET: the deterministic twin (nbm_bwd_desc.workspace): same K loop, the epilogue stores into the split's own slice instead of adding
// to dW / bias_grad with atomics.
template <int BN, int BMODE, int BM = 128, bool DET = false>
__global__ __launch_bounds__(256, 2) void igemm_tn_kernel(const BwdParams p) {
  constexpr int WM = BM / 2, WN = BN / 2, MT = WM / 32, NT = WN / 32;
  constexpr int AP = BM + 4, BP = BN + 4;
  __shared__ __attribute__((aligned(16))) float lds[2 * BK * AP + 2 * BK * BP];
  nbm_stagger_priority();
  float* As = lds;                    // [2][32][AP]   G tile:  pixel-major, n contiguous
  float* Bs = lds + 2 * BK * AP;      // [2][32][BP]   X tile:  pixel-major, c contiguous

  const int wg = xcd_tile(gridDim.x, blockIdx.x);
  const int tile_m = wg / p.n_tiles, tile_n = wg - tile_m * p.n_tiles;
  const int bm0 = tile_m * BM;                      // n0
  const int grp = blockIdx.z;
  const int taps = p.kh * p.kw;
  // N-tile -> (tap, c0)  [fast]   or   j0 over (tap, c) flattened  [generic]
  constexpr bool GEN = BMODE == B_GENERIC;
  const int ctiles = GEN ? 1 : (p.Cin + BN - 1) / BN;
  const int tap = GEN ? 0 : tile_n / ctiles;
  const int c0 = GEN ? 0 : (tile_n - tap * ctiles) * BN;
  const int j0 = tile_n * BN;                       // generic only
  const int tr = tap / p.kw, ts = tap - tr * p.kw;

  const float* __restrict__ gg = p.g + (long long)grp * p.g_gs;
  const float* __restrict__ xg = p.x + (long long)grp * p.x_gs;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm0 = (wave >> 1) * WM, wn0 = (wave & 1) * WN;
  const int lrow = lane & 31, lh = lane >> 5;

  constexpr int ACH = BM / 4, AROWS = 256 / ACH, APASS = BK / AROWS;   // 32 chunks, 8 rows/pass, 4 passes
  constexpr int BCH = BN / 4, BROWS = 256 / BCH, BPASS = BK / BROWS;
  const int ac = tid % ACH, ar0 = tid / ACH;
  const int bc = tid % BCH, br0 = tid / BCH;

  const int m_begin = blockIdx.y * p.k_chunk;
  const int m_end = min(p.M, m_begin + p.k_chunk);
  const int nk = (m_end - m_begin + BK - 1) / BK;
  if (nk <= 0) return;

  f32x4 ra[APASS], rb[BPASS];
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const int HoWo = p.Ho * p.Wo;

  // A rows: pixel-major G; rows beyond m_end fall outside the per-step resource and read zeros
  unsigned a_rel[APASS];
#pragma unroll
  for (int i = 0; i < APASS; ++i)
    a_rel[i] = (bm0 + ac * 4 < p.N) ? (unsigned)((ar0 + AROWS * i) * p.g_ld + bm0 + ac * 4) * 4u : OOB;
  // B rows (fast path): output pixel -> input pixel, tracked incrementally (+32 pixels per K-step)
  int b_b[BPASS], b_oy[BPASS], b_ox[BPASS];
  const bool c_ok = c0 + bc * 4 < p.Cin;
#pragma unroll
  for (int i = 0; i < BPASS; ++i) {
    const int m = m_begin + br0 + BROWS * i;
    b_b[i] = (int)nbm_fdiv((unsigned)m, p.fd_howo);
    const int rem = m - b_b[i] * HoWo;
    b_oy[i] = (int)nbm_fdiv((unsigned)rem, p.fd_wo);
    b_ox[i] = rem - b_oy[i] * p.Wo;
  }
  int kt_load = 0;
  // B_SAME: constant row offsets relative to the K-step base pixel (+ the tap's displacement)
  unsigned b_rel[BPASS];
#pragma unroll
  for (int i = 0; i < BPASS; ++i) b_rel[i] = c_ok ? (unsigned)((br0 + BROWS * i) * p.x_ld + c0 + bc * 4) * 4u : OOB;
  const long long dpix = (long long)(tr - p.pad) * p.W + (ts - p.pad);

  auto load_tiles = [&]() {
    const int mbase = m_begin + kt_load * BK;
    const int rows = min(BK, m_end - mbase);
    const __amdgpu_buffer_rsrc_t rsrc_a = make_rsrc(gg + (long long)mbase * p.g_ld, (unsigned)(rows * p.g_ld * 4));
#pragma unroll
    for (int i = 0; i < APASS; ++i) ra[i] = buf_load4(rsrc_a, a_rel[i], 0);
    if constexpr (BMODE == B_SAME) {
      const __amdgpu_buffer_rsrc_t rsrc_b = make_rsrc(xg + ((long long)mbase + dpix) * p.x_ld, (unsigned)(rows * p.x_ld * 4));
#pragma unroll
      for (int i = 0; i < BPASS; ++i) {
        if (p.plain) {                                                  // plain GEMM rows: always inside
          rb[i] = buf_load4(rsrc_b, b_rel[i], 0);
          continue;
        }
        const bool ok = (unsigned)(b_oy[i] + tr - p.pad) < (unsigned)p.H && (unsigned)(b_ox[i] + ts - p.pad) < (unsigned)p.W;
        rb[i] = buf_load4(rsrc_b, ok ? b_rel[i] : OOB, 0);
        b_ox[i] += BK;                                                  // Wo >= BK on this path
        if (b_ox[i] >= p.Wo) { b_ox[i] -= p.Wo; if (++b_oy[i] == p.Ho) b_oy[i] = 0; }
      }
    } else if constexpr (BMODE == B_STRIDED) {
#pragma unroll
      for (int i = 0; i < BPASS; ++i) {
        const int m = mbase + br0 + BROWS * i;
        const int iy = b_oy[i] * p.stride - p.pad + tr, ix = b_ox[i] * p.stride - p.pad + ts;
        const bool ok = c_ok && m < m_end && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
        const float* src = xg + ((long long)(b_b[i] * p.H + (ok ? iy : 0)) * p.W + (ok ? ix : 0)) * p.x_ld + c0 + bc * 4;
        const f32x4 v = *reinterpret_cast<const f32x4*>(ok ? src : xg);
        rb[i] = ok ? v : zero4;
        // advance this row by 32 output pixels
        if (p.Wo >= BK) {
          b_ox[i] += BK;
          if (b_ox[i] >= p.Wo) { b_ox[i] -= p.Wo; if (++b_oy[i] == p.Ho) { b_oy[i] = 0; ++b_b[i]; } }
        } else {
          const int mn = m + BK;
          b_b[i] = (int)nbm_fdiv((unsigned)mn, p.fd_howo);
          const int rem = mn - b_b[i] * HoWo;
          b_oy[i] = (int)nbm_fdiv((unsigned)rem, p.fd_wo);
          b_ox[i] = rem - b_oy[i] * p.Wo;
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < BPASS; ++i) {
        const int m = mbase + br0 + BROWS * i;
        f32x4 v = zero4;
        if (m < m_end) {
          const int b = (int)nbm_fdiv((unsigned)m, p.fd_howo), rem = m - b * HoWo;
          const int oy = (int)nbm_fdiv((unsigned)rem, p.fd_wo), ox = rem - oy * p.Wo;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int j = j0 + bc * 4 + e;
            if (j < taps * p.Cin) {
              const int t = j / p.Cin, c = j - t * p.Cin;
              const int r = t / p.kw, s = t - r * p.kw;
              const int iy = oy * p.stride - p.pad + r, ix = ox * p.stride - p.pad + s;
              if ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W)
                v[e] = xg[((long long)(b * p.H + iy) * p.W + ix) * p.x_ld + c];
            }
          }
        }
        rb[i] = v;
      }
    }
    ++kt_load;
  };
  auto store_lds = [&](int buf) {
#pragma unroll
    for (int i = 0; i < APASS; ++i)
      *reinterpret_cast<f32x4*>(As + (buf * BK + ar0 + AROWS * i) * AP + ac * 4) = ra[i];
#pragma unroll
    for (int i = 0; i < BPASS; ++i)
      *reinterpret_cast<f32x4*>(Bs + (buf * BK + br0 + BROWS * i) * BP + bc * 4) = rb[i];
  };

  f32x16 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const bool do_bias = p.bias_grad != nullptr && tile_n == 0;
  float bsum = 0.f;

  auto mfma_group = [&](const float* Ab, const float* Bb, int q) {
    float a[MT][4], b[NT][4];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) a[i][e] = Ab[(q * 4 + e) * AP + i * 32];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) b[j][e] = Bb[(q * 4 + e) * BP + j * 32];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][e], b[j][e], acc[i][j], 0, 0, 0);
  };

  load_tiles();
  store_lds(0);
  if (nk > 1) load_tiles();

  auto k_step = [&](int kt, auto store_c, auto load_c) {
    constexpr bool STORE = decltype(store_c)::value, LOAD = decltype(load_c)::value;
    const int cur = kt & 1;
    __syncthreads();
    if (do_bias) {            // workgroup-uniform: column sums of the G tile (bias gradient), 32 * BM / 256 pixels per thread
      constexpr int BT = 256 / BM, PX = BK / BT;
      const float* Ar = As + (cur * BK + (tid / BM) * PX) * AP + (tid % BM);
#pragma unroll
      for (int e = 0; e < PX; ++e) bsum += Ar[e * AP];
    }
    const float* Ab = As + (cur * BK + lh * 16) * AP + wm0 + lrow;
    const float* Bb = Bs + (cur * BK + lh * 16) * BP + wn0 + lrow;
    mfma_group(Ab, Bb, 0);
    if constexpr (STORE) {
      store_lds(cur ^ 1);
      __builtin_amdgcn_sched_group_barrier(0x100, 4 * (MT + NT), 0);
#pragma unroll
      for (int z = 0; z < APASS + BPASS; ++z) {
        __builtin_amdgcn_sched_group_barrier(0x008, (4 * MT * NT) / (APASS + BPASS) > 0 ? (4 * MT * NT) / (APASS + BPASS) : 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    mfma_group(Ab, Bb, 1);
    if constexpr (LOAD) {
      load_tiles();
      __builtin_amdgcn_sched_group_barrier(0x100, 4 * (MT + NT), 0);
#pragma unroll
      for (int z = 0; z < 4 * MT * NT; ++z) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);
        if (z < APASS + BPASS) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    mfma_group(Ab, Bb, 2);
    mfma_group(Ab, Bb, 3);
  };
  {
    using T = std::true_type;
    using F = std::false_type;
    int kt = 0;
    for (; kt + 2 < nk; ++kt) k_step(kt, T{}, T{});
    if (nk >= 2) { k_step(kt, T{}, F{}); ++kt; }
    k_step(kt, F{}, F{});
  }

  if (do_bias) {
    const int n = bm0 + (tid % BM);
    if constexpr (DET) {
      // (256 / BM threads hold shares of one column: added in thread order through LDS, then one store)
      constexpr int BT = 256 / BM;
      __syncthreads();
      As[tid] = bsum;
      __syncthreads();
      if (tid < BM && n < p.N) {
        float t = As[tid];
#pragma unroll
        for (int k = 1; k < BT; ++k) t += As[tid + k * BM];
        p.ws[(long long)blockIdx.y * p.ws_stride + (long long)p.groups * p.N * p.ws_ld + (long long)grp * p.N + n] = t;
      }
    } else if (n < p.N) {
      atomicAdd(p.bias_grad + (long long)grp * p.N + n, bsum);
    }
  }
  float* __restrict__ og = DET ? p.ws + (long long)blockIdx.y * p.ws_stride + (long long)grp * p.N * p.ws_ld
                               : p.out + (long long)grp * p.out_gs;
  const int o_ld = DET ? p.ws_ld : p.out_ld;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int jj = wn0 + j * 32 + lrow;
    int col;
    if constexpr (!GEN) { const int c = c0 + jj; if (c >= p.Cin) continue; col = tap * p.Cin + c; }
    else { col = j0 + jj; if (col >= taps * p.Cin) continue; }
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int n = bm0 + wm0 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        if (n >= p.N) continue;
        float v = acc[i][j][e] * p.alpha;
        if (p.row_scale) v *= p.row_scale[n];
        if constexpr (DET) og[(long long)n * o_ld + col] = v;
        else atomicAdd(og + (long long)n * o_ld + col, v);
      }
  }
}

}  // namespace


using namespace nbm_igemm;

static BwdParams fill_common(const nbm_bwd_desc* d, const GemmPlan& pl) {
  BwdParams p{};
  p.g = d->g; p.w = d->w; p.x = d->x; p.out = d->out;
  p.a_scale = d->a_scale; p.row_scale = d->row_scale; p.residual = d->residual; p.mask = d->mask;
  p.residual2 = d->residual2; p.res2_ld = d->res2_ld;
  p.g_gs = d->g_gs; p.w_gs = d->w_gs; p.x_gs = d->x_gs; p.out_gs = d->out_gs; p.res_gs = d->res_gs;
  p.B = d->B; p.H = d->H; p.W = d->W; p.Cin = d->Cin; p.N = d->N; p.kh = d->kh; p.kw = d->kw;
  p.stride = d->stride; p.pad = d->pad; p.Ho = d->Ho; p.Wo = d->Wo;
  p.fd_howo = nbm_fastdiv_make((unsigned)(d->Ho * d->Wo)); p.fd_wo = nbm_fastdiv_make((unsigned)d->Wo);
  p.g_ld = d->g_ld; p.w_ld = d->w_ld; p.x_ld = d->x_ld; p.out_ld = d->out_ld; p.res_ld = d->res_ld; p.mask_ld = d->mask_ld;
  p.alpha = d->alpha;
  p.bias_grad = d->bias_grad;
  p.m_tiles = pl.m_tiles; p.n_tiles = pl.n_tiles;
  return p;
}

extern "C" int nbm_conv_dgrad(const nbm_bwd_desc* d, void* stream) {
  if (!d) return NBM_EINVAL;
  const GemmPlan pl = plan_dgrad(*d, read_gemm_switches(1));
  if (pl.rc) return pl.rc;
  BwdParams p = fill_common(d, pl);
  p.mask_bits = d->mask_bits;
  p.M = d->B * d->H * d->W;
  p.w_row = d->w_ld;
  p.vec_epi = pl.vec_epi;
  p.fd_st = nbm_fastdiv_make((unsigned)d->stride);
  p.fd_HW = p.fd_hw[0] = nbm_fastdiv_make((unsigned)(d->H * d->W));
  p.fd_W = p.fd_w[0] = nbm_fastdiv_make((unsigned)d->W);
  p.phased = pl.phased;
  if (pl.phased) {                       // the M tiles grouped by parity class (see igemm_nn_kernel)
    for (int ph = 0; ph < 4; ++ph) {
      const int y0 = ((ph >> 1) + d->pad) & 1, x0 = ((ph & 1) + d->pad) & 1;
      const int Hp = (d->H - y0 + 1) >> 1, Wp = (d->W - x0 + 1) >> 1;
      p.ph_tiles[ph] = pl.ph_tiles[ph];
      p.fd_hw[ph] = nbm_fastdiv_make((unsigned)(Hp * Wp));     // (an empty class: no tile of it gets past its early exit)
      p.fd_w[ph] = nbm_fastdiv_make((unsigned)Wp);
    }
  }
  const dim3 grid(pl.grid[0], pl.grid[1], pl.grid[2]), block(pl.block);
  hipStream_t st = (hipStream_t)stream;
  switch (pl.kernel) {
    case K_NN_128_S1: hipLaunchKernelGGL((igemm_nn_kernel<128, 1>), grid, block, 0, st, p); break;
    case K_NN_128_H16: hipLaunchKernelGGL((igemm_nn_kernel<128, 2, true>), grid, block, 0, st, p); break;
    case K_NN_128: hipLaunchKernelGGL((igemm_nn_kernel<128, 2>), grid, block, 0, st, p); break;
    case K_NN_64_S1: hipLaunchKernelGGL((igemm_nn_kernel<64, 1>), grid, block, 0, st, p); break;
    case K_NN_64_H16: hipLaunchKernelGGL((igemm_nn_kernel<64, 2, true>), grid, block, 0, st, p); break;
    case K_NN_64: hipLaunchKernelGGL((igemm_nn_kernel<64, 2>), grid, block, 0, st, p); break;
    default: return NBM_EINVAL;
  }
  return nbm_launch_status();
}

extern "C" int nbm_conv_wgrad_workspace(const nbm_bwd_desc* d, int64_t* bytes, int64_t* split_stride) {
  if (!d || !bytes) return NBM_EINVAL;
  int rc = 0;
  *bytes = wgrad_workspace_bytes(*d, read_gemm_switches(2), &rc);
  if (!rc && split_stride) *split_stride = wgrad_slice_floats(*d);
  return rc;
}

extern "C" int nbm_conv_wgrad(const nbm_bwd_desc* d, void* stream) {
  if (!d) return NBM_EINVAL;
  const GemmPlan pl = plan_wgrad(*d, read_gemm_switches(2));
  if (pl.rc) return pl.rc;
  if (pl.halves) {               // Cin is 64 past a multiple of 128: the first Cin - 64 columns, then the last 64 (see plan_wgrad)
    nbm_bwd_desc a = *d, b = *d;
    a.Cin = d->Cin - 64;
    b.Cin = 64;
    b.x = d->x + (d->Cin - 64);
    b.out = d->out + (d->Cin - 64);
    b.bias_grad = nullptr;                                   // (the column sums of G come from the first launch)
    const int rc = nbm_conv_wgrad(&a, stream);
    return rc ? rc : nbm_conv_wgrad(&b, stream);
  }
  const int M = d->B * d->Ho * d->Wo;
  const dim3 grid(pl.grid[0], pl.grid[1], pl.grid[2]), block(pl.block);
  hipStream_t st = (hipStream_t)stream;
  if (pl.kernel >= K_SPLIT_TN_R0) {
    SplitTnParams q{};
    q.g = d->g; q.x = d->x; q.out = d->out; q.row_scale = d->row_scale;
    q.g_gs = d->g_gs; q.x_gs = d->x_gs; q.out_gs = d->out_gs;
    q.M = M; q.N = d->N; q.K = d->Cin; q.g_ld = d->g_ld; q.x_ld = d->x_ld; q.out_ld = d->out_ld; q.alpha = d->alpha;
    q.n_tiles = pl.n_tiles;
    q.k_chunk = pl.k_chunk;
    return split_tn_launch(q, pl, st);
  }
  BwdParams p = fill_common(d, pl);
  p.M = M;
  p.b_generic = pl.b_generic;
  p.plain = pl.plain;
  p.k_chunk = pl.k_chunk;
  if (d->workspace) {            // the deterministic twin: every split stores its slice, nbm_ordered_sum_launch adds them in split order
    const long long slice = wgrad_slice_floats(*d);
    if (d->ws_split_stride < slice || (d->ws_split_stride & 3)) return NBM_EINVAL;
    if ((long long)pl.splits * d->ws_split_stride * 4 > d->workspace_bytes) return NBM_EINVAL;
    if (!nbm_aligned16(d->workspace)) return NBM_EALIGN;
    p.ws = d->workspace; p.ws_stride = d->ws_split_stride; p.groups = d->groups; p.ws_ld = wgrad_slice_ld(*d);
    switch (pl.kernel) {
      case K_TN_GENERIC: hipLaunchKernelGGL((igemm_tn_kernel<64, B_GENERIC, 128, true>), grid, block, 0, st, p); break;
      case K_TN_128_SAME_M64: hipLaunchKernelGGL((igemm_tn_kernel<128, B_SAME, 64, true>), grid, block, 0, st, p); break;
      case K_TN_128_STRIDED_M64: hipLaunchKernelGGL((igemm_tn_kernel<128, B_STRIDED, 64, true>), grid, block, 0, st, p); break;
      case K_TN_64_SAME_M64: hipLaunchKernelGGL((igemm_tn_kernel<64, B_SAME, 64, true>), grid, block, 0, st, p); break;
      case K_TN_64_STRIDED_M64: hipLaunchKernelGGL((igemm_tn_kernel<64, B_STRIDED, 64, true>), grid, block, 0, st, p); break;
      case K_TN_128_SAME: hipLaunchKernelGGL((igemm_tn_kernel<128, B_SAME, 128, true>), grid, block, 0, st, p); break;
      case K_TN_128_STRIDED: hipLaunchKernelGGL((igemm_tn_kernel<128, B_STRIDED, 128, true>), grid, block, 0, st, p); break;
      case K_TN_64_SAME: hipLaunchKernelGGL((igemm_tn_kernel<64, B_SAME, 128, true>), grid, block, 0, st, p); break;
      case K_TN_64_STRIDED: hipLaunchKernelGGL((igemm_tn_kernel<64, B_STRIDED, 128, true>), grid, block, 0, st, p); break;
      default: return NBM_EINVAL;
    }
    OrderedSumShape s{};
    s.slots = pl.splits; s.groups = d->groups; s.cols = d->kh * d->kw * d->Cin; s.accumulate = 1;
    s.slot_stride = d->ws_split_stride; s.part_gs = (long long)d->N * p.ws_ld; s.part_ld = p.ws_ld; s.rows = d->N;
    s.out_gs = d->out_gs; s.out_ld = d->out_ld;
    nbm_ordered_sum_launch((const float*)d->workspace, d->out, s, st);
    if (d->bias_grad) {              // the bias partials sit behind the dW rows of every slice
      OrderedSumShape b{};
      b.slots = pl.splits; b.groups = 1; b.cols = 1; b.accumulate = 1;
      b.slot_stride = d->ws_split_stride; b.part_ld = 1; b.rows = (long long)d->groups * d->N; b.out_ld = 1;
      nbm_ordered_sum_launch((const float*)d->workspace + (long long)d->groups * d->N * p.ws_ld, d->bias_grad, b, st);
    }
    return nbm_launch_status();
  }
  switch (pl.kernel) {
    case K_TN_GENERIC: hipLaunchKernelGGL((igemm_tn_kernel<64, B_GENERIC>), grid, block, 0, st, p); break;
    case K_TN_128_SAME_M64: hipLaunchKernelGGL((igemm_tn_kernel<128, B_SAME, 64>), grid, block, 0, st, p); break;
    case K_TN_128_STRIDED_M64: hipLaunchKernelGGL((igemm_tn_kernel<128, B_STRIDED, 64>), grid, block, 0, st, p); break;
    case K_TN_64_SAME_M64: hipLaunchKernelGGL((igemm_tn_kernel<64, B_SAME, 64>), grid, block, 0, st, p); break;
    case K_TN_64_STRIDED_M64: hipLaunchKernelGGL((igemm_tn_kernel<64, B_STRIDED, 64>), grid, block, 0, st, p); break;
    case K_TN_128_SAME: hipLaunchKernelGGL((igemm_tn_kernel<128, B_SAME>), grid, block, 0, st, p); break;
    case K_TN_128_STRIDED: hipLaunchKernelGGL((igemm_tn_kernel<128, B_STRIDED>), grid, block, 0, st, p); break;
    case K_TN_64_SAME: hipLaunchKernelGGL((igemm_tn_kernel<64, B_SAME>), grid, block, 0, st, p); break;
    case K_TN_64_STRIDED: hipLaunchKernelGGL((igemm_tn_kernel<64, B_STRIDED>), grid, block, 0, st, p); break;
    default: return NBM_EINVAL;
  }
  return nbm_launch_status();
}
