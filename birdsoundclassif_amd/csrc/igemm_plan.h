// Which kernel, with what grid: the launch plan of the three GEMM entry points (nbm_gemm_conv, nbm_conv_dgrad, nbm_conv_wgrad).
// Host arithmetic on a descriptor and five environment switches, nothing else: no HIP types, compiles with a plain C++17 host compiler.
// The entry points validate / plan here, fill their parameter struct from the descriptor and the plan, and launch through one switch over
// the kernel id; nbm_gemm_plan (include/nbm_hip.h) returns the same plan without launching (tests/test_gemm_plan_cpu.py pins it to a
// recorded table).
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include "nbm_hip.h"

namespace nbm_igemm {

// ---- environment switches.  Read per call: the parity tests flip them inside one process.  One rule: a default-on switch is off iff its
// value begins with '0', a default-off switch is on iff its value begins with '1'.
struct GemmSwitches { bool stream1x1, split_bf16, h16, nn_h16, split_tn; };
constexpr GemmSwitches kDefaultSwitches = {true, false, true, true, true};
inline bool switch_on(const char* v, bool dflt) { return dflt ? !(v && v[0] == '0') : (v && v[0] == '1'); }
// kind (0 forward, 1 data gradient, 2 weight gradient) names the entry point: each reads the switches its plan can depend on, the others
// keep their defaults (three, one and two reads -- what the entry points read at most before)
inline GemmSwitches read_gemm_switches(int kind) {
  GemmSwitches s = kDefaultSwitches;
  if (kind == 0) {
    s.stream1x1 = switch_on(getenv("NBM_STREAM1X1"), true);
    s.split_bf16 = switch_on(getenv("NBM_SPLIT_BF16"), false);
    s.h16 = switch_on(getenv("NBM_H16"), true);
  } else if (kind == 1) {
    s.nn_h16 = switch_on(getenv("NBM_NN_H16"), true);
  } else {
    s.split_bf16 = switch_on(getenv("NBM_SPLIT_BF16"), false);
    s.split_tn = switch_on(getenv("NBM_SPLIT_TN"), true);
  }
  return s;
}

// ---- kernel ids: one per instantiation the entry points launch (name = the instantiation, as a profiler prints it)
#define NBM_GEMM_KERNELS(X)                                                                                                          \
  X(K_FWD_ROWS, "igemm_kernel<128,128,64,64,0,0,1,true>")            /* listed rows: single stage, 1x1 */                            \
  X(K_STREAM_64_256, "stream1x1_kernel<2,8,4,8>")                    /* stream1x1: 64 -> 256 with a residual */                      \
  X(K_STREAM_64_64, "stream1x1_kernel<2,2,2,8>")                     /* 64 -> 64, two workgroups per CU */                           \
  X(K_STREAM_256_64, "stream1x1_kernel<8,2,2,8>")                    /* 256 -> 64 */                                                 \
  X(K_STREAM_128_SLICED, "stream1x1_kernel<4,4,4,8>")                /* 128 -> 128 s (<= 1024) with a residual: s slices of 128 */   \
  X(K_STREAM_256_SLICED, "stream1x1_kernel<8,2,2,8>")                /* 256 -> 64 s (<= 2048) with a residual: s slices of 64 */     \
  X(K_FWD_SPLIT_R0, "igemm_split_kernel<0>")                         /* split-bf16, (2 nk) % 6 == 0 */                               \
  X(K_FWD_SPLIT_R2, "igemm_split_kernel<2>")                                                                                         \
  X(K_FWD_SPLIT_R4, "igemm_split_kernel<4>")                                                                                         \
  X(K_FWD_H16, "igemm_h16_kernel")                                   /* deep K, half-step LDS stages */                              \
  X(K_FWD_128_S1, "igemm_kernel<128,128,64,64,0,0,1,false>")         /* short K, single stage */                                     \
  X(K_FWD_128_FAST, "igemm_kernel<128,128,64,64,0,0,2,false>")       /* two stages */                                                \
  X(K_FWD_128_GENERIC, "igemm_kernel<128,128,64,64,1,0,2,false>")                                                                    \
  X(K_FWD_64_S1, "igemm_kernel<128,64,64,32,0,0,1,false>")                                                                           \
  X(K_FWD_64_FAST, "igemm_kernel<128,64,64,32,0,0,2,false>")                                                                         \
  X(K_FWD_64_GENERIC, "igemm_kernel<128,64,64,32,1,0,2,false>")                                                                      \
  X(K_FWD_32_FAST, "igemm_kernel<128,32,32,32,0,0,2,false>")                                                                         \
  X(K_FWD_32_GENERIC, "igemm_kernel<128,32,32,32,1,0,2,false>")                                                                      \
  X(K_NN_128_S1, "igemm_nn_kernel<128,1,false>")                                                                                     \
  X(K_NN_128_H16, "igemm_nn_kernel<128,2,true>")                                                                                     \
  X(K_NN_128, "igemm_nn_kernel<128,2,false>")                                                                                        \
  X(K_NN_64_S1, "igemm_nn_kernel<64,1,false>")                                                                                       \
  X(K_NN_64_H16, "igemm_nn_kernel<64,2,true>")                                                                                       \
  X(K_NN_64, "igemm_nn_kernel<64,2,false>")                                                                                          \
  X(K_TN_GENERIC, "igemm_tn_kernel<64,2,128>")                                                                                       \
  X(K_TN_128_SAME_M64, "igemm_tn_kernel<128,0,64>")                                                                                  \
  X(K_TN_128_STRIDED_M64, "igemm_tn_kernel<128,1,64>")                                                                               \
  X(K_TN_64_SAME_M64, "igemm_tn_kernel<64,0,64>")                                                                                    \
  X(K_TN_64_STRIDED_M64, "igemm_tn_kernel<64,1,64>")                                                                                 \
  X(K_TN_128_SAME, "igemm_tn_kernel<128,0,128>")                                                                                     \
  X(K_TN_128_STRIDED, "igemm_tn_kernel<128,1,128>")                                                                                  \
  X(K_TN_64_SAME, "igemm_tn_kernel<64,0,128>")                                                                                       \
  X(K_TN_64_STRIDED, "igemm_tn_kernel<64,1,128>")                                                                                    \
  X(K_SPLIT_TN_R0, "igemm_split_tn_kernel<0>")                       /* split-bf16 weight gradient, (k_chunk / 16) % 6 == 0 */       \
  X(K_SPLIT_TN_R2, "igemm_split_tn_kernel<2>")                                                                                       \
  X(K_SPLIT_TN_R4, "igemm_split_tn_kernel<4>")

enum GemmKernel {
#define X(id, name) id,
  NBM_GEMM_KERNELS(X)
#undef X
  K_COUNT
};
inline const char* gemm_kernel_name(int k) {
  static const char* const names[] = {
#define X(id, name) name,
      NBM_GEMM_KERNELS(X)
#undef X
  };
  return k >= 0 && k < K_COUNT ? names[k] : "";
}

// ---- the rules' numbers
constexpr int PLAN_BK = 32;                // floats per K-step
// Up to 8 K-steps (K <= 256: 1x1 convolutions whose time is output / residual traffic, not MFMA) a 128-wide tile runs on the single-stage
// kernel, three workgroups per CU; from 9 steps up on a deep-K form.
constexpr int SHORTK_STEPS = 8, DEEPK_STEPS = SHORTK_STEPS + 1;
// The 64-wide tile spends half the MFMA cycles per K-step of the 128-wide one, so its prologue / epilogue weigh double and the third
// workgroup pays up to K = 576 (layer1's 3x3 64 -> 64 @94x256: forward 1.075 -> 0.99 ms at B = 64, 2.05 -> 1.83 at B = 128; data gradient
// 2.39 -> 2.15 ms at B = 128; same K order, same bits).
constexpr int SHORTK_STEPS_64 = 20;
// Stride-2 data gradient (phased): a tile's K loop visits its parity class's taps only -- (N / 32) x {1, 2, 2, 4} steps for a 3x3; the
// largest class's step count decides (128 -> 128 @94x256, steps 4 / 8 / 8 / 16: 3.61 -> 3.46 ms at B = 128 on the single-stage kernel).
constexpr int SHORTK_STEPS_PHASED = 16;
constexpr int DEEPK_MAX_TAPS = 63;         // the deep-K forms (split-bf16, h16) hold a tap table: kh * kw < 63
constexpr int STREAM_MIN_ROWS = 8192;      // stream1x1: a persistent grid needs rows to stream
constexpr int SPLIT_TN_MIN_ROWS = 192;     // split-bf16 weight gradient: dW rows (N) from 192 up (256-row tiles)
constexpr long long ROWS_SPAN_MAX = 0x7fffffffll;    // listed rows: two image rows of x inside one 2 GB buffer resource
constexpr long long DGRAD_SPAN_MAX = 0x70000000ll;   // data gradient: the gather window of one 128-row tile (+ one image boundary), 2 GB resource
constexpr long long TN_SPAN_MAX = 0x40000000ll;      // weight gradient: 32 operand rows inside 1 GB

inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }

// The plan IS the C ABI's nbm_gemm_plan_t: everything a launch needs beyond the descriptor.
using GemmPlan = nbm_gemm_plan_t;

inline GemmPlan plan_error(int rc) {
  GemmPlan pl{};
  pl.rc = rc;
  pl.kernel = -1;
  pl.name = "";
  return pl;
}
inline void plan_kernel(GemmPlan& pl, int kernel, int gx, int gy, int gz, int block = 256) {
  pl.kernel = kernel;
  pl.name = gemm_kernel_name(kernel);
  pl.grid[0] = gx; pl.grid[1] = gy; pl.grid[2] = gz;
  pl.block = block;
}

// ------------------------------------------------------------------------------------------------ forward
inline GemmPlan plan_fwd(const nbm_gemm_desc& d, GemmSwitches sw) {
  if (!d.x || !d.w || !d.y) return plan_error(NBM_EINVAL);
  if (d.B <= 0 || d.H <= 0 || d.W <= 0 || d.Cin <= 0 || d.N <= 0 || d.kh <= 0 || d.kw <= 0 || d.stride <= 0 || d.Ho <= 0 || d.Wo <= 0 ||
      d.groups <= 0)
    return plan_error(NBM_EINVAL);
  // host-side shape check: the output geometry must be the one the gather assumes
  if ((d.H + 2 * d.pad - d.kh) / d.stride + 1 != d.Ho || (d.W + 2 * d.pad - d.kw) / d.stride + 1 != d.Wo) return plan_error(NBM_EINVAL);
  if (d.x_ld < d.Cin || d.y_ld < d.N || (d.residual && d.res_ld < d.N)) return plan_error(NBM_EINVAL);
  GemmPlan pl{};
  const int taps = d.kh * d.kw, K = taps * d.Cin, nk = (K + PLAN_BK - 1) / PLAN_BK;
  // An output width 64 past a multiple of 128 (the cell-domain data-gradient planes of the deferred lateral: 256 -> 448): the last 128-wide
  // tile would be half padding -- the first N - 64 channels on 128-wide tiles, the last 64 on the 64-wide kernel.  Every output element is the
  // same sum in the same order either way (round 5; weight-gradient twin: plan_wgrad).  The entry point runs the halves as two calls; this
  // plan is the first one's.
  if (d.N > 128 && (d.N & 127) == 64 && !d.rows && !d.up && !d.bits_out && !d.shift_per_row && (d.Cin % PLAN_BK) == 0 && K > SHORTK_STEPS * PLAN_BK) {
    nbm_gemm_desc a = d;
    a.N = d.N - 64;
    pl = plan_fwd(a, sw);
    pl.halves = 1;
    return pl;
  }
  if (d.w_ld < nk * PLAN_BK) return plan_error(NBM_EINVAL);  // every W row must hold nk*32 readable floats
  if (d.mask && (d.rows || d.groups != 1 || d.mask_ld < d.N)) return plan_error(NBM_EUNSUPPORTED);
  pl.vec_epi = ((d.N & 3) == 0 && (d.y_ld & 3) == 0 && (d.y_gs & 3) == 0 && aligned16(d.y) &&
                (!d.residual || ((d.res_ld & 3) == 0 && (d.res_gs & 3) == 0 && aligned16(d.residual))) &&
                (!d.scale || aligned16(d.scale)) && (!d.shift || d.shift_per_row || aligned16(d.shift)) &&
                (!d.mask || ((d.mask_ld & 3) == 0 && aligned16(d.mask))))
                   ? 1 : 0;
  if ((d.w_ld & 3) || (d.w_gs & 3) || !aligned16(d.w)) return plan_error(NBM_EALIGN);
  // (y > 0) bits: written by the vector epilogue, whole 32-channel words
  if (d.bits_out && (!pl.vec_epi || (d.N & 31) || d.groups != 1 || d.rows)) return plan_error(NBM_EUNSUPPORTED);
  if (d.up && (!pl.vec_epi || d.groups != 1 || d.up_H <= 0 || d.up_W <= 0 || !aligned16(d.up))) return plan_error(NBM_EUNSUPPORTED);
  pl.fast = ((d.Cin % PLAN_BK) == 0 && (d.x_ld & 3) == 0 && (d.x_gs & 3) == 0 && aligned16(d.x)) ? 1 : 0;
  const bool fast_vec = pl.fast && pl.vec_epi;
  const int M = d.B * d.Ho * d.Wo;
  pl.m_tiles = (M + 127) / 128;
  if (d.rows) {                  // listed rows: the short-K 1x1 variant only
    if (d.kh != 1 || d.kw != 1 || d.stride != 1 || d.pad != 0 || d.groups != 1 || !fast_vec || d.shift_per_row || nk > SHORTK_STEPS ||
        d.N <= 64 || (d.rows_mode != 1 && d.rows_mode != 2) || d.rows_count <= 0 || (d.rows_count % 128))
      return plan_error(NBM_EUNSUPPORTED);
    if (d.rows_mode == 2 && (d.rows_TH != (d.H + 1) / 2 || d.rows_TW != (d.W + 1) / 2)) return plan_error(NBM_EINVAL);
    if (2ll * d.H * d.W * d.x_ld * 4 > ROWS_SPAN_MAX) return plan_error(NBM_EUNSUPPORTED);
    pl.m_tiles = d.rows_count / 128;
    pl.n_tiles = (d.N + 127) / 128;
    // with a device-side block count the grid is rounded up to whole XCD rounds of M tiles
    plan_kernel(pl, K_FWD_ROWS, (d.rows_blocks ? (pl.m_tiles + 7) / 8 * 8 : pl.m_tiles) * pl.n_tiles, 1, 1);
    return pl;
  }
  // streaming form for 1x1 / stride 1 layers whose weights fit LDS (see stream1x1_kernel)
  if (sw.stream1x1 && d.kh == 1 && d.kw == 1 && d.stride == 1 && d.pad == 0 && d.groups == 1 && fast_vec && !d.up && !d.mask &&
      !d.shift_per_row && (d.N % 32) == 0 && M >= STREAM_MIN_ROWS) {
    const int k32 = d.Cin / 32, nt = d.N / 32;
    int kernel = -1, wg_per_cu = 1, slices = 1;
    // 64 -> 256 without a residual is write-bound and gains nothing (0.78 ms either way at B = 64): tiled kernel
    if (k32 == 2 && nt == 8 && d.residual) kernel = K_STREAM_64_256;
    else if (k32 == 2 && nt == 2) kernel = K_STREAM_64_64, wg_per_cu = 2;
    else if (k32 == 8 && nt == 2) kernel = K_STREAM_256_64;
    // wider layers in slices of N
    else if (d.residual && k32 == 4 && nt % 4 == 0 && nt <= 32) kernel = K_STREAM_128_SLICED, slices = nt / 4;      // 128 -> 512: 4 slices of 128
    else if (d.residual && k32 == 8 && nt % 2 == 0 && nt <= 64) kernel = K_STREAM_256_SLICED, slices = nt / 2;      // 256 -> 1024: 16 slices of 64
    if (kernel >= 0) {
      const int waves = 8;
      pl.m_tiles = (M + 31) / 32;                       // 32-row tiles, one per wave
      pl.slices = slices;
      const int wgs = (pl.m_tiles + waves - 1) / waves;
      int gx = 256 * wg_per_cu / slices;                // the persistent grid is shared by the slices
      if (gx < 1) gx = 1;
      plan_kernel(pl, kernel, wgs < gx ? wgs : gx, slices, 1, waves * 64);
      return pl;
    }
  }
  if (d.N > 64) {
    pl.n_tiles = (d.N + 127) / 128;
    const bool deep = fast_vec && nk >= DEEPK_STEPS && taps < DEEPK_MAX_TAPS;
    // deep K on the bf16 matrix pipe through split fp32 operands (igemm_split.hip, 256 x 128 tiles); default: the fp32 instruction.
    // The choice depends on the LAYER (K, N), never on the number of rows: a clip's result must not depend on how many clips share its
    // batch (the two kernels sum in different orders).
    if (sw.split_bf16 && deep) {
      pl.m_tiles = (M + 255) / 256;
      const int rem = (2 * nk) % 6;
      plan_kernel(pl, rem == 0 ? K_FWD_SPLIT_R0 : rem == 2 ? K_FWD_SPLIT_R2 : K_FWD_SPLIT_R4, pl.m_tiles * pl.n_tiles, 1, d.groups);
    }
    // deep K: half-step LDS stages, three workgroups per CU (igemm_h16.hip: the same products in the same order as the two-stage kernel,
    // 2-14 % faster launch by launch at B = 64, scripts/h16_probe.py).  NBM_H16 = 0: the two-stage kernel.
    else if (sw.h16 && deep) plan_kernel(pl, K_FWD_H16, pl.m_tiles * pl.n_tiles, 1, d.groups);
    // short K and a 16-byte epilogue: the three-workgroups-per-CU variant (see the kernel template's comment)
    else if (fast_vec && nk <= SHORTK_STEPS) plan_kernel(pl, K_FWD_128_S1, pl.m_tiles * pl.n_tiles, 1, d.groups);
    else plan_kernel(pl, pl.fast ? K_FWD_128_FAST : K_FWD_128_GENERIC, pl.m_tiles * pl.n_tiles, 1, d.groups);
  } else if (d.N > 32) {
    pl.n_tiles = 1;
    // (NEGATIVE, round 5: 256 x 64 tiles with a 64 x 64 patch per wave -- the fragment reuse of the 128 x 128 kernel -- on the layer1 3x3
    // 64 -> 64 @94x256: two LDS stages / one workgroup per CU 1.30 ms against 1.14 at B = 64, one stage / two workgroups per CU 1.15:
    // the 64-wide tile's time is not its LDS reads per MFMA)
    if (fast_vec && nk <= SHORTK_STEPS_64) plan_kernel(pl, K_FWD_64_S1, pl.m_tiles, 1, d.groups);
    else plan_kernel(pl, pl.fast ? K_FWD_64_FAST : K_FWD_64_GENERIC, pl.m_tiles, 1, d.groups);
  } else {
    pl.n_tiles = 1;
    plan_kernel(pl, pl.fast ? K_FWD_32_FAST : K_FWD_32_GENERIC, pl.m_tiles, 1, d.groups);
  }
  return pl;
}

// ------------------------------------------------------------------------------------------------ backward
inline int check_bwd_common(const nbm_bwd_desc& d) {
  if (!d.g || !d.out) return NBM_EINVAL;
  if (d.B <= 0 || d.H <= 0 || d.W <= 0 || d.Cin <= 0 || d.N <= 0 || d.kh <= 0 || d.kw <= 0 || d.stride <= 0 || d.groups <= 0 ||
      d.kh * d.kw > 64)
    return NBM_EINVAL;
  if ((d.H + 2 * d.pad - d.kh) / d.stride + 1 != d.Ho || (d.W + 2 * d.pad - d.kw) / d.stride + 1 != d.Wo) return NBM_EINVAL;
  return NBM_OK;
}

inline GemmPlan plan_dgrad(const nbm_bwd_desc& d, GemmSwitches sw) {
  if (int rc = check_bwd_common(d)) return plan_error(rc);
  if (!d.w) return plan_error(NBM_EINVAL);
  // G rows must hold ceil(N/32)*32 readable floats (zero padded), 16-byte aligned; W rows are read along c
  if ((d.g_ld & 3) || d.g_ld < ((d.N + 31) / 32) * 32 || (d.Cin & 3) || (d.w_ld & 3) || (d.g_gs & 3) || (d.w_gs & 3) || !aligned16(d.g) ||
      !aligned16(d.w) || (d.a_scale && !aligned16(d.a_scale)))
    return plan_error(NBM_EALIGN);
  if (d.out_ld < d.Cin || (d.residual && d.res_ld < d.Cin) || (d.mask && d.mask_ld < d.Cin)) return plan_error(NBM_EINVAL);
  if (d.residual2 && (d.stride != 1 || d.groups != 1 || d.res2_ld < d.Cin)) return plan_error(NBM_EINVAL);
  if (d.a_scale && (d.N & 31)) return plan_error(NBM_EINVAL);
  // the ReLU mask as bits: whole 32-channel words, one group
  if (d.mask_bits && ((d.Cin & 31) || d.groups != 1)) return plan_error(NBM_EUNSUPPORTED);
  // the gather window of one 128-row tile (+ one image boundary) must stay inside the 2 GB buffer resource
  {
    const long long row = (long long)d.Wo * d.g_ld * 4;                    // bytes per G image row
    const long long span = (d.W == 1 && d.kh == 1) ? 130ll * d.g_ld * 4     // plain GEMM: 128 consecutive rows
                                                    : (d.kh + 130) * row + (long long)d.Ho * row;
    if (span > DGRAD_SPAN_MAX) return plan_error(NBM_EUNSUPPORTED);
  }
  GemmPlan pl{};
  pl.vec_epi = ((d.out_ld & 3) == 0 && (d.out_gs & 3) == 0 && aligned16(d.out) &&
                (!d.residual || ((d.res_ld & 3) == 0 && (d.res_gs & 3) == 0 && aligned16(d.residual))) &&
                (!d.mask || ((d.mask_ld & 3) == 0 && aligned16(d.mask))) &&
                (!d.residual2 || ((d.res2_ld & 3) == 0 && aligned16(d.residual2)))) ? 1 : 0;
  pl.m_tiles = (d.B * d.H * d.W + 127) / 128;
  if (d.stride == 2) {                  // group the M tiles by parity class (see igemm_nn_kernel)
    pl.phased = 1;
    int tmax = 0;
    for (int ph = 0; ph < 4; ++ph) {
      const int y0 = ((ph >> 1) + d.pad) & 1, x0 = ((ph & 1) + d.pad) & 1;
      const int Hp = (d.H - y0 + 1) >> 1, Wp = (d.W - x0 + 1) >> 1;
      pl.ph_tiles[ph] = (int)(((long long)d.B * Hp * Wp + 127) / 128);
      if (pl.ph_tiles[ph] > tmax) tmax = pl.ph_tiles[ph];
    }
    pl.m_tiles = 4 * tmax;
  }
  // short K and a 16-byte epilogue: the three-workgroups-per-CU variant (see the kernel template's comment)
  const int n_steps = (d.N + PLAN_BK - 1) / PLAN_BK;
  const int ph_max = n_steps * ((d.kh + 1) / 2) * ((d.kw + 1) / 2);
  const bool shortk = pl.vec_epi && (pl.phased ? ph_max <= SHORTK_STEPS_PHASED
                                               : n_steps * d.kh * d.kw <= (d.Cin <= 64 ? SHORTK_STEPS_64 : SHORTK_STEPS));
  // deep K: the half-step form of the two-stage kernel (three workgroups per CU, same bits; NBM_NN_H16=0: the two-stage kernel)
  const bool hs = sw.nn_h16 && pl.vec_epi;
  const bool wide = d.Cin > 64;
  pl.n_tiles = wide ? (d.Cin + 127) / 128 : 1;
  plan_kernel(pl, wide ? (shortk ? K_NN_128_S1 : hs ? K_NN_128_H16 : K_NN_128) : (shortk ? K_NN_64_S1 : hs ? K_NN_64_H16 : K_NN_64),
              pl.m_tiles * pl.n_tiles, 1, d.groups);
  return pl;
}

// Split count of the weight gradient's pixel reduction, so that the grid fills the chip in WHOLE rounds: `slots` workgroups are resident at
// once, all of equal length, so a grid of 4.01 rounds costs 5 (the old ">= 2048 workgroups" rule hit exactly that on the largest layer:
// 54 tiles x 38 splits = 2052).  The split count with the best fill of its last round among those with >= rows_per_split_min pixels per
// split and <= 16 rounds; ties go to fewer splits (fewer atomics).
inline int best_split(int M, int tiles, int slots, int rows_per_split_min) {
  const int max_splits = (M + rows_per_split_min - 1) / rows_per_split_min;
  int splits = 1;
  double best = -1.0;
  for (int sp = 1; sp <= max_splits && (long long)sp * tiles <= 16ll * slots; ++sp) {
    const long long wg = (long long)sp * tiles;
    const long long rounds = (wg + slots - 1) / slots;
    const double fill = (double)wg / (double)(rounds * slots);
    if (fill > best + 0.005) { best = fill; splits = sp; }
  }
  return splits;
}
// pixels per split (a multiple of the K-step) and the split count that covers M with it
inline void plan_splits(GemmPlan& pl, int M, int tiles, int slots, int rows_per_split_min) {
  const int sp = best_split(M, tiles, slots, rows_per_split_min);
  pl.k_chunk = (((M + sp - 1) / sp) + PLAN_BK - 1) / PLAN_BK * PLAN_BK;
  pl.splits = (M + pl.k_chunk - 1) / pl.k_chunk;
}

// Deterministic twin of the weight gradient (nbm_bwd_desc.workspace): floats of one split's slice -- the dW rows of every
// group, then the bias partials where a bias gradient rides -- and the ceiling on the whole workspace.  A plan
// whose slices would exceed it gets fewer, longer splits (k_chunk grows to cover M with them): the grid then fills fewer of the chip's
// rounds, which is the price.  best_split allows at most 16 rounds of 512 tiles of at most 128 x 128 floats, so the slices of one launch
// never need more than 512 MB: the ceiling does not bind for any plan best_split makes and guards the arithmetic; one slice beyond it is
// refused (NBM_EUNSUPPORTED).
constexpr long long WGRAD_WS_MAX_BYTES = 1ll << 30;
// (rows at their own pitch, taps * Cin rounded up to 4 floats -- not at out_ld: `out` may be a column slice of a much wider matrix, as the
// attention's dV' / dK inside the [M][3 d] gradient of the fused projection, one group per image)
inline int wgrad_slice_ld(const nbm_bwd_desc& d) { return (d.kh * d.kw * d.Cin + 3) / 4 * 4; }
inline long long wgrad_slice_floats(const nbm_bwd_desc& d) {
  return (long long)d.groups * d.N * wgrad_slice_ld(d) + (d.bias_grad ? ((long long)d.groups * d.N + 3) / 4 * 4 : 0);
}

// det: plan for the deterministic twin (what nbm_conv_wgrad does when d.workspace is set)
inline GemmPlan plan_wgrad(const nbm_bwd_desc& d, GemmSwitches sw, bool det) {
  if (int rc = check_bwd_common(d)) return plan_error(rc);
  if (!d.x) return plan_error(NBM_EINVAL);
  if ((d.g_ld & 3) || (d.g_gs & 3) || !aligned16(d.g) || d.g_ld < ((d.N + 3) / 4) * 4) return plan_error(NBM_EALIGN);
  GemmPlan pl{};
  pl.b_generic = ((d.Cin & 3) || (d.x_ld & 3) || (d.x_gs & 3) || !aligned16(d.x)) ? 1 : 0;
  const int taps = d.kh * d.kw;
  if (d.out_ld < taps * d.Cin) return plan_error(NBM_EINVAL);
  pl.plain = (taps == 1 && d.stride == 1 && d.pad == 0) ? 1 : 0;
  // Plain GEMMs whose column count is 64 past a multiple of 128 (the cell-domain planes of the deferred lateral: [T][256]^T x [T][448]): the
  // 128-wide tiles would multiply 64 columns of padding in the last tile (1 / 8 of the MFMA work of 448 columns: 110 against 122 TF/s for
  // the 384-column twin, round 5) -- the first Cin - 64 columns on 128-wide tiles, the last 64 on the 64-wide kernel.  Same sums per element
  // (the split over the pixels is chosen per launch; the atomics make the order free anyway).  The entry point runs the halves as two calls;
  // this plan is the first one's.
  if (pl.plain && !pl.b_generic && d.Cin > 128 && (d.Cin & 127) == 64) {
    nbm_bwd_desc a = d;
    a.Cin = d.Cin - 64;
    pl = plan_wgrad(a, sw, det);
    pl.halves = 1;
    return pl;
  }
  const int M = d.B * d.Ho * d.Wo;
  // opt-in (NBM_SPLIT_BF16=1): plain weight-gradient GEMMs (1x1 convolutions, nn.Linear, the grouped Winograd- / cell-domain
  // products) with >= 192 rows and > 64 columns on the bf16 matrix pipe through split fp32 operands (igemm_split_tn.hip: 256 x 128 tiles).
  // Chosen by the LAYER, never by the number of pixels.  The bias gradient is not produced there (the caller sums the columns of G).
  if (!det && sw.split_bf16 && sw.split_tn && pl.plain && !pl.b_generic && !d.bias_grad && d.N >= SPLIT_TN_MIN_ROWS && d.Cin > 64 && d.out_ld >= d.Cin &&
      32ll * d.g_ld * 4 < TN_SPAN_MAX && 32ll * d.x_ld * 4 < TN_SPAN_MAX) {
    pl.m_tiles = (d.N + 255) / 256;
    pl.n_tiles = (d.Cin + 127) / 128;
    // 256 slots: one workgroup per CU; >= 32 K16 stages per split
    plan_splits(pl, M, pl.m_tiles * pl.n_tiles * d.groups, 256, 16 * 32);
    const int rem = (pl.k_chunk >> 4) % 6;
    plan_kernel(pl, rem == 0 ? K_SPLIT_TN_R0 : rem == 2 ? K_SPLIT_TN_R2 : K_SPLIT_TN_R4, pl.m_tiles * pl.n_tiles, pl.splits, d.groups);
    return pl;
  }
  pl.narrow_m = (d.N <= 64 && !pl.b_generic) ? 1 : 0;            // 64-row dW tiles: no MFMA spent on the zero half of a 128-row G tile
  pl.m_tiles = pl.narrow_m ? 1 : (d.N + 127) / 128;
  const bool wide = !pl.b_generic && d.Cin > 64;
  const int BN = wide ? 128 : 64;
  pl.n_tiles = pl.b_generic ? (taps * d.Cin + BN - 1) / BN : taps * ((d.Cin + BN - 1) / BN);
  // 512 slots = 256 CUs x the two workgroups of the 128 x 128 instantiation; >= 8 K-steps per split.  (The narrower instantiations hold 3
  // or 4 workgroups per CU; sizing the rounds for 768 / 1024 was measured in round 5 and changes nothing -- 2.161 vs 2.155 ms on layer1's
  // 3x3: a CU with fewer workgroups left runs them faster, the matrix pipe is what they share -- scripts/wgrad_cycles.py, in the git history)
  plan_splits(pl, M, pl.m_tiles * pl.n_tiles * d.groups, 512, 8 * PLAN_BK);
  if (det) {
    const long long max_splits = WGRAD_WS_MAX_BYTES / (wgrad_slice_floats(d) * 4);
    // one slice beyond the ceiling (a dW of more than 2^28 floats at its pitch): refused, never run on the default kernels instead
    if (max_splits < 1) return plan_error(NBM_EUNSUPPORTED);
    if (pl.splits > max_splits) {
      const long long sp = max_splits;
      pl.k_chunk = (int)(((M + sp - 1) / sp + PLAN_BK - 1) / PLAN_BK * PLAN_BK);
      pl.splits = (M + pl.k_chunk - 1) / pl.k_chunk;
    }
  }
  const bool same = !pl.b_generic && d.stride == 1 && d.Ho == d.H && d.Wo == d.W && (d.Wo >= PLAN_BK || pl.plain) &&
                    (long long)PLAN_BK * d.x_ld * 4 < TN_SPAN_MAX;
  const int kernel = pl.b_generic ? K_TN_GENERIC
                     : pl.narrow_m ? (wide ? (same ? K_TN_128_SAME_M64 : K_TN_128_STRIDED_M64) : (same ? K_TN_64_SAME_M64 : K_TN_64_STRIDED_M64))
                                   : (wide ? (same ? K_TN_128_SAME : K_TN_128_STRIDED) : (same ? K_TN_64_SAME : K_TN_64_STRIDED));
  plan_kernel(pl, kernel, pl.m_tiles * pl.n_tiles, pl.splits, d.groups);
  return pl;
}
inline GemmPlan plan_wgrad(const nbm_bwd_desc& d, GemmSwitches sw) { return plan_wgrad(d, sw, d.workspace != nullptr); }

// Bytes of the twin's workspace: splits x slice; 0 when one split sums every element and no bias gradient rides (the default kernel then
// adds exactly one value per element, which no order can change).  Both calls of a `halves` plan use the same workspace in turn.
inline long long wgrad_workspace_bytes(const nbm_bwd_desc& d, GemmSwitches sw, int* rc) {
  const GemmPlan pl = plan_wgrad(d, sw, true);
  *rc = pl.rc;
  if (pl.rc) return 0;
  if (pl.halves) {
    nbm_bwd_desc a = d, b = d;
    a.Cin = d.Cin - 64;
    b.Cin = 64; b.x = d.x + (d.Cin - 64); b.out = d.out + (d.Cin - 64); b.bias_grad = nullptr;
    // (both calls get the caller's one stride, the slice of the whole descriptor: the larger split count times that)
    const GemmPlan pa = plan_wgrad(a, sw, true), pb = plan_wgrad(b, sw, true);
    *rc = pa.rc ? pa.rc : pb.rc;
    if (*rc) return 0;
    const int na = (pa.splits <= 1 && !a.bias_grad) ? 0 : pa.splits, nb = pb.splits <= 1 ? 0 : pb.splits;
    return (long long)(na > nb ? na : nb) * wgrad_slice_floats(d) * 4;
  }
  if (pl.splits <= 1 && !d.bias_grad) return 0;
  return (long long)pl.splits * wgrad_slice_floats(d) * 4;
}

}  // namespace nbm_igemm
