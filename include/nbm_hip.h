/* nbm_hip.h — C ABI of the MI355X-native NBM hot path (libnbm_hip.so).
 *
 * The reference (LouisBearing/BirdSoundClassif) is 100 % Python: it has no FFI layer, its "native"
 * boundary is torch's own CPU/CUDA operators.  Every entry point below replaces the torch / numpy /
 * librosa operator call(s) named in its comment (reference file:line, relative to /root/reference).
 * The host side (birdsoundclassif_amd/ops.py) binds them with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless the name ends in _host; no ownership transfer,
 *     the caller allocates outputs and workspaces;
 *   - activations are NHWC fp32 ("pixel pitch" = *_ld floats between consecutive pixels);
 *   - `stream` is a hipStream_t passed as void*; all functions are asynchronous on it, re-entrant,
 *     and keep no global state;
 *   - return value: 0 = success, otherwise a negative NBM_E* code (bad argument) or a positive
 *     hipError_t from the launch.
 */
#ifndef NBM_HIP_H
#define NBM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NBM_OK 0
#define NBM_EINVAL (-1)
#define NBM_EALIGN (-2)
#define NBM_EUNSUPPORTED (-3)

#define NBM_ACT_NONE 0
#define NBM_ACT_RELU 1
#define NBM_ACT_SILU 2
#define NBM_ACT_LEAKY 3 /* LeakyReLU, negative slope 0.01 (nn.LeakyReLU default) */

const char* nbm_version(void);

/* Census of a captured graph (a `hipGraph_t`, e.g. torch.cuda.CUDAGraph(keep_graph=True).raw_cuda_graph()): counts[0..5] = kernel,
 * memcpy, memset, host, empty (fork / join), other nodes.  No counterpart in the reference (nbm_detect.py:23-28 runs one eager model
 * call per file); it is the fence of the captured bulk loop (bulk.GraphedDetector): the HIP runtime torch 2.10+rocm7.0 bundles
 * (7.0.51831) loses MEMSET nodes of a graph exec from its second launch on (scripts/graph_pair_repro.hip), so a step is
 * only replayed when its graph holds kernel (and empty) nodes alone.  This library itself never creates memset nodes. */
int nbm_graph_census(void* graph, long long counts[6]);

/* ------------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution / batched GEMM on the fp32 MFMA (v_mfma_f32_32x32x2_f32).
 *
 *   y[g][m][n] = act( alpha * sum_k A[g][m][k] * W[g][n][k] * scale[n] + shift[n|m] + residual[g][m][n] )
 *
 *   A is the im2col view of x (NHWC): m = (b, oy, ox), k = (r, s, c) -> x[b][oy*stride-pad+r][ox*stride-pad+s][c]
 *   (zero outside the image).  W is [N][w_ld] with k contiguous (KRSC weights).  A plain GEMM is the
 *   case H = M, W = 1, kh = kw = 1.  `groups` (blockIdx.z) strides x / w / y / residual by *_gs floats
 *   (attention: one GEMM per clip; 0 = operand shared by all groups).
 *
 * Replaces: F.conv2d / nn.Linear / torch.matmul call sites of the detector forward
 *   backbone.py:104-113 (+ torchvision ResNet-50 convs), self_attention.py:43-49, fpn.py:132-146,
 *   layers.py:25-46,79-99,574-579; FrozenBatchNorm2d affine (backbone.py:52-62), bias, ReLU/SiLU and
 *   the residual add are fused in the epilogue.
 */
typedef struct nbm_gemm_desc {
  const float* x;        /* A source, NHWC [B][H][W][Cin] with pixel pitch x_ld            */
  const float* w;        /* [N][w_ld], K = kh*kw*Cin valid columns (rest must be finite)   */
  float* y;              /* [M][y_ld] (NHWC output, N valid channels)                      */
  const float* scale;    /* [N] or NULL                                                    */
  const float* shift;    /* [N] (or [M] when shift_per_row) or NULL                        */
  const float* residual; /* [M][res_ld] or NULL                                            */
  int64_t x_gs, w_gs, y_gs, res_gs; /* per-group strides in floats                        */
  int groups;
  int B, H, W, Cin;      /* input geometry                                                 */
  int N;                 /* output channels                                                */
  int kh, kw, stride, pad;
  int Ho, Wo;            /* output geometry; M = B*Ho*Wo                                   */
  int x_ld, w_ld, y_ld, res_ld;
  float alpha;
  int act;               /* NBM_ACT_*                                                      */
  int shift_per_row;     /* 1: shift is indexed by m (row) instead of n                    */
  const float* up;       /* optional [B][up_H][up_W][N]: y += bilinear_align_corners(up -> Ho x Wo), added after
                            shift/residual and before act -- the FPN top-down merge fused into the lateral 1x1
                            (fpn.py:143-144); needs the 16-byte epilogue (N % 4 == 0, aligned) and groups == 1  */
  int up_H, up_W;
  /* Listed rows (optional; 1x1 / stride 1 / pad 0, one group, Cin % 32 == 0, Cin <= 256, N > 64, 16-byte epilogue): the GEMM
   * runs over rows_count (% 128 == 0) listed pixels of the dense maps instead of all B*H*W of them; x, y, residual and `up`
   * keep their dense addressing, pixels that are not listed are neither read nor written.  Used for the lateral 1x1 +
   * top-down merge that feeds a demand-driven FPN output convolution (nbm_wino23_conv_fused_tiles).
   *   rows_mode 1: rows[m] = pixel index b*H*W + y*W + x, ascending, -1 = none (only at the end of the list);
   *   rows_mode 2: rows[m / 16] = linear 2x2-tile id b*TH*TW + ty*TW + tx (-1 = none), row m = pixel m % 16 of that tile's
   *                4x4 input patch (the list nbm_roi_tiles builds; rows_count = 16 x its entries);
   *   rows_blocks: optional device scalar, number of leading 128-entry blocks of `rows` that are filled. */
  const int* rows;
  const int* rows_blocks;
  int rows_mode, rows_count, rows_TH, rows_TW;
  /* Optional producer mask [M][mask_ld] (not with `rows`): y is zeroed where mask <= 0, after everything else -- the ReLU of the layer
   * whose data gradient this launch computes (what autograd derives for reference train.py:212 through torchvision's Bottleneck): with
   * the transposed, BatchNorm-scaled weights as `w` and the incoming gradient as `x`, a 1x1 data gradient IS this forward GEMM, which
   * lets it take the split-bf16 form below (NBM_SPLIT_BF16=1; ops.conv_dgrad routes it).  One group; the 16-byte epilogue needs it
   * 16-byte aligned with mask_ld % 4 == 0 (otherwise the scalar epilogue runs). */
  const float* mask;
  int mask_ld;
  /* Optional (round 5): one BIT per output element, (stored y > 0), 32 channels per word -- bits_out[m * (N / 32) + n / 32], bit
   * 8 (n % 4) + (n % 32) / 4 (the four comparison masks of a 16-byte lane group side by side: no bit shuffling in the epilogue) --
   * written by the same epilogue (vector epilogue, N % 32 == 0, one group, not with `rows`; otherwise NBM_EUNSUPPORTED).  The ReLU mask of
   * the consumer's data gradient (nbm_bwd_desc.mask_bits) at 1/32 of the bytes of re-reading y. */
  unsigned* bits_out;
} nbm_gemm_desc;

/* Environment switch, read on every call: NBM_SPLIT_BF16=1 runs the deep-K launches (K = kh*kw*Cin > 256, N > 64, Cin % 32 == 0,
 * 16-byte epilogue; chosen by the LAYER, never by the number of rows) on the bf16 matrix pipe with each fp32 operand split into three
 * bf16 terms and six products accumulated in fp32 (csrc/igemm_split.hip): same interface, fp32-accurate results in another
 * summation order.  Default: the fp32 matrix instruction. */
int nbm_gemm_conv(const nbm_gemm_desc* d, void* stream);

/* Grouped 3x3 convolution on the fp32 matrix instruction v_mfma_f32_16x16x4_f32 (csrc/gconv.hip), NHWC fp32:
 *
 *   y[b][oy][ox][g*Cg + n] = relu?( scale[.] * sum_{r,s,c} x[b][oy*stride-1+r][ox*stride-1+s][g*Cg + c] * W[g*Cg + n][c][r][s] + shift[.] )
 *
 * 3x3, pad 1, dilation 1, stride 1 or 2, zeros outside the image; `groups` groups of Cg input = Cg output channels, Cg in
 * {4, 8, 16, 32, 64}, C = groups * Cg a multiple of 64.  scale / shift [C] are optional (the folded FrozenBatchNorm2d).
 * w is the PREPARED weight, C * 9 * max(Cg, 16) floats in the kernel's fragment order (`_prep.gconv` of the host layer):
 *   w[t][tap = 3 r + s][j][lane][e] = W[n][ci][r][s]  when input channel ci and output channel n lie in the same group, else 0,
 *   n = 16 t + (lane & 15), ci = (16 t / CI) * CI + 16 j + 4 (lane >> 4) + e, CI = max(Cg, 16), j < CI / 16, lane < 64, e < 4.
 * Anything else -- another Cg, kernel size, padding or stride, C % 64 != 0, a pointer that is not 16-byte aligned or a pitch that is no
 * multiple of 4 -- returns NBM_EUNSUPPORTED and launches nothing: there is no slow path.  Allocates nothing, clears nothing.
 *
 * Replaces: the grouped `conv2` (+ bn2 + ReLU) of torchvision's ResNeXt Bottleneck, which the reference reaches through
 *   backbone.py:131 `getattr(torchvision.models, name)` with name = resnext50_32x4d / resnext101_32x8d / resnext101_64x4d. */
typedef struct nbm_gconv_desc {
  const float* x;      /* [B][H][W] pixels of x_ld floats, C valid channels    */
  const float* w;      /* prepared weights, see above                          */
  float* y;            /* [B][Ho][Wo] pixels of y_ld floats, C valid channels  */
  const float* scale;  /* [C] or NULL                                          */
  const float* shift;  /* [C] or NULL                                          */
  int B, H, W;
  int groups, Cg;
  int kh, kw, stride, pad;
  int Ho, Wo;          /* (H - 1) / stride + 1, (W - 1) / stride + 1           */
  int x_ld, y_ld;
  int relu;
} nbm_gconv_desc;
int nbm_gconv3x3(const nbm_gconv_desc* d, void* stream);

/* Gradients of nbm_gconv3x3 followed by the folded FrozenBatchNorm2d + ReLU, y = relu(scale * gconv(x, W) + shift) (csrc/gconv_bwd.hip;
 * same geometry: 3x3, pad 1, stride 1 or 2, NHWC fp32, Cg in {4, 8, 16, 32, 64}, C = groups * Cg a multiple of 64, pitched pixels).
 * g = dL/dy [B][Ho][Wo][C]; both kernels use dz = g * (y > 0), the mask applied while the operand is staged (y optional: without it
 * g is used as it is), and scale[n] enters through the prepared weights (data gradient) or the reduction (weight gradient).
 *
 * nbm_gconv3x3_dgrad:  out = gx [B][H][W] pixels of out_ld floats,
 *   gx[b][iy][ix][g*Cg + c] = sum over n < Cg and the taps (r, s) with (iy + 1 - r) and (ix + 1 - s) divisible by stride of
 *                             dz[b][(iy+1-r)/stride][(ix+1-s)/stride][g*Cg + n] * scale[g*Cg + n] * W[g*Cg + n][c][r][s]
 *   (positions outside [0,Ho) x [0,Wo) count as zero; H and W are given because at stride 2 Ho does not determine H).  w is the
 *   PREPARED weight `_prep.gconv_dgrad(weight, groups, scale)`: the fragments (layout of nbm_gconv3x3) of
 *   W'[g*Cg + c][n][r][s] = scale[g*Cg + n] * W[g*Cg + n][c][2-r][2-s].  x, scale, workspace, accumulate and splits are not read.
 *
 * nbm_gconv3x3_wgrad:  out = dW [C][Cg][3][3], the parameter's own layout (C rows of 9 Cg floats, 4-byte aligned),
 *   dW[g*Cg + n][c][r][s] (+)= scale[g*Cg + n] * sum over b, oy, ox of dz[b][oy][ox][g*Cg + n] * x[b][oy*stride-1+r][ox*stride-1+s][g*Cg + c]
 *   (`accumulate`: added to what is there; scale optional).  The sum over the pixels is split over `splits` workgroups per 64 channels
 *   (0: the library's choice, 1 .. 4096: as given); every split stores its partial fragments to `workspace` (at least the bytes
 *   nbm_gconv3x3_wgrad_workspace returns for the same descriptor, 16-byte aligned; its previous contents are not read) and a second
 *   kernel sums them in ascending order and is the only writer of dW: no atomics, the same bits every run.  w is not read.
 *
 * nbm_gconv3x3_wgrad_workspace: host only, no HIP call; *bytes = splits * C * 9 * max(Cg, 16) * 4 with the split count the launch
 *   will use (pointers of the descriptor are not looked at).
 *
 * Anything outside the geometry, a pointer that is not 16-byte aligned or a pitch that is no multiple of 4 returns NBM_EUNSUPPORTED and
 * launches nothing: there is no slow path.  Nothing is allocated inside.
 *
 * Replaces: what autograd derives for reference train.py:212 `losses.backward()` through the grouped `conv2` + bn2 + ReLU of
 *   torchvision's ResNeXt Bottleneck (backbone.py:131 `getattr(torchvision.models, name)`): d/d(input) and d/d(conv2.weight). */
typedef struct nbm_gconv_bwd_desc {
  const float* g;        /* dL/dy, [B][Ho][Wo] pixels of g_ld floats                        */
  const float* y;        /* forward output (ReLU mask), pixels of y_ld floats, or NULL      */
  const float* w;        /* dgrad: prepared weights, see above                              */
  const float* x;        /* wgrad: forward input, [B][H][W] pixels of x_ld floats           */
  float* out;            /* dgrad: gx, pixels of out_ld floats; wgrad: dW [C][Cg*9]         */
  const float* scale;    /* wgrad: [C] or NULL                                              */
  void* workspace;       /* wgrad: partial fragments of the splits                          */
  long long workspace_bytes;
  int B, H, W;
  int groups, Cg;
  int kh, kw, stride, pad;
  int Ho, Wo;            /* (H - 1) / stride + 1, (W - 1) / stride + 1                      */
  int g_ld, y_ld, x_ld, out_ld;
  int accumulate;        /* wgrad: dW += instead of dW =                                    */
  int splits;            /* wgrad: 0 = the library's choice                                 */
} nbm_gconv_bwd_desc;
int nbm_gconv3x3_dgrad(const nbm_gconv_bwd_desc* d, void* stream);
int nbm_gconv3x3_wgrad(const nbm_gconv_bwd_desc* d, void* stream);
int nbm_gconv3x3_wgrad_workspace(const nbm_gconv_bwd_desc* d, long long* bytes);

/* Winograd transforms for 3x3 / stride 1 / pad 1 convolutions (the FPN output convolutions, fpn.py:137,145, and their data /
 * weight gradients).  m = 2: F(2x2,3x3), 16 transformed planes, used by the forward pass (error ~3e-6, proposals stay
 * bit-identical to the reference); m = 4: F(4x4,3x3) with interpolation points {0, 1, -1, 1/2, -2, inf}, 36 planes, used by
 * the two backward convolutions only (error ~2e-5).  V[xi][t][c] = (B^T d B)[xi] of the (m+2)x(m+2) input patch of tile t
 * (zero padded); the (m+2)^2 GEMMs M[xi] = V[xi] x U[xi]^T run through nbm_gemm_conv with groups = (m+2)^2;
 * y = act((A^T M A) * scale + shift), zeroed where mask <= 0 (scale / shift / mask may be NULL: FrozenBN + ReLU of the ResNet
 * 3x3 layers, the producer's ReLU mask of a data gradient).  T = B*ceil(H/m)*ceil(W/m) tiles; V: [(m+2)^2][T][C], M: [(m+2)^2][T][N].
 * residual [B][H][W][N] (optional, m = 4 only): added after the epilogue -- the gradient that another consumer of the same
 * tensor has already produced (what autograd would otherwise add in a pass of its own). */
int nbm_wino_input(const float* x, int B, int H, int W, int C, float* V, int m, void* stream);
int nbm_wino_output(const float* M, const float* scale, const float* shift, const float* mask, int relu, int B, int H, int W,
                    int N, float* y, int m, const float* residual, void* stream);
/* weight gradient side: dM[xi][t][n] = (A g A^T)[xi] of the m x m output-gradient tile; dU[xi] = dM[xi]^T V[xi] through
 * nbm_conv_wgrad (groups = (m+2)^2) and dW = G^T dU G on the host.  bias_grad [N] (may be NULL): += sum over pixels of g. */
int nbm_wino_outgrad(const float* g, int B, int H, int W, int N, float* dM, float* bias_grad, int m, void* stream);
/* Deterministic twins of the four transforms whose bias gradient rides along (nbm_wino_outgrad, nbm_wino23_outgrad_tiles,
 * nbm_cell_outgrad, nbm_cell_dgrad_output): instead of LDS atomics followed by global ones, every workgroup adds its threads' shares in
 * thread order and stores them into its own slot of `workspace` (16-byte aligned, >= nbm_bias_grad_workspace(N) bytes, never zeroed); an
 * ordered reduction adds the slots into bias_grad (still +=).  Everything else is the default kernel.  nbm_bias_grad_workspace: host only. */
int nbm_bias_grad_workspace(int N, int64_t* bytes);
int nbm_wino_outgrad_det(const float* g, int B, int H, int W, int N, float* dM, float* bias_grad, int m, void* workspace,
                         int64_t workspace_bytes, void* stream);

/* Weight side of the Winograd convolutions (csrc/winograd.hip).
 *   nbm_wino_weight:      g [N][C][3][3] (checkpoint layout) -> U [(m+2)^2][N'][C'] = G g' G^T in float64, rounded once.
 *                         transposed = 0: g' = g.  transposed = 1: the data-gradient convolution's weights, g'[c][n][a][b] =
 *                         scale[n] g[n][c][2-a][2-b] (kernel rotated by 180 degrees, channel roles swapped, optional
 *                         per-output-channel FrozenBN scale folded in), N' = C, C' = N.
 *   nbm_wino_weight_grad: dU [(m+2)^2][N][C] -> dW [N][C][3][3] = row_scale[n] G^T dU G (row_scale optional). */
int nbm_wino_weight(const float* g, const float* scale, int N, int C, int transposed, int m, float* U, void* stream);
int nbm_wino_weight_grad(const float* dU, const float* row_scale, int N, int C, int m, float* dW, void* stream);

/* Winograd F(2x2,3x3) forward convolution in two launches (csrc/wino_fused.hip):
 *   nbm_wino23_rows:       x [B][H][W][C] -> R [4][B][TH][WP][C], TH = ceil(H/2), WP = 2 ceil(W/2) + 2: the four row
 *                          combinations (B^T d)_i of every tile row as zero-bordered image rows (2x the input);
 *   nbm_wino23_conv_fused: R, U [16][N][C] (G g G^T) -> y [B][H][W][N] = mask(relu(conv * scale + shift)); the column half
 *                          of the input transform, the 16 transformed-domain GEMMs (fp32 MFMA) and the output transform
 *                          run in one kernel.  scale / shift / mask optional.  C % 32 == 0, C >= 64, N % 4 == 0.
 *                          variant: 0 = automatic, 128 / 64 = channel-tile width. */
int nbm_wino23_rows(const float* x, int B, int H, int W, int C, float* R, void* stream);
int nbm_wino23_conv_fused(const float* R, const float* U, const float* scale, const float* shift, const float* mask,
                          int relu, int B, int H, int W, int C, int N, float* y, int variant, void* stream);

/* Demand-driven evaluation of a 3x3 convolution: only the listed 2 x 2 output tiles are computed.  The finest FPN output map
 * (fpn.py:145, level P1 at 188x512) has two consumers in the reference: the RPN's stride-8 depthwise convolution
 * (layers.py:62-65,81: a fixed 3x3-every-8 pixel pattern) and the RoI pooling of the RoIs assigned to that level
 * (layers.py:408-417,464-467); every other pixel of the map is computed by the reference and never read.
 *   tiles:     n_entries int32 (n_entries % 128 == 0): linear tile id b * TH * TW + ty * TW + tx, ascending inside each
 *              128-entry block, -1 = none (only at the end of a block); the tiles of a block lie within 8 consecutive images.
 *   n_blocks:  optional device scalar: number of leading 128-entry blocks that are filled (the rest is not read).
 *   blk_info:  optional, one word per 128-entry block: bits 0-15 = the transformed-domain planes xi = 4 i + j to compute,
 *              bits 16-19 = the output pixels 2 p + q of every tile of the block to store.  A tile of which the reader only
 *              wants the second output row (the stride-8 pattern enters most tiles through one row or one pixel) needs the
 *              planes i = 1..3 only: 12 or 9 GEMMs instead of 16; the pixels it does store are bit-identical.
 *   nbm_wino23_rows_tiles:       row half of the input transform for the four columns of every listed tile;
 *   nbm_wino23_conv_fused_tiles: as nbm_wino23_conv_fused, writes ONLY the pixels of the listed tiles;
 *   nbm_roi_tiles:               builds such a list on the device from the RoI windows (exactly the windows nbm_roi_pool
 *                                reads, one shared device function; a window with no pixel in the map lists no tile;
 *                                n_roi: device int32 [B], one count per image) of pyramid level `level`, without the tiles flagged in skip [TH * TW] (optional);
 *                                dilate > 0: the tiles within `dilate` pixels of a window instead (where the data gradient of
 *                                a 3x3 convolution of those windows is non-zero);
 *                                tiles must hold B * ceil(TH * TW / 128) * 128 entries; writes *n_blocks. */
int nbm_wino23_rows_tiles(const float* x, int B, int H, int W, int C, const int* tiles, int n_entries, const int* n_blocks,
                          const unsigned* blk_info, float* R,
                          int skip_pattern_stride /* S > 0: the pixels of the 3x3 / stride-S / pad-1 pattern read as zeros (x is a
                                                     gradient map whose pattern share the cell transforms take, see below) */,
                          void* stream);
int nbm_wino23_conv_fused_tiles(const float* R, const float* U, const float* scale, const float* shift, const float* mask,
                                int relu /* bit 0: ReLU; bit 1: ADD the result to y instead of storing it (a tile may then be
                                            listed only once); bit 2: y is COMPACT, [n_entries][2][2][N] in list order (pixels
                                            outside the image are not written) instead of the map */,
                                int B, int H, int W, int C, int N, float* y, const int* tiles, int n_entries,
                                const int* n_blocks, const unsigned* blk_info, void* stream);
int nbm_roi_tiles(const float* rois, const int* n_roi, int B, int roi_cap, int n_levels, int level, const int* fh,
                  const int* fw, const unsigned char* skip, int dilate, int* tiles, int* n_blocks, void* stream);
/* Deterministic twin: the blocks are placed by the exclusive prefix of the images' block counts (a counting pass into `counts`, [B] ints of
 * device scratch, then the placing pass) instead of an atomic counter, so the list is ascending in (image, tile id) on every launch and
 * every kernel that sums over the list sums in that order. */
int nbm_roi_tiles_det(const float* rois, const int* n_roi, int B, int roi_cap, int n_levels, int level, const int* fh,
                      const int* fw, const unsigned char* skip, int dilate, int* tiles, int* n_blocks, int* counts, void* stream);
/* Weight gradient of such a demand-driven convolution: the gradient wrt its output is zero outside the tiles that were
 * read, so only those tiles enter dU[xi] = dM[xi]^T V[xi].  F(2x2,3x3) transforms of the listed tiles (entry -1 = a zero
 * row) into COMPACT operands V [16][n_list][C] and dM [16][n_list][N] (+ bias gradient [N], optional, accumulated); the 16
 * TN GEMMs are nbm_conv_wgrad with groups = 16 over n_list rows.  plane_mask (optional, one word per ENTRY, bits 0-15 = planes
 * xi): the other planes of that entry are written as zeros -- planes the forward pass skipped (their input pixels may never
 * have been computed), or planes that a second entry of the same tile contributes; bit 16 = this entry's pixels enter the
 * bias gradient (a tile that is listed twice sets it once).  skip_pattern_stride S > 0: the pixels of the 3x3 / stride-S /
 * pad-1 reader pattern are read as zeros (their share of the gradient goes through the cell transforms below). */
int nbm_wino23_input_tiles(const float* x, int B, int H, int W, int C, const int* tiles, int n_list, const unsigned* plane_mask,
                           float* V, void* stream);
int nbm_wino23_outgrad_tiles(const float* g, int B, int H, int W, int N, const int* tiles, int n_list, const unsigned* plane_mask,
                             float* dM, float* bias_grad, int skip_pattern_stride, void* stream);
int nbm_wino23_outgrad_tiles_det(const float* g, int B, int H, int W, int N, const int* tiles, int n_list, const unsigned* plane_mask,
                                 float* dM, float* bias_grad, int skip_pattern_stride, void* workspace, int64_t workspace_bytes,
                                 void* stream);
/* Backward pass of the same convolution over the PATTERN pixels of its output gradient (what autograd derives for
 * fpn.py:145 from the RPN's stride-S depthwise convolution, layers.py:62-65,81): the gradient is one 3x3 block per S x S cell
 * (rows S*oy-1 .. S*oy+1, cells = output pixels of the 3x3 / stride-S / pad-1 reader), so per cell the data gradient is the
 * FULL convolution block * kernel (a 5x5 patch) and the weight gradient the correlation of the 5x5 input patch with the
 * block: Toom-Cook with the points {0, 1, -1, 2, -2}, 25 multiplications per (cell, n, c) instead of 81 (csrc/cellwino.hip):
 *   nbm_cell_outgrad       g [B][H][W][N] -> Vg [25][cells][N] = E blk E^T (+ bias_grad [N] += sum of the block pixels, optional)
 *   nbm_cell_input         x [B][H][W][C] -> Vx [25][cells][C] = Vinv^T patch Vinv
 *   nbm_cell_dgrad_output  M [25][cells][C] (= Vg_xi U_xi^T, nbm_gemm_conv with groups = 25, U = E w E^T from the host)
 *                          -> the 5x5 pixels of every cell in gx [B][H][W][C] (parity_class < 0: stored, patches do not overlap:
 *                          S >= 5, other pixels are not written; parity_class 0..3, S >= 3: the cells with
 *                          (oy & 1, ox & 1) == (class >> 1, class & 1) only, ADDED to gx -- four launches accumulate the
 *                          overlapping patches of a stride-3 / 4 pattern)
 * the weight gradient's 25 TN GEMMs dU_xi = Vg_xi^T Vx_xi are nbm_conv_wgrad with groups = 25; dW = E^T dU E on the host. */
int nbm_cell_outgrad(const float* g, int B, int H, int W, int N, int stride, float* Vg, float* bias_grad, void* stream);
int nbm_cell_outgrad_det(const float* g, int B, int H, int W, int N, int stride, float* Vg, float* bias_grad, void* workspace,
                         int64_t workspace_bytes, void* stream);
/* Kernel side of the same algorithm (float64 arithmetic on the device, one rounding; replaces the reference-side autograd of
 * fpn.py:137,145's weights through torch.einsum):
 *   nbm_cell_weight       w [N][C][3][3] (checkpoint layout) -> U = E w E^T as U_nc [25][N][ld] (columns 0..C-1: B operand of the
 *                         FORWARD plane GEMMs) and / or U_cn [25][ldt][N] (rows 0..C-1: B operand of the data-gradient GEMMs); either
 *                         pointer may be NULL
 *   nbm_cell_weight_fold  the deferred lateral (fpn.py:143-144: x = alpha W_lat t + b + up(x1)) folded into those operands:
 *                         alpha U W_lat, W_lat [C][Cin] with row pitch wl_ld, -> columns C..C+Cin-1 of U_nc / rows C..C+Cin-1 of U_cn
 *   nbm_cell_weight_grad  dU [25][N][ld] (columns 0..C-1) -> dW [N][C][3][3] = E^T dU E */
int nbm_cell_weight(const float* w, int N, int C, float* U_nc, int ld, float* U_cn, int ldt, void* stream);
int nbm_cell_weight_fold(const float* w, const float* w_lat, int wl_ld, int N, int C, int Cin, float alpha, float* U_nc, int ld,
                         float* U_cn, int ldt, void* stream);
int nbm_cell_weight_grad(const float* dU, int N, int C, int ld, float* dW, void* stream);
int nbm_cell_input(const float* x, int B, int H, int W, int C, int stride, float* Vx, int ld /* row pitch of Vx, >= c_off + C */,
                   int c_off /* channel offset written */, void* stream);
/* the same transform of patches that are not in memory: pixel = bilinear_align_corners(x1 [B][Hc][Wc][C])[pixel] + bias[C] (the
 * top-down merge of fpn.py:143-144 without its lateral term), 0 outside the image */
int nbm_cell_input_up(const float* x1, const float* bias, int B, int H, int W, int C, int Hc, int Wc, int stride, float* Vx, int ld,
                      int c_off, void* stream);
/* The untransformed forms: Vx [25][cells][ld], plane 5 a + l = pixel (row a, column l) of every cell's 5x5 patch (0 outside the image)
 * -- the operand of a 5x5 / stride S convolution written as 25 taps.  The RPN's strided reader (layers.py:62-65: depthwise 3x3 / stride S
 * -> 1x1 -> BatchNorm -> SiLU) composed with the linear output convolution in front of it (fpn.py:137,145) is ONE such convolution: in
 * evaluation mode the pattern pixels of the on-demand FPN levels are never formed (ondemand.rpn_composite). */
int nbm_cell_patches(const float* x, int B, int H, int W, int C, int stride, float* Vx, int ld, int c_off, void* stream);
int nbm_cell_patches_up(const float* x1, const float* bias, int B, int H, int W, int C, int Hc, int Wc, int stride, float* Vx, int ld,
                        int c_off, void* stream);
/* nbm_cell_patches_up before its horizontal interpolation: with a ratio of about 1/2 the five pixels of a patch row read at
 * most four consecutive columns xb(ox) .. xb(ox) + 3 of x1, in combinations that depend on the cell column ox alone and that the
 * consumer holds in its weights.  Vx [OW][20][B * OH][C], plane 4 j + s of cell (b, oy, ox) at row b * OH + oy of group ox:
 * (hy x1[y0][xb + s] + ly x1[y1][xb + s]) + bias with the row arithmetic of nbm_cell_patches_up; 0 where patch row j lies outside the
 * image or no in-image pixel of the row reads that column.  NBM_EUNSUPPORTED when some cell column's window is wider than four. */
int nbm_cell_patches_up_cols(const float* x1, const float* bias, int B, int H, int W, int C, int Hc, int Wc, int stride, float* Vx,
                             void* stream);

/* Rectangle copy between a strided array and packed rows (no counterpart in the reference: plumbing of the composed RPN reader in
 * training mode, DESIGN 4h -- the border-cell classes of reference layers.py:22-29's depthwise padding are rectangles [r0, r1) x [c0, c1)
 * of the OH x OW cell grid of every (plane, image)): for o < n_outer, r < n_rows:  packed[(o * n_rows + r) * width ...] <->
 * strided[o * outer_pitch + r * row_pitch ...], `width` floats each.  to_strided = 0: packed <- strided (zero_strided = 1 also clears
 * the source rectangle); to_strided = 1: strided <- packed.  All counts in floats, multiples of 4; 16-byte aligned pointers. */
int nbm_copy_rect(float* strided, float* packed, int64_t n_outer, int64_t outer_pitch, int n_rows, int64_t row_pitch, int64_t width,
                  int to_strided, int zero_strided, void* stream);
int nbm_cell_dgrad_output(const float* M, int B, int H, int W, int C, int stride, float* gx, int parity_class,
                          int ld /* row pitch of M, >= c_off + C */, int c_off /* first channel of M read */,
                          float* bias_grad /* optional [C]: += sum of the patch pixels written (inside the image) */, void* stream);
int nbm_cell_dgrad_output_det(const float* M, int B, int H, int W, int C, int stride, float* gx, int parity_class, int ld, int c_off,
                              float* bias_grad, void* workspace, int64_t workspace_bytes, void* stream);
/* FORWARD of the pattern pixels with the same 25 products per cell (the correlation form, F(3x3,3x3)): nbm_cell_input of the
 * input, M_xi = Vx_xi U_xi^T (U = E w E^T as [25][N][C]), then blk = E^T M E + bias into the 3x3 pattern block of every cell of
 * y [B][H][W][N] (other pixels are not written). */
int nbm_cell_output(const float* M, const float* bias, int B, int H, int W, int N, int stride, float* y, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Spectrogram front end.  Replaces File_Processor.load/spectrogram/split_power_spec
 * (nbm_model/nbm_datasets/prepare_dataset.py:160-184, 228-252, 255-294) incl. librosa.stft and the
 * ffmpeg 2x resample (third-party).
 */

/* PCM16 -> centre-padded fp32 waveform rows of one STFT chunk.  The 44.1 kHz signal y of row b is pcm/32768
 * (upsample=0, length n) or its 2x half-band integer interpolation (upsample=1, length 2n; hq = 16 Q15 odd-phase taps,
 * oracle/frontend_ref.py:upsample2x_coeffs); the piece y[first, first+count) is written to out[b][lead ...].
 * pad_mode 0 ('constant', librosa >= 0.10): everything else in the row [0, out_ld) is 0.  pad_mode 1 ('reflect',
 * librosa <= 0.9): the `lead` samples in front of and behind the piece mirror it (np.pad(mode='reflect'), needs
 * lead < count), the rest of the row is 0. */
int nbm_pcm16_to_wave(const int16_t* pcm, int64_t pcm_ld, int batch, int n, int upsample,
                      const int32_t* hq, int64_t first, int64_t count, float* out, int64_t out_ld, int lead,
                      int pad_mode, void* stream);

/* fp32 samples at any rate -> centre-padded fp32 waveform rows of one STFT chunk (same row layout and padding as
 * nbm_pcm16_to_wave).  L = M = 1: the piece [first, first+count) of the samples themselves (float / 24- / 32-bit files at
 * 44.1 kHz, librosa.load, prepare_dataset.py:162).  Otherwise the 44.1 kHz signal is the rational L / M polyphase
 * resampling of x (44100 / sr = L / M reduced): y[m] = sum_k taps[(m M) mod L][k] x[floor(m M / L) - T/2 + 1 + k], taps
 * float64 [L][T] (prepare_dataset.py:resample_taps), float64 accumulation in index order; quant16 = 1 rounds y to the
 * 16-bit grid like the reference's `ffmpeg ... -acodec pcm_s16le -ar 44100` (prepare_dataset.py:175-178).  The signal has
 * ceil(n L / M) samples. */
int nbm_resample_to_wave(const float* x, int64_t x_ld, int batch, int64_t n, int L, int M, const double* taps, int T,
                         int64_t first, int64_t count, float* out, int64_t out_ld, int lead, int pad_mode, int quant16,
                         void* stream);

/* Wav payload decoder: the interleaved little-endian sample bytes of `batch` RIFF/WAVE `data` payloads (row b at raw +
 * b * raw_pitch BYTES, n frames of `channels` samples each) -> mono float32 rows out[b][0 .. n) (row pitch out_pitch
 * ELEMENTS; nothing else of a row is written).  Replaces the host decode of File_Processor.load (librosa.load(sr=None,
 * mono=True), prepare_dataset.py:162 = prepare_dataset.read_wav here) in front of nbm_resample_to_wave on the bulk routes
 * (bulk.detect_files, bulk.detect_recordings), bit for bit:
 *   (tag, bits) = (1, 8): (u8 - 128) / 128; (1, 16), (1, 24): i / 2^(bits-1); (1, 32): (float)i32 to nearest even, * 2^-31;
 *   (3, 32): the float itself (one channel: its bits, NaN payloads included); (3, 64): rounded to nearest even;
 *   channels 2 .. NBM_WAV_MAX_CHANNELS: float32 sum in numpy's order (left to right up to 7 channels, pairwise
 *   ((0+1)+(2+3))+((4+5)+(6+7)) for 8), one correctly rounded division by the channel count.
 * `tag` is the resolved format tag (WAVE_FORMAT_EXTENSIBLE 0xFFFE -> the first 16 bits of its sub-format GUID).  Any other
 * (tag, bits) or channel count: NBM_EUNSUPPORTED.  raw must be 16-byte aligned, and raw_pitch a multiple of 16 when
 * batch > 1 (NBM_EALIGN); raw_pitch >= n * frame bytes, out_pitch >= n.  All offsets are 64-bit.  One kernel launch on
 * `stream`, nothing else (capturable). */
#define NBM_WAV_MAX_CHANNELS 8
int nbm_wav_decode(const void* raw, int64_t raw_pitch, int batch, int tag, int bits, int channels, int64_t n, float* out,
                   int64_t out_pitch, void* stream);

/* STFT magnitude in dB for n_bins bins on the fp64 MFMA (librosa.stft + np.abs + amp_to_db + crop,
 * prepare_dataset.py:228-247):
 *   db[b][f][t] = 20 log10(max(floor, | sum_n w[n] wave[b][t*hop + n] exp(-2 pi i (low_bin + f) n / n_fft) |))
 * for a symmetric window with w[0] = 0 (periodic Hann), evaluated as two real GEMMs over k = 0 .. n_fft/2 on
 * s[k] = x[k] + x[N-k] and d[k] = x[k] - x[N-k] (csrc/stft.hip).  basis: float64, MFMA fragment order
 * [basis_bin_tiles][basis_ksteps][64 lanes]{cos, sin}, lane l of (tile bt, step ks) = bin bt*16 + (l & 15),
 * k = 4 ks + (l >> 4); window folded in, the k = n_fft/2 column halved, zero beyond n_fft/2 and beyond n_bins
 * (prepare_dataset.py:dft_basis_f64 builds it).  basis_bin_tiles % 8 == 0.  wave rows are already centre-padded;
 * hop % 4 == 0.  minmax[b] = {min, max} over the row as order-preserving uint32 keys, accumulated into
 * (initialise with nbm_minmax_init). */
int nbm_minmax_init(uint32_t* minmax, int batch, void* stream);
int nbm_stft_db(const float* wave, int64_t wave_ld, int batch, int n_frames, int hop, int n_fft,
                const double* basis, int basis_bin_tiles, int basis_ksteps, int n_bins, float floor_amp,
                float* db, int64_t db_bs, int db_ld, uint32_t* minmax, void* stream);

/* (x - min)/(max - min) + window split (File_Processor.split_power_spec, prepare_dataset.py:255-294):
 * img[b][k][f][c] = norm(db[b][f][k*hop_img + c]) for k < n_img - 1; the LAST window takes its columns from
 * last_cols[c] (w_pix absolute column indices < n_frames, device memory): the host lists there the reference's chunk-end
 * cut and its stepwise reflect padding (prepare_dataset.py:window_columns). */
int nbm_spec_windows(const float* db, int64_t db_bs, int db_ld, int batch, int n_bins, int n_frames,
                     const uint32_t* minmax, float* img, int n_img, int w_pix, int hop_img,
                     const int32_t* last_cols, void* stream);

/* One slot of nbm_spec_windows_table: window `window` (of `n_img`) of one file's dB plane db[n_bins][db_ld] (n_frames
 * valid columns) with that file's min/max keys (minmax[0..1], as nbm_stft_db writes them) and the column list of its LAST
 * window (last_cols[w_pix], prepare_dataset.py:window_columns).  db == NULL: a padding slot. */
typedef struct nbm_window_entry {
  const float* db;
  const uint32_t* minmax;
  const int32_t* last_cols;
  int32_t db_ld, n_frames, window, n_img;
} nbm_window_entry;

/* nbm_spec_windows with the windows of a batch named by a device table (one entry per slot, files of any length mixed):
 * img[b][f][c] = the pixel nbm_spec_windows computes for window table[b].window of table[b]'s file, bit for bit; padding
 * slots are zeroed.  img: [batch][n_bins][w_pix].  Reads only the table and the planes it names: a captured graph takes a
 * new batch of windows through a new table. */
int nbm_spec_windows_table(const nbm_window_entry* table, int batch, int n_bins, float* img, int w_pix, int hop_img,
                           void* stream);

/* ------------------------------------------------------------------------------------------------
 * Point-wise / small-window detector stages (NHWC fp32).
 */

/* y[p][c] = x[p]*w[c] + b[c]  -- BackboneBase.init_conv (backbone.py:104-105,110-113), 1 -> C. */
int nbm_init_conv(const float* x, int64_t n_pix, const float* w, const float* b, int C, float* y, void* stream);

/* Network stem in one kernel (csrc/stem.hip): y [B][Ho][Wo][64] = relu(scale * conv7x7_s2_p3(init_conv(img)) + shift) on the
 * single-channel image img [B][H][W]: BackboneBase.init_conv (1x1, 1 -> 3, + bias; backbone.py:104-105,110-113) folded into
 * torchvision's conv1 + FrozenBN + ReLU (backbone.py:131).  weff [56][64]: k = 8 r + s (s = 7: zero), weff[k][o] =
 * sum_c W1[o][c][r][s] w_init[c]; wb [64][49] = sum_c W1[o][c][r][s] b_init[c] (summed over the taps INSIDE the image for
 * border pixels), wb_full [64] its sum over all 49 taps (prepared by nets/_prep.py:stem_fold). */
int nbm_stem7x7(const float* img, int B, int H, int W, const float* weff, const float* wb, const float* wb_full,
                const float* scale, const float* shift, float* y, void* stream);

/* Weight-side gradient of the same stem (csrc/stem.hip): g [B][Ho][Wo][64] = gradient wrt the stem output, already masked by the
 * ReLU.  D [64][64] (zeroed here): D[n][8 r + s] = U[n][r][s] = sum_px g[px][n] img[pix(px) + (r, s)], D[n][56] = S[n] =
 * sum_px g[px][n];  Cb [64][49] (zeroed here): Cb[n][7 r + s] = sum of g[px][n] over the pixels whose tap (r, s) lies outside
 * the image, so that V[n][r][s] = S[n] - Cb[n][7 r + s] counts the init_conv bias only inside conv1's zero padding.  The
 * caller forms dW1 = a U + b V, da = sum W1 U, db = sum W1 V (backbone.py:104-113,131). */
int nbm_stem7x7_wgrad(const float* img, const float* g, int B, int H, int W, float* D, float* Cb, void* stream);
/* its deterministic twin (see the twins under nbm_conv_wgrad_workspace): every workgroup of both kernels stores its accumulators into
 * its own slot of `workspace` (16-byte aligned, >= nbm_stem7x7_wgrad_workspace bytes, host-only query), added in slot order. */
int nbm_stem7x7_wgrad_workspace(int B, int H, int W, int64_t* bytes);
int nbm_stem7x7_wgrad_det(const float* img, const float* g, int B, int H, int W, float* D, float* Cb, void* workspace,
                          int64_t workspace_bytes, void* stream);

/* 3x3 / stride 2 / pad 1 max pooling -- torchvision ResNet `maxpool` (backbone.py:131).  idx (may be NULL; training):
 * one byte per output element = r*3+s of the first maximum in scan order, consumed by nbm_maxpool3x3s2_bwd. */
int nbm_maxpool3x3s2(const float* x, int B, int H, int W, int C, float* y, int Ho, int Wo, uint8_t* idx, void* stream);
/* `--dilation` (backbone.py:129-131, torchvision replace_stride_with_dilation on layer4): a 3x3 / dilation-2 / pad-2 convolution on an
 * even-sized map is four ordinary 3x3 / pad-1 convolutions on the parity classes of its pixels, so the dilated bottlenecks run the
 * ordinary kernels on the space-to-batch form  y[(2a+b)*B + n][u][v][c] = x[n][2u+a][2v+b][c]  (x [B][H][W][C] -> y [4B][H/2][W/2][C];
 * inverse != 0: the same map read the other way, x the packed side).  H, W even. */
int nbm_space_to_batch2(const float* x, int B, int H, int W, int C, float* y, int inverse, void* stream);
/* nn.AdaptiveAvgPool2d to exactly half the size (layers.py:84,94 on the 48x128 RPN map of the dilated level): x [B][2Ho][2Wo][C] ->
 * y [B][Ho][Wo][C], mean of each 2x2 block; and its gradient (gx = gy / 4 on the block's four pixels). */
int nbm_avgpool2x2(const float* x, int B, int Ho, int Wo, int C, float* y, void* stream);
int nbm_avgpool2x2_bwd(const float* gy, int B, int Ho, int Wo, int C, float* gx, void* stream);

/* y = bilinear_align_corners(src -> Ho x Wo) [+ add]  -- fpn.py:143-144, layers.py:35-37. */
int nbm_upsample_bilinear_add(const float* src, int B, int Hi, int Wi, int C, const float* add,
                              float* y, int Ho, int Wo, void* stream);

/* in-place row softmax of [rows][cols] with pitch ld -- self_attention.py:47, layers.py:579. */
int nbm_softmax_rows(float* x, int64_t rows, int cols, int64_t ld, void* stream);

/* depthwise 3x3, pad 1, channel multiplier `mult` (out channel o reads in channel o/mult), + bias;
 * optional FiLM: y = y*gamma + beta with film[p][0:Cout]=gamma, film[p][Cout:2Cout]=beta
 * -- DepthwiseSepConv2d.depth_wise / FiLM (layers.py:25-26,38-42). */
int nbm_dwconv3x3(const float* x, int B, int H, int W, int Cin, int mult, int stride,
                  const float* w /*[Cin*mult][9]*/, const float* bias, const float* film, int64_t film_ld,
                  float* y, int Ho, int Wo, void* stream);

/* ---- MBConv (EfficientNet-B0..B4 bodies; csrc/mbconv.hip) -------------------------------------------------------
 * Depthwise k x k convolution (k in {3, 5}, stride in {1, 2}, pad (k - 1) / 2, channel multiplier 1) of an NHWC map, then
 * y = act(conv * scale[c] + shift[c]) with act in {NBM_ACT_NONE, NBM_ACT_SILU}; scale / shift may be NULL (1 / 0).
 * w_taps [k * k][C]: tap-major weights (tap = r * k + s).  C % 4 == 0; anything else: NBM_EUNSUPPORTED (no slow path).
 * Every output element is the sum of its k * k products in (r, s) order (zero products outside the image), whatever the launch shape.
 * pool_part (or NULL) [B][nbm_dwconv_pool_slots(C, Ho, Wo)][C]: every slot is WRITTEN with one workgroup's sum of its activated
 * outputs -- no atomics, no zero fill needed; the slots of image b depend on image b alone. */
int nbm_dwconv_bn_act(const float* x, int B, int H, int W, int C, int k, int stride, const float* w_taps, const float* scale,
                      const float* shift, int act, float* y, int Ho, int Wo, float* pool_part, void* stream);
/* slots per image of pool_part for an output map of Ho x Wo x C (< 0: an error code); output rows per strip of a workgroup */
int nbm_dwconv_pool_slots(int C, int Ho, int Wo);
int nbm_dwconv_strip_rows(void);
/* Squeeze-and-excitation behind nbm_dwconv_bn_act, one launch: mean[b][c] = inv_hw * (pool_part[b][0][c] + pool_part[b][1][c] + ...),
 * s = silu(w1 mean + b1) (w1 [Csq][C]), gate[b] = sigmoid(w2 s + b2) (w2 [C][Csq]) -> gate [B][C].  Csq is any positive number.
 * wb (or NULL) [B][N][w_ld], w_ld % 32 == 0, w_ld >= C: the project convolution's weights wproj [N][wp_ld >= C] with the gate folded
 * in, wb[b][n][c] = wproj[n][c] * gate[b][c], columns C .. w_ld - 1 written as zeros -- the B operand of nbm_gemm_conv with groups = B. */
int nbm_se_gate(const float* pool_part, int B, int n_slots, int C, float inv_hw, const float* w1, const float* b1, int Csq,
                const float* w2, const float* b2, float* gate, const float* wproj, int wp_ld, int N, float* wb, int w_ld, void* stream);

/* y = x * sigmoid(x) -- nn.SiLU (layers.py:31,41). */
int nbm_silu(const float* x, float* y, int64_t n, void* stream);

/* y[r][:] = (x[r][:] - mean_r) / sqrt(var_r + eps) * w + b over rows of E floats (biased variance) -- nn.LayerNorm of the
 * Transformer_RCNN head (reference layers.py:589-651, self_attention.py:110-131). */
int nbm_layernorm(const float* x, int64_t rows, int E, const float* w, const float* b, float eps, float* y, void* stream);

/* out = softmax(scale * Q K^T) V per (batch entry, head) for sequences of S <= 1024 tokens, hd <= 512: token (s, n) is row
 * s*seq_stride + n*batch_stride of q/k/v/out (row pitches *_ld floats, head h at columns [h*hd, (h+1)*hd)); keys with
 * s >= *n_valid (device counter, may be NULL) are masked -- nn.MultiheadAttention inside the Transformer_RCNN encoder
 * (reference layers.py:613-621,645-646; self_attention.py:110-126).  hd <= 64: one lane per output column, K and V of an
 * (entry, head) whole in LDS; 64 < hd <= 512: the head dimension passes through LDS in 64-column chunks (csrc/mha.hip, "wide
 * heads"); hd > 512 is NBM_EINVAL.  128 < S <= 1024, any hd: the "long" kernels -- K and V pass through LDS in blocks of 128 keys,
 * the score rows of 8 queries wait in LDS, the softmax is the plain one over the whole row; the choice follows the launch's S,
 * never *n_valid.  S > 1024 is NBM_EINVAL with nothing launched.  The same split and limits hold for the three entry points below
 * that share this token layout, and for nbm_mha_segments_wide in ACROSS_ROIS (nbm_mha_plan reports the choice). */
int nbm_mha_small(const float* q, const float* k, const float* v, int q_ld, int k_ld, int v_ld, float* out, int out_ld,
                  int S, int N, int nhead, int hd, int64_t seq_stride, int64_t batch_stride, const int32_t* n_valid,
                  float scale, void* stream);

/* nbm_mha_small for a batch that is several model calls (evaluation only, no backward form): token (b, r) is row b*R + r of
 * q/k/v/out, `segments` the int32 [2][B] table of nbm_rpn_select (first image and image count of b's segment), n_roi[b] the RoI
 * count of image b (equal within a segment).  ACROSS_ROIS (tf_pe_qk): per image, keys and queries r < n_roi[b]; `segments` is
 * not read.  ACROSS_IMAGES (default flavour, batch_first=False): per segment and slot r < n_roi[first], the sequence is the
 * segment's images.  EVERY row of `out` is written: rows that are no valid token (r >= n_roi, failed segments) are zero, so
 * the caller need not pre-fill.  A valid row holds the bits nbm_mha_small gives when it is run on that row's segment alone.
 * hd <= 64 (callers rely on the refusal above it; nbm_mha_segments_wide below takes the wider heads).
 * max_count: the caller's bound on the table's segment counts (<= 128); the rows of a segment above it, or of an entry that
 * is no segment inside [0, B), are zero -- the per-segment model calls of the reference CLI (run_detection.py:49-55) through
 * layers.py:613-621,645-646. */
#define NBM_MHA_ACROSS_ROIS 0
#define NBM_MHA_ACROSS_IMAGES 1
int nbm_mha_segments(const float* q, const float* k, const float* v, int q_ld, int k_ld, int v_ld, float* out, int out_ld,
                     int B, int R, int nhead, int hd, int mode, const int32_t* segments, const int32_t* n_roi, int max_count,
                     float scale, void* stream);
/* nbm_mha_segments for every head dim nbm_mha_small takes, 1 <= hd <= 512: the same arguments, checks and results; hd <= 64 is
 * the launch nbm_mha_segments makes, above it the wide segments kernel (csrc/mha.hip).  hd > 512: NBM_EINVAL.
 * ACROSS_ROIS also takes 128 < R <= 1024 slots, through the long kernels of nbm_mha_small (a valid row holds the bits
 * nbm_mha_small gives with S = R); R > 1024: NBM_EINVAL.  ACROSS_IMAGES takes any R and keeps max_count <= 128. */
int nbm_mha_segments_wide(const float* q, const float* k, const float* v, int q_ld, int k_ld, int v_ld, float* out, int out_ld,
                          int B, int R, int nhead, int hd, int mode, const int32_t* segments, const int32_t* n_roi,
                          int max_count, float scale, void* stream);

/* softmax over the (bg, fg) pair of every anchor: x[p][2a], x[p][2a+1] (pitch ld) -> y (pitch y_ld)
 * -- layers.py:90. */
int nbm_pair_softmax(const float* x, int64_t n_pix, int n_anchor, int x_ld, float* y, int y_ld, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Proposal / RoI / detection stages (integer + sort work; bit-exact vs the oracle).
 */

/* ProposalLayer decode (layers.py:266-285, nets_utils.py:169-186): per image and anchor (K-major):
 * boxes[b][i][4] (rounded, clipped), keys[b][i] = order-preserving uint32 of the fg score or 0 when the
 * box is smaller than min_size; keep_count[b] = #kept. cls: [B][K][2A] softmaxed, reg: [B][K][4A]. */
int nbm_rpn_decode(const float* cls, const float* reg, const float* anchors /*[K*A][4]*/, int B, int KA,
                   int n_anchor /*A: anchors per location*/, int img_w, int img_h, int min_size, float* boxes,
                   uint32_t* keys, int* keep_count, void* stream);

/* Input images that hold a NaN keep no anchor: keep_count[b] = 0 for every image b of img [B][n] with a NaN among its n
 * values (the reference's NaN reaches every RPN output, and no comparison with NaN is true).  Launch after nbm_rpn_decode
 * on the same stream, before nbm_rpn_select. */
int nbm_nan_images(const float* img, int B, int64_t n, int* keep_count, void* stream);

/* Proposal counts.  Every count pointer of this section (n_sel, n_in, n_out, n_roi) is a device int32 [B], one count
 * per image.  How the images are coupled is decided by the segment table `seg` of the two entry points below, a device
 * int32 [2][B]: seg[b] = first image of b's segment, seg[B + b] = its image count.  Each contiguous segment is one model
 * call of the reference: the pre- and post-NMS top-N (layers.py:287, nets_utils.py:236) and the "RPN failed" rule are
 * minima over that segment alone.  One segment of B images is the reference's single call on the batch; B segments of
 * one image are B independent calls (bulk inference over files that the reference CLI runs one per model call,
 * nbm_detect.py:24-28; windows [k*bs, (k+1)*bs) of one file, run_detection.py:40-67, form one segment each).
 * seg == NULL returns NBM_EINVAL. */

/* Top-N selection by (score desc, index asc) among kept anchors, N_b = min(top_n, min over b's segment of
 * keep_count); N_b = 0 if < fail_below ("RPN failed", layers.py:287-290).  Writes sel_boxes[b][cap][4],
 * sel_scores[b][cap], n_sel[b] = N_b.  -- layers.py:292-297.  cap >= top_n, cap power of two <= 4096 (the keys are sorted in
 * LDS; nbm_rpn_select_big below takes larger ones). */
int nbm_rpn_select(const float* boxes, const uint32_t* keys, const int* keep_count, int B, int KA,
                   int top_n, int fail_below, int cap, float* sel_boxes, float* sel_scores, int* n_sel,
                   const int* seg, void* stream);

/* Greedy NMS in the given order (suppress IoU >= thresh, +1 pixel convention) of the n_in[b] boxes of image b, then
 * the coupled truncation R_b = min(post_n, min over b's segment of #keep) -- nets_utils.py:189-245.
 * Workspaces: mask_ws B*cap*(cap/64) uint64, keep_ws B*(cap+1) int32.  Writes rois[b][post_n][4],
 * roi_scores[b][post_n], n_out[b] = R_b.  cap: multiple of 64, <= 4096 (one wave holds the removed bits; nbm_nms_big below
 * takes larger ones). */
int nbm_nms_batched(const float* boxes, const float* scores, const int* n_in, int B, int cap, float thresh,
                    int post_n, uint64_t* mask_ws, int* keep_ws, float* rois, float* roi_scores, int* n_out,
                    const int* seg, void* stream);

/* The two stages above for up to 65 536 boxes per image (--pre_nms_topN / --pre_nms_topN_eval above 4 096), with the same
 * contracts and, on any input both take, the same bits.  Kernel launches only: they run inside a captured graph.  The
 * workspaces may hold stale bytes.
 * nbm_rpn_select_big: cap >= top_n, cap a power of two in 64 .. 65 536; ws: ws_bytes >= nbm_rpn_select_big_workspace(B, cap)
 * = 8 * B * cap (the composite keys are sorted in global memory, run by run through LDS), 8-byte aligned.  A segment
 * minimum above KA is cut to KA. */
int nbm_rpn_select_big_workspace(int B, int cap, int64_t* bytes);
int nbm_rpn_select_big(const float* boxes, const uint32_t* keys, const int* keep_count, int B, int KA, int top_n,
                       int fail_below, int cap, void* ws, int64_t ws_bytes, float* sel_boxes, float* sel_scores,
                       int* n_sel, const int* seg, void* stream);

/* nbm_nms_big: cap a multiple of 64 up to 65 536, 0 < post_n <= cap, n_in[b] clamped into [0, cap].  No IoU mask is stored:
 * one workgroup per image walks 64-box blocks and tests each block against the boxes kept so far, and the walk ends at
 * post_n kept boxes.  ws: ws_bytes >= nbm_nms_big_workspace(B, cap) = one int32 per image + padding, 4-byte aligned. */
int nbm_nms_big_workspace(int B, int cap, int64_t* bytes);
int nbm_nms_big(const float* boxes, const float* scores, const int* n_in, int B, int cap, float thresh, int post_n,
                void* ws, int64_t ws_bytes, float* rois, float* roi_scores, int* n_out, const int* seg, void* stream);

/* ROIPooling (layers.py:406-497) at any pool size (train.py:115-117, --roi_pool_h / --roi_pool_w).  fmaps: n_levels device
 * pointers (NHWC, C channels); pe_f [img_h][C/2], pe_t [img_w][C/2].  n_roi[b] RoIs in image b out of roi_cap slots.
 * Level assignment (layers.py:408-417), rounding, the y2 clamp, the clamped x2 for the map / unclamped x2 for the encoding;
 * the window is grown to at least pool_h x pool_w (layers.py:459-465, as a loop bounded by the pool size), bins are
 * [floor(i*h/ph), ceil((i+1)*h/ph)) x [floor(j*w/pw), ceil((j+1)*w/pw)), each summed row-major in fp32 and divided once by its
 * area; the positional encoding is accumulated in double and rounded once.  One window function (csrc/roipool.hip) serves these
 * kernels, nbm_roi_tiles and nbm_zero_roi_windows.  A RoI whose window has no pixel in the map (coordinates outside the image):
 * its level is written, nothing else is read or written -- with zeroed outputs its rows stay zero.
 * Only the window of a RoI is read, so a demand-driven map whose tiles under the RoIs are computed (nbm_roi_tiles) serves as well
 * as a dense one.  One workgroup per RoI slot, 16-byte accesses along C when C % 4 == 0 and the map and output pointers are
 * 16-byte aligned, 4-byte accesses otherwise.  Slots r >= n_roi[b] are left untouched.
 * Outputs NHWC [B*roi_cap][pool_h][pool_w][C].
 * Refused before any launch, nothing written: NBM_EUNSUPPORTED for pool_h < 2 or pool_w < 2 (the reference's one-row
 * positional-encoding slice layers.py:484 is empty, its mean NaN) and for pool_h > min(fh) or pool_w > min(fw) (the reference's
 * growth loop does not terminate); NBM_EINVAL for n_levels outside 1..5, odd C, a map below 2 x 2, null pointers. */
typedef struct nbm_roi_hw_desc {
  const float* fmap[5];
  int fh[5], fw[5];
  int n_levels, C;
  const float* rois;     /* [B][roi_cap][4] */
  const int* n_roi;      /* device int32 [B] */
  int B, roi_cap;
  const float* pe_f; const float* pe_t; int img_h, img_w;
  float* pool; float* pe; int* level;
  int pool_h, pool_w;
} nbm_roi_hw_desc;
int nbm_roi_pool_hw(const nbm_roi_hw_desc* d, void* stream);

/* The reference's default pool: nbm_roi_pool_hw with pool_h = pool_w = 2 (nbm_roi_desc is nbm_roi_hw_desc without the pool
 * size), same kernel, same argument checks.  Outputs NHWC [B*roi_cap][2][2][C]. */
typedef struct nbm_roi_desc {
  const float* fmap[5];
  int fh[5], fw[5];
  int n_levels, C;
  const float* rois;     /* [B][roi_cap][4] */
  const int* n_roi;      /* device int32 [B] */
  int B, roi_cap;
  const float* pe_f; const float* pe_t; int img_h, img_w;
  float* pool; float* pe; int* level;
} nbm_roi_desc;
int nbm_roi_pool(const nbm_roi_desc* d, void* stream);

/* FastRCNN eval post-processing (layers.py:688-776) for B images, n_roi[b] RoIs in image b:
 * class arg-max, per-class delta gather, decode+clip, sort by score, drop background, class-agnostic
 * NMS, per-class NMS (top proposal_number) and score > min_score.  Output rows sorted by (class asc,
 * score desc): det[b][cap][6] = {class, x1, y1, x2, y2, score}, n_det[b]. */
int nbm_rcnn_post(const float* rois, const int* n_roi, int B, int roi_cap, const float* bbox_reg,
                  const float* bbox_cls, int n_cls1 /*1+num_classes*/, int img_w, int img_h,
                  float nms_thresh, float min_score, int proposal_number, float* det, int* n_det, void* stream);

/* Per-file merge of the window outputs of one recording (run_detection.py:163-249), for any box count up to
 * NBM_MERGE_MAX_N.  nbm_merge_collect -> nbm_merge_nms -> nbm_merge_gather, all on one stream, no host sync. */
#define NBM_MERGE_MAX_N 131072

/* Collect (run_detection.py:180-221): det[n_img][cap][6] = the rows nbm_rcnn_post writes for the file's windows in order
 * ({class, x1, y1, x2, y2, score}, sorted by (class, score desc)), n_det[n_img].  Per row of window i: the border rules as the
 * reference's if/elif chain (:195-200; first window: x2 >= w_pix - 5, last: x1 <= 4, inner: either; each only for widths
 * x2 - x1 < float32(0.9 * (w_pix - hop))), then x1, x2 += hop * i (one fp32 add each, :208-209), then the drop of
 * x2 >= spectrogram_length (:211-217).  Output compacted in the reference's collected order -- class 1..num_classes, then window,
 * then row: boxes[N][4] (shifted), scores[N], species[N] (int class), n_out[0] = N <= n_img * cap.  Rows whose class is not
 * in 1..num_classes are dropped.  cell_ws: n_img * num_classes int32.  n_img * cap and n_img * num_classes <= 2^30. */
int nbm_merge_collect(const float* det, const int* n_det, int n_img, int cap, int num_classes, int w_pix, int hop,
                      int64_t spectrogram_length, int* cell_ws, float* boxes, float* scores, int* species, int* n_out,
                      void* stream);

/* Workspace bytes of nbm_merge_nms for capacity cap (0 <= cap <= NBM_MERGE_MAX_N, else NBM_EINVAL): the bitmask tiles of
 * the dense worst case, 64 x 64 bits per pair of 64-box blocks (rb <= cb), = 512 * nb * (nb + 1) / 2 bytes with
 * nb = ceil(cap / 64) (about cap^2 / 16: 300 MB at 69 250 boxes, 1.07 GB at 2^17), plus the block x-ranges. */
int nbm_merge_nms_workspace(int cap, int64_t* bytes);

/* Greedy NMS of nets_utils.nms with post_nms_topN = n (nets_utils.py:210-245, run_detection.py:233) over
 * n = min(max(n_in[0], 0), cap) boxes[n][4]: walk in the GIVEN order (no re-sort), a kept box removes every later box with
 * IoU >= thresh (fp32, +1 pixel, union = (aa + ab) - inter, no contraction).  keep[0 .. n_keep[0]) = kept indices in walk
 * order.  Tiles of block pairs whose x-ranges cannot overlap under the +1 convention are skipped when thresh > 0.
 * ws: ws_bytes >= nbm_merge_nms_workspace(cap).  cap <= NBM_MERGE_MAX_N and a non-null ws, else NBM_EINVAL. */
int nbm_merge_nms(const float* boxes, const int* n_in, int cap, float thresh, void* ws, int64_t ws_bytes, int* keep,
                  int* n_keep, void* stream);

/* Gather (run_detection.py:234-249): rows[r] = {species, x1, y1, x2, y2, score} of box keep[r] for r < n_rows[0] =
 * min(n_keep[0], cap); the kept (class-major) order, ready for one device-to-host copy. */
int nbm_merge_gather(const float* boxes, const float* scores, const int* species, const int* keep, const int* n_keep, int cap,
                     float* rows, int* n_rows, void* stream);

/* Training, AnchorTargetLayer (layers.py:150-179, nets_utils.py:103-126): IoU (inclusive-pixel convention, the reference's fp32
 * operations in its order) of every anchor inside the image with the n_gt[b] boxes of gt[b]; amx[b][a] = index of the FIRST best box,
 * lab[b][a] = the anchor's label BEFORE the random subsampling (0: best overlap < neg_t; 1: best overlap >= pos_t, or the anchor is a
 * best anchor -- ties included -- of a box whose best overlap is > 0; else -1); flag[b] != 0: a NaN / negative overlap occurred
 * (degenerate box), the caller recomputes that image on the host.  The NumPy RNG draws stay on the host (layers.py:183-197).
 * nbm_proposal_iou below: ProposalTargetLayer (layers.py:320-330, nets_utils.py:103-126): rows j < R = proposals rois[b][j], rows R + i = the
 * image's own ground-truth boxes gt[b][i] (the reference appends them to the proposals); for every row the IoU (inclusive-pixel
 * convention, the reference's fp32 operations in its order) with the n_gt[b] <= G boxes of gt[b]: mx[b][j] = best overlap,
 * asg[b][j] = index of the FIRST best box.  The thresholds and the NumPy RNG draws stay on the host (layers.py:332-376). */
int nbm_anchor_targets(const float* anchors /*[n_in][4]: the anchors inside the image*/, int n_in, const float* gt /*[B][G][4]*/,
                       const int* n_gt /*[B]*/, int B, int G /* <= 256 */, float neg_t, float pos_t, signed char* lab /*[B][n_in]*/,
                       short* amx /*[B][n_in]*/, int* flag /*[B]*/, void* stream);
int nbm_proposal_iou(const float* rois /*[B][R][4]*/, const float* gt /*[B][G][4]*/, const int* n_gt /*[B]*/, int B, int R, int G,
                     float* mx /*[B][R+G]*/, int* asg /*[B][R+G]*/, void* stream);

/* ================================================================================================
 * Training path: backward implicit GEMMs, point-wise gradients, train-mode BatchNorm, optimiser.
 * Replaces what torch.autograd derives for the reference's train step (train.py:205-217):
 * conv/linear/matmul backward, ReLU/SiLU/max-pool/bilinear/softmax/BatchNorm backward,
 * torch.nn.utils.clip_grad_norm_ (train.py:213-214) and torch.optim.AdamW.step (train.py:215,302-303).
 */
typedef struct nbm_bwd_desc {
  const float* g;        /* upstream gradient, NHWC [B][Ho][Wo][N] rows (pitch g_ld)                         */
  const float* w;        /* dgrad: KRSC weights [N][w_ld]                                                    */
  const float* x;        /* wgrad: forward input NHWC [B][H][W][Cin] (pitch x_ld)                            */
  float* out;            /* dgrad: dX [B*H*W][out_ld];  wgrad: dW [N][out_ld] (KRSC, += with fp32 atomics)   */
  const float* a_scale;  /* dgrad: per-n multiplier of g (needs N % 32 == 0) or NULL                         */
  const float* row_scale;/* wgrad: per-n multiplier of the dW rows or NULL                                   */
  const float* residual; /* dgrad: added to dX (gradient accumulation) or NULL                               */
  const float* mask;     /* dgrad: dX := 0 where mask <= 0 (ReLU of the producing layer) or NULL             */
  int64_t g_gs, w_gs, x_gs, out_gs, res_gs;
  int groups;
  int B, H, W, Cin, N, kh, kw, stride, pad, Ho, Wo;   /* geometry of the FORWARD convolution                */
  int g_ld, w_ld, x_ld, out_ld, res_ld, mask_ld;
  float alpha;
  float* bias_grad;      /* wgrad: [groups][N], += sum_m g[m][n] (the bias gradient rides along; zeroed by the caller) or NULL */
  const float* residual2;/* dgrad (groups == 1): a HALF-resolution map [B][ceil(H/2)][ceil(W/2)][Cin] (pitch res2_ld), added to dX at
                            the pixels with even iy and ix -- the data gradient of the block's 1x1 / stride-2 shortcut
                            (torchvision Bottleneck.downsample), which is non-zero only there -- or NULL                    */
  int res2_ld;
  const unsigned* mask_bits;/* dgrad (round 5): the ReLU mask as BITS instead of `mask` -- [M][Cin / 32] words, bit c % 32 of word
                            m * (Cin / 32) + c / 32 (bit order of nbm_gemm_desc.bits_out) set where the producer's output was > 0 -- or NULL.
                            Cin % 32 == 0, one group; takes precedence over `mask`.                                          */
  float* workspace;      /* wgrad: NULL = the default kernels (fp32 atomics).  Else the DETERMINISTIC twin: every pixel split stores
                            its scaled dW tile and its bias partial into its own slice of `workspace`, and an ordered reduction adds
                            the slices in split order into `out` / `bias_grad` (still +=).  No atomic; the workspace needs no zeroing.
                            16-byte aligned; size and stride from nbm_conv_wgrad_workspace.                                          */
  int64_t ws_split_stride;/* wgrad: floats between the slices of consecutive splits (>= what nbm_conv_wgrad_workspace reports, % 4 == 0) */
  int64_t workspace_bytes;/* wgrad: bytes behind `workspace`; splits * ws_split_stride * 4 must fit                                   */
} nbm_bwd_desc;

/* dX[b][iy][ix][c] = alpha * sum_{r,s,n} g[b][(iy+pad-r)/stride][(ix+pad-s)/stride][n] * a_scale[n] * W[n][r][s][c]
 * (+ residual, ReLU mask).  stride 2: the pixels are processed by parity class of (iy+pad, ix+pad), each class visiting
 * only the taps that reach it (no multiply-by-structural-zero work).  g rows must be readable (zero padded) up to ceil(N/32)*32 floats.  Also the plain
 * C[M][Cin] = A[M][N] * B[N][Cin] ("NN") GEMM with H = M, W = 1, 1x1. */
int nbm_conv_dgrad(const nbm_bwd_desc* d, void* stream);
/* dW[n][(r,s,c)] += alpha * row_scale[n] * sum_m g[m][n] * x[pix(m)+(r,s)][c]; dW must be zeroed by the caller.
 * Also the plain C[N][Cin] += A[M][N]^T * B[M][Cin] ("TN") GEMM. */
int nbm_conv_wgrad(const nbm_bwd_desc* d, void* stream);
/* Workspace of nbm_conv_wgrad's deterministic twin for this descriptor (its `workspace` fields are ignored): *bytes = splits x slice,
 * with `splits` of the twin's plan (nbm_gemm_plan of the descriptor with `workspace` set; at most 1 GiB, a plan beyond it gets fewer
 * splits; ONE slice beyond it: NBM_EUNSUPPORTED) and slice = groups * N * ceil4(kh * kw * Cin) floats (+ ceil4(groups * N) where bias_grad
 * is set) = *split_stride (may be NULL) -- the rows at their own pitch, not at out_ld.  *bytes = 0: one split and no bias gradient -- the default kernel adds one value per element, nothing to order.  Host only,
 * launches nothing; returns what nbm_conv_wgrad would return for an invalid descriptor. */
int nbm_conv_wgrad_workspace(const nbm_bwd_desc* d, int64_t* bytes, int64_t* split_stride);

/* ---- deterministic twins of the reductions that sum with floating-point atomics (train.py --deterministic; no reference counterpart).
 * Each twin's workgroups STORE partial sums into slots of `workspace` (16-byte aligned, >= nbm_det_workspace bytes, never zeroed, its
 * previous contents never read) and an ordered reduction adds the slots in ascending order: the same bits on every launch, whatever the
 * placement of the workgroups.  Arguments before `workspace` are those of the default entry point. */
enum { NBM_DET_COLSUM = 0, NBM_DET_SQNORM = 1, NBM_DET_BN = 2, NBM_DET_WEIGHTED_SUM = 3, NBM_DET_DWCONV = 4 };
/* workspace bytes of twin `op` -- COLSUM / BN: rows = M, cols = N / C; SQNORM / WEIGHTED_SUM: rows = n, cols = 1; DWCONV: rows =
 * B * Ho * Wo, cols = Cin * mult.  Host only. */
int nbm_det_workspace(int op, int64_t rows, int cols, int64_t* bytes);
/* the ordered reduction itself: out[i] (+)= sum_{s < slots} part[s * n + i] in ascending s; part float or double (part_is_double) */
int nbm_ordered_sum(const void* part, int part_is_double, int slots, int64_t n, float* out, int accumulate, void* stream);
int nbm_colsum_det(const float* g, int64_t M, int N, int ld, float* out, void* workspace, int64_t workspace_bytes, void* stream);
int nbm_weighted_sum_bwd_det(const float* x0, const float* x1, const float* x2, const float* weights, const float* g, float* gx0,
                             float* gx1, float* gx2, float* gw, int64_t n, void* workspace, int64_t workspace_bytes, void* stream);
int nbm_dwconv3x3_bwd_det(const float* x, const float* g, const float* w, int B, int H, int W, int Cin, int mult, int stride, float* gx,
                          float* gw, float* gb, int Ho, int Wo, void* workspace, int64_t workspace_bytes, void* stream);
int nbm_bn_train_fwd_det(const float* x, int64_t M, int C, const float* w, const float* b, float eps, float momentum, float* run_mean,
                         float* run_var, double* stats_ws, float* mean, float* invstd, float* y, void* workspace,
                         int64_t workspace_bytes, void* stream);
int nbm_bn_train_bwd_det(const float* g, const float* x, int64_t M, int C, const float* mean, const float* invstd, const float* w,
                         double* red_ws, float* gx, float* gw, float* gb, void* workspace, int64_t workspace_bytes, void* stream);
/* *out += sum g^2, partials and sum in double */
int nbm_sqnorm_accum_det(const float* g, int64_t n, double* out, void* workspace, int64_t workspace_bytes, void* stream);

/* The launch plan of the three GEMM entry points: which kernel instantiation a descriptor runs on, with what grid, and the tiling values
 * the launch derives beyond the descriptor (csrc/igemm_plan.h; no counterpart in the reference, whose convolutions are dispatched inside
 * torch).  nbm_gemm_plan reads the environment switches as the entry point would, plans and launches NOTHING: it touches no HIP API and
 * works on a machine without a GPU.  kind: 0 = nbm_gemm_conv (desc: nbm_gemm_desc), 1 = nbm_conv_dgrad, 2 = nbm_conv_wgrad (desc:
 * nbm_bwd_desc).  Returns (and stores in rc) what the entry point would return before launching: NBM_OK or its NBM_E* code; on an error
 * the other fields are unset.  halves = 1: the channel count is 64 past a multiple of 128 (N of nbm_gemm_conv, Cin of nbm_conv_wgrad) and
 * the entry point runs the first count - 64 channels and the last 64 as two calls of itself; the plan is that of the first call. */
typedef struct nbm_gemm_plan_t {
  const char* name;      /* the kernel instantiation, e.g. "igemm_kernel<128,128,64,64,0,0,2,false>" (static storage)           */
  int rc;
  int kernel;            /* id of `name` (csrc/igemm_plan.h: GemmKernel)                                                        */
  int grid[3], block;
  int m_tiles, n_tiles;  /* tile counts as the kernel receives them                                                             */
  int vec_epi;           /* 16-byte epilogue                                                                                    */
  int fast;              /* forward: 16-byte gather (Cin % 32 == 0, aligned) instead of the generic one                         */
  int slices;            /* stream1x1 forms: slices of N (grid y)                                                               */
  int phased;            /* data gradient, stride 2: M tiles grouped by parity class, ph_tiles[class] tiles each                */
  int ph_tiles[4];
  int splits, k_chunk;   /* weight gradient: splits of the pixel reduction (grid y), pixels per split                           */
  int plain, b_generic, narrow_m; /* weight gradient: 1x1 / stride 1 / pad 0; scalar gather of x; 64-row dW tiles               */
  int halves;
} nbm_gemm_plan_t;
int nbm_gemm_plan(int kind, const void* desc, nbm_gemm_plan_t* out);

/* What a launch of nbm_mha_small, nbm_mha_small_drop or their backwards with this S, hd, N and nhead runs on (csrc/mha.hip), in the spirit
 * of nbm_gemm_plan: host only, launches nothing, touches no HIP API.  family: narrow (S <= 128, hd <= 64), wide (S <= 128, 64 < hd <= 512)
 * or long (128 < S <= 1024, hd <= 512); nbm_mha_segments_wide in ACROSS_ROIS takes the family of (R, hd).  Returns (and stores in rc)
 * NBM_OK, or the NBM_EINVAL the entry points return for that geometry, with the other fields zero. */
#define NBM_MHA_NARROW 0
#define NBM_MHA_WIDE 1
#define NBM_MHA_LONG 2
typedef struct nbm_mha_plan_t {
  int rc;
  int family;
  int lds_bytes;            /* static LDS of the forward kernel's workgroup ...                                                  */
  int lds_bytes_bwd;        /* ... and of the backward's pass 1 (pass 2 uses none)                                               */
  int rows;                 /* query rows per workgroup (narrow: the whole sequence)                                             */
  int row_blocks;           /* workgroups per (batch entry, head)                                                                */
  int64_t workspace_bytes;  /* the backward's workspace: 2 * S * S floats per (batch entry, head)                                */
} nbm_mha_plan_t;
int nbm_mha_plan(int S, int hd, int N, int nhead, nbm_mha_plan_t* out);

int nbm_relu_bwd(const float* gy, const float* y, float* out, int64_t n, void* stream);
int nbm_silu_bwd(const float* gy, const float* x, float* out, int64_t n, void* stream);
/* out[i] = alpha*a[i] + beta*b[i % b_period] (b may be NULL; b_period 0: b has n elements): gradient accumulation, the
 * doubled identity levels of SAPyramid (self_attention.py:76), `features + pos` of --add_posenc (nbm_model.py:45-46) */
int nbm_axpby(const float* a, const float* b, float* out, float alpha, float beta, int64_t n, int64_t b_period, void* stream);
/* BiFPN FusionModule (fpn.py:20-30): out = (sum_i relu(w_i) x_i) / (sum_i relu(w_i) + 1e-4), 2 inputs (x2 NULL) or 3;
 * `weights` is the raw learnable parameter on the device.  Backward: gx_i (any may be NULL) and gw[i] += d/dw_i (zeroed
 * by the caller). */
int nbm_weighted_sum(const float* x0, const float* x1, const float* x2, const float* weights, float* out, int64_t n,
                     void* stream);
int nbm_weighted_sum_bwd(const float* x0, const float* x1, const float* x2, const float* weights, const float* g, float* gx0,
                         float* gx1, float* gx2, float* gw, int64_t n, void* stream);
/* Targeted re-zeroing of a gradient map [B][H][W][C] (C % 4 == 0) that is zero except for known footprints -- the gradient of
 * a demand-driven FPN map (training): what RoiPooling's backward scattered into the windows of level `lvl` (the windows of
 * nbm_roi_pool_bwd, one shared device function; a window with no pixel in the map zeroes nothing), what the stride-`stride` depthwise convolution's backward added on its 3x3 blocks (layers.py:62-65), and
 * the 2x2 tiles of a list (layout of nbm_roi_tiles; n_blocks optional device count).  The map can then be kept across steps
 * instead of being filled (12.6 + 18.9 GB per step at B = 128) -- there is no reference counterpart, autograd allocates. */
int nbm_zero_roi_windows(float* g, int H, int W, int C, const float* rois /*[B][n_roi][4]*/, const int* level /*[B][n_roi]*/,
                         int B, int n_roi, int lvl, void* stream);
int nbm_zero_pattern(float* g, int B, int H, int W, int C, int stride, void* stream);
int nbm_zero_tiles(float* g, int B, int H, int W, int C, const int* tiles, int n_entries, const int* n_blocks, void* stream);
/* the 2x2 tiles of such a list <-> compact [n_entries][2][2][C] in list order (the compact output layout of
 * nbm_wino23_conv_fused_tiles): gather reads the map (zeros outside the image), scatter_add adds the compact values into it (every
 * tile listed once).  The RoI share of the finest level's lateral gradients runs on these compact operands. */
int nbm_tiles_gather(const float* map, int B, int H, int W, int C, const int* tiles, int n_entries, const int* n_blocks, float* compact,
                     void* stream);
int nbm_tiles_scatter_add(float* map, int B, int H, int W, int C, const int* tiles, int n_entries, const int* n_blocks,
                          const float* compact, void* stream);
/* out[n] = sum_m g[m][n] (bias gradients) */
int nbm_colsum(const float* g, int64_t M, int N, int ld, float* out, void* stream);
int nbm_maxpool3x3s2_bwd(const uint8_t* idx, const float* gy, float* gx, int B, int H, int W, int C, int Ho, int Wo,
                         const float* residual /* [B][H][W][C], optional: added to gx (another consumer's gradient) */,
                         const float* mask /* [B][H][W][C], optional: gx *= (mask > 0), after the addition -- the pooled tensor is a
                                              ReLU output (backbone.py:131) and its producer need not mask the gradient again */,
                         void* stream);
/* out = gy * (y > 0 ? 1 : slope) -- nn.LeakyReLU backward (Transformer_RCNN embeddings / DETR-style feed-forward) */
int nbm_leaky_relu_bwd(const float* gy, const float* y, float* out, float slope, int64_t n, void* stream);
/* nn.LayerNorm backward over rows of E <= 1024 floats; gw, gb (E floats each) must be zeroed, they are added to */
int nbm_layernorm_bwd(const float* x, const float* w, const float* g, int64_t rows, int E, float eps, float* gx, float* gw,
                      float* gb, void* stream);
/* backward of nbm_mha_small: gq/gk/gv get every VALID token row written (pre-zero them when *n_valid < S);
 * workspace: 2*S*S floats per (batch entry, head), whatever hd (<= 512) and S (<= 1024; 8 MiB per (entry, head) there) */
int nbm_mha_small_bwd(const float* q, const float* k, const float* v, const float* go, int q_ld, int k_ld, int v_ld,
                      int go_ld, float* gq, float* gk, float* gv, int gq_ld, int gk_ld, int gv_ld, float* workspace, int S,
                      int N, int nhead, int hd, int64_t seq_stride, int64_t batch_stride, const int32_t* n_valid,
                      float scale, void* stream);
/* ---- dropout of the Transformer_RCNN head in training mode, `--tf_rcnn --dropout p` (csrc/dropout.hip, csrc/mha.hip).  A mask is a pure function
 * of (seed, call, site_id, element index) -- Philox4x32-10, csrc/nbm_philox.h: counter (q & 0xffffffff, q >> 32, site_id, call) with
 * q = element index >> 2, key = (low, high) half of `seed`, element i takes output word i & 3 and is kept iff word >= threshold
 * (threshold = round(p * 2^32)); a kept element is multiplied by `scale` = float32(1) / float32(1 - p), computed by the caller.
 * Nothing is stored: a backward pass evaluates the same mask again.  ops.dropout_keep_reference (NumPy) states the mask and the
 * kernels agree with it bit for bit.
 *
 * nbm_dropout: y[i] = (residual ? residual[i] : 0) + (keep(i) ? x[i] * scale : 0), i < n, each product and sum rounded to float32 on
 * its own (no fused multiply-add).  One Philox evaluation and one 16-byte access per four elements, a scalar tail for n % 4.  With
 * residual == NULL it is also its own backward pass (the incoming gradient takes the place of x); the residual branch passes the
 * gradient through.  n <= 0 or a missing x / y: NBM_EINVAL; x, y or residual not 16-byte aligned: NBM_EALIGN.
 * Replaces: `src + self.dropout1(src2)`, `self.dropout(self.activation(...))` and `src + self.dropout2(src2)` of both encoder
 *   layers in training mode -- self_attention.py:132-135 (`--tf_pe_qk`) and nn.TransformerEncoderLayer (layers.py:619-621) -- and
 *   what autograd derives for them. */
int nbm_dropout(const float* x, const float* residual, float* y, int64_t n, uint32_t threshold, float scale, uint64_t seed,
                uint32_t call, uint32_t site_id, void* stream);
/* nbm_mha_small with dropout on the softmax probabilities: A[r][j] = keep ? (e_j / sum) * drop_scale : 0, out = A V.  Token layout,
 * *n_valid handling, limits (S <= 1024, hd <= 512) and argument checks are nbm_mha_small's.  The mask element of (batch entry n,
 * head h, query r, key j) is ((n * nhead + h) * S + r) * S + j -- a dense [N][nhead][S][S] tensor, S the launch's S whatever
 * *n_valid holds.
 * Replaces: nn.MultiheadAttention(dropout=p) in training mode, self_attention.py:113,131 / layers.py:619-621. */
int nbm_mha_small_drop(const float* q, const float* k, const float* v, int q_ld, int k_ld, int v_ld, float* out, int out_ld,
                       int S, int N, int nhead, int hd, int64_t seq_stride, int64_t batch_stride, const int32_t* n_valid,
                       float scale, uint32_t threshold, float drop_scale, uint64_t seed, uint32_t call, uint32_t site_id,
                       void* stream);
/* backward of nbm_mha_small_drop (arguments, workspace, S <= 1024 and hd <= 512 of nbm_mha_small_bwd): dA = dO V^T, dP = keep ? dA * drop_scale : 0,
 * dS = P (dP - sum_j P dP), dQ = scale dS K, dK = scale dS^T Q, dV = A^T dO.
 * Replaces: autograd through nn.MultiheadAttention(dropout=p), train.py:212. */
int nbm_mha_small_drop_bwd(const float* q, const float* k, const float* v, const float* go, int q_ld, int k_ld, int v_ld,
                           int go_ld, float* gq, float* gk, float* gv, int gq_ld, int gk_ld, int gv_ld, float* workspace, int S,
                           int N, int nhead, int hd, int64_t seq_stride, int64_t batch_stride, const int32_t* n_valid,
                           float scale, uint32_t threshold, float drop_scale, uint64_t seed, uint32_t call, uint32_t site_id,
                           void* stream);
/* nbm_layernorm_bwd with the parameter gradients summed in a fixed order (no atomics; gw, gb are written, not added to): two
 * calls on the same inputs give the same bits, which the dropout path promises for a (seed, call) pair.  gx holds the bits of
 * nbm_layernorm_bwd.  workspace: min(ceil(rows / 4), 256) * 8 * E floats or more (previous contents never read); a smaller one,
 * E > 1024 or a missing pointer: NBM_EINVAL.
 * Replaces: autograd through norm1 / norm2 of the encoder layers, self_attention.py:133,136 / layers.py:619-621 (train.py:212). */
int nbm_layernorm_bwd_det(const float* x, const float* w, const float* g, int64_t rows, int E, float eps, float* gx, float* gw,
                          float* gb, float* workspace, int64_t workspace_floats, void* stream);
/* gradient of the bilinear (align_corners) up-sampling of fpn.py:143-144 wrt the coarse map [B][Hi][Wi][C], gather form.
 * pattern_stride = S >= 5: the caller guarantees that gy [B][Ho][Wo][C] is zero outside the 5x5 patches around the 3x3 / stride-S /
 * pad-1 pattern (rows and columns o*S - 2 .. o*S + 2): those rows / columns are not read (61 % of the map at S = 8); 0: every
 * pixel is read.  nbm_tiles_upsample_bilinear_bwd_add: the same operator in scatter form for the 2x2 tiles of a list (layout of
 * nbm_roi_tiles, ids relative to [B][Ho][Wo]) held as compact [n_entries][2][2][C] values (nbm_wino23_conv_fused_tiles), ADDED
 * into gsrc with fp32 atomics -- the RoI share of the same gradient, a few % of the map. */
int nbm_upsample_bilinear_bwd(const float* gy, int B, int Hi, int Wi, int C, float* gsrc, int Ho, int Wo, int pattern_stride,
                              void* stream);
int nbm_tiles_upsample_bilinear_bwd_add(const float* compact, int B, int Ho, int Wo, int C, const int* tiles, int n_entries,
                                        const int* n_blocks, float* gsrc, int Hi, int Wi, void* stream);
int nbm_softmax_rows_bwd(const float* p, const float* gp, float* out, int64_t rows, int cols, float alpha, void* stream);
int nbm_pair_softmax_bwd(const float* y, const float* gy, float* gx, int64_t n_pairs, void* stream);
/* depthwise 3x3 gradients: gx (may be NULL), gw [Cout][9] and gb [Cout] (gw NULL = skip both) */
int nbm_dwconv3x3_bwd(const float* x, const float* g, const float* w, int B, int H, int W, int Cin, int mult, int stride,
                      float* gx, float* gw, float* gb, int Ho, int Wo, void* stream);
/* the data gradient of the same depthwise convolution ADDED into gx, which already holds the gradient another consumer of the
 * map sent (the RoI pooling's scatter map, nbm_roi_pool_bwd): only the pixels a tap reaches are touched -- replaces a dense
 * write, a dense zero fill and autograd's dense add for an FPN map with these two consumers */
int nbm_dwconv3x3_bwd_acc(const float* g, const float* w, int B, int H, int W, int Cin, int mult, int stride, float* gx, int Ho,
                          int Wo, void* stream);
int nbm_film_fwd(const float* z, const float* film, float* y, int64_t n_pix, int C, void* stream);
int nbm_film_bwd(const float* gy, const float* z, const float* film, float* gz, float* gfilm, int64_t n_pix, int C,
                 void* stream);
/* nn.BatchNorm2d in training mode over rows [M][C]: batch statistics (biased variance for the output, unbiased for the
 * running estimate), running stats updated in place with `momentum`.  stats_ws / red_ws: 2*C doubles. */
int nbm_bn_train_fwd(const float* x, int64_t M, int C, const float* w, const float* b, float eps, float momentum,
                     float* run_mean, float* run_var, double* stats_ws, float* mean, float* invstd, float* y, void* stream);
int nbm_bn_train_bwd(const float* g, const float* x, int64_t M, int C, const float* mean, const float* invstd,
                     const float* w, double* red_ws, float* gx, float* gw, float* gb, void* stream);
/* ---- live BatchNorm of the backbone (csrc/bnorm.hip): nn.BatchNorm2d in training mode over rows [M][C] (NHWC, M = B*H*W), with
 * the residual add and the ReLU that follow it in a bottleneck in the same passes:
 *   forward : mean[c], invstd[c] = batch statistics (biased variance), y = act((z - mean) * invstd * gamma + beta (+ residual)),
 *             act = ReLU when `relu`; run_mean / run_var (both or neither) <- (1 - momentum) * old + momentum * new, the variance
 *             unbiased (M / (M - 1)) for M > 1.  Two passes over z (reduce, apply) and one write of y.
 *   backward: g' = gy * (y > 0) with `relu` (y: the forward output; may be NULL without relu), else g' = gy;
 *             gbeta = sum g', ggamma = sum g' * xhat, gz = gamma * invstd * (g' - gbeta / M - xhat * ggamma / M),
 *             gres (optional) = g'.  Two passes over (gy, y, z).
 * Every sum is carried in double: one partial per workgroup, stored to a slot of `workspace`, and a finish kernel sums the slots in a
 * fixed ascending order.  No atomics, no zero fill: the previous contents of `workspace` are never read, two runs give the same
 * bits.  nbm_bn_act_plan: host only, no HIP call; *parts = the number of slots, *workspace_bytes = what both calls need, functions of
 * (M, C) alone.  All offsets are 64-bit; every global access of the streaming kernels is a 16-byte access.
 * C % 4 != 0: NBM_EUNSUPPORTED; a pointer that is not 16-byte aligned: NBM_EALIGN; M < 1, C < 1, a missing pointer, a workspace
 * smaller than the plan's: NBM_EINVAL.  Nothing is launched then.
 *
 * Replaces: `nn.BatchNorm2d` as the body's norm layer, reference backbone.py:125-126 (`--norm_layer_backbone batchnorm`), with the
 *   ReLU / `out += identity` of torchvision's Bottleneck behind it, and what autograd derives for them (train.py:212). */
int nbm_bn_act_plan(int64_t M, int C, int* parts, int64_t* workspace_bytes);
int nbm_bn_act_train_fwd(const float* z, int64_t M, int C, const float* gamma, const float* beta, float eps, float momentum,
                         float* run_mean, float* run_var, const float* residual, int relu, void* workspace, int64_t workspace_bytes,
                         float* mean, float* invstd, float* y, void* stream);
int nbm_bn_act_train_bwd(const float* gy, const float* y, const float* z, int64_t M, int C, const float* mean, const float* invstd,
                         const float* gamma, int relu, void* workspace, int64_t workspace_bytes, float* gz, float* ggamma,
                         float* gbeta, float* gres, void* stream);
/* ROIPooling backward at any pool size (autograd of layers.py:406-497 with --roi_pool_h / --roi_pool_w): scatter-add of
 * gpool [B*n_roi][pool_h][pool_w][C] into the given gradient maps, windows and bins of nbm_roi_pool_hw on the levels in
 * `level`.  The sums are fp32 atomics: RoI windows overlap, so their order -- and the last bits of the result -- is not fixed.
 * Argument checks as nbm_roi_pool_hw. */
int nbm_roi_pool_hw_bwd(float* const* gfmap_host, const int* fh_host, const int* fw_host, int n_levels, int C,
                        const float* rois, const int* level, int B, int n_roi, int pool_h, int pool_w, const float* gpool,
                        void* stream);
/* Deterministic twin, gather form: a workgroup owns a 16 x 16 pixel tile of one level and image, walks the image's RoIs in index order and
 * adds each RoI's shares for the pixels inside its window (the same window function), one read-modify-write per touched element and no
 * atomic.  Pixels outside every window are not written (the footprint of nbm_zero_roi_windows holds).  Work grows linearly with n_roi. */
int nbm_roi_pool_hw_bwd_det(float* const* gfmap_host, const int* fh_host, const int* fw_host, int n_levels, int C,
                            const float* rois, const int* level, int B, int n_roi, int pool_h, int pool_w, const float* gpool,
                            void* stream);
/* nbm_roi_pool_hw_bwd with pool_h = pool_w = 2 (gpool [B*n_roi][2][2][C]): same kernel, same argument checks */
int nbm_roi_pool_bwd(float* const* gfmap_host, const int* fh_host, const int* fw_host, int n_levels, int C,
                     const float* rois, const int* level, int B, int n_roi, const float* gpool, void* stream);
/* out[0] += sum g^2 (double); then AdamW on a flat range with the clip coefficient min(1, max_norm/(sqrt(*sqnorm)+1e-6))
 * evaluated on device (sqnorm NULL or max_norm <= 0: no clipping). */
int nbm_sqnorm_accum(const float* g, int64_t n, double* out, void* stream);
int nbm_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                   float weight_decay, int step, const double* sqnorm, float max_norm, void* stream);

/* ---- training-input stage: Img_dataset (reference nbm_datasets/image_dataset.py:36-96) ------------------------- */
/* per-image augmentation draws, filled by the host in the reference's RNG call order (image_dataset.py:59,68,71-81,90) */
struct nbm_augment_params {
  float gain;                 /* np.random.uniform(-0.1, 0.35)                                   :68 */
  float coef, denom;          /* hard-negative weight c and 1 + c for the positive image         :79-80 */
  float neg_coef, neg_denom;  /* same for the negative image                                      :82-83 */
  int32_t flags;              /* bit 0: bool_transform[0] (hard-negative mix), bit 1: [1] (low-pass) :71 */
  int32_t hard_index;         /* image of `hard` to mix in */
  int32_t pad;
  uint64_t noise_seed;        /* stream of the device counter RNG when noise_unit == NULL */
};

/* PNG scanline reconstruction (filter types 0-4, PNG spec 9.2) of `batch` inflated 8-bit greyscale images:
 * raw[b] = H lines of (1 filter byte + W bytes) -> out[b] = H*W pixels; *status != 0 afterwards <=> bad filter byte.
 * Replaces the pixel half of `imageio.imread` (image_dataset.py:44,62,77); the zlib inflate stays on the host. */
int nbm_png_unfilter_gray8(const uint8_t* raw, int64_t raw_bs, int batch, int H, int W, uint8_t* out, int64_t out_bs,
                           int32_t* status, void* stream);
/* DEFLATE decoder (RFC 1950 / 1951) for the IDAT payloads of `batch` PNG files: the half of `imageio.imread`
 * (image_dataset.py:44,62,77) that nbm_png_unfilter_gray8's comment says "stays on the host", for callers that ship the
 * file bytes instead (Img_dataset(device_inflate=True)).  payload: one packed buffer of payload_bytes bytes; table[b] =
 * {offset, length} (int64 pairs, device memory) of stream b, a whole zlib stream; out[b][0 .. expect) = the inflated
 * bytes, expect = H * (W + 1), exactly what nbm_png_unfilter_gray8 takes as raw (row pitch out_pitch >= expect BYTES;
 * nothing behind the expect bytes of a row is written); status[b] = NBM_OK or one of the codes below, written for every
 * stream.  Stored, fixed and dynamic blocks, any number of them, lengths 3..258, distances 1..32768, overlapping copies;
 * header (CM = 8, window <= 32 KiB, FCHECK; a preset dictionary is refused) and Adler-32 trailer checked; bytes behind
 * the trailer are ignored, like zlib.decompress does.  No input can make the kernel read outside [offset, offset +
 * length) of the payload, write outside out[b][0 .. expect), or run longer than expect + 8 * length steps: a stream that
 * is malformed sets its own status and the others are decoded.  The rows of a failed stream hold unspecified bytes.
 * payload and out 16-byte aligned, every offset and (batch > 1) out_pitch a multiple of 16 (NBM_EALIGN; a bad table row:
 * NBM_INFLATE_ETABLE); expect, length <= 2^30.  One kernel launch on `stream`, one wavefront per stream, no atomics,
 * no workspace (capturable). */
#define NBM_INFLATE_EHEADER 1       /* zlib header: CM != 8, window > 32 KiB, FCHECK wrong or FDICT set */
#define NBM_INFLATE_EBLOCKTYPE 2    /* block type 3 */
#define NBM_INFLATE_ESTORED 3       /* stored block: LEN != ~NLEN */
#define NBM_INFLATE_ECODELENGTHS 4  /* dynamic header: HLIT > 286, HDIST > 30, a repeat with nothing to repeat or past the
                                       announced count, no end-of-block code */
#define NBM_INFLATE_ECODESET 5      /* over-subscribed or incomplete set of code lengths (zlib's rule: incomplete is allowed
                                       only for a literal/length or distance set whose single code has length 1, and for
                                       a distance set without any code) */
#define NBM_INFLATE_ECODE 6         /* a code no symbol owns, literal/length symbol 286 / 287 or distance symbol 30 / 31 */
#define NBM_INFLATE_EDISTANCE 7     /* distance reaches before the first output byte */
#define NBM_INFLATE_EOUTPUT 8       /* the stream inflates to more or fewer than `expect` bytes */
#define NBM_INFLATE_EINPUT 9        /* the payload ends before the stream does */
#define NBM_INFLATE_EADLER 10       /* Adler-32 of the output differs from the trailer */
#define NBM_INFLATE_ETABLE 11       /* table row outside the payload, negative, too long or not 16-byte aligned */
int nbm_png_inflate(const uint8_t* payload, int64_t payload_bytes, const int64_t* table, int batch, uint8_t* out,
                    int64_t out_pitch, int64_t expect, int32_t* status, void* stream);
/* half_std[b] = std(float32(img_b / 255), unbiased) / 2 -- the noise scale of image_dataset.py:66 */
int nbm_image_half_std_u8(const uint8_t* img, int64_t bs, int batch, int64_t n, float* half_std, void* stream);
/* out[i] = i-th N(0,1) draw of counter stream `seed` (splitmix64 + Box-Muller) -- device stand-in for torch.randn :66 */
int nbm_randn_fill(uint64_t seed, int64_t n, float* out, void* stream);
/* the whole `if self.transform:` block (:65-94) for a batch: img = u8/255 (+gain, +clamp(noise*half_std, +-0.5),
 * hard-negative mix, low-pass curve[b][row]); neg = u8/255 (hard-negative mix).  noise_unit (N(0,1) field, may be
 * NULL => device counter RNG), curve [batch][H]. */
int nbm_augment_batch(const uint8_t* pos, const uint8_t* neg, const uint8_t* hard, int batch, int H, int W,
                      const struct nbm_augment_params* params, const float* half_std, const float* noise_unit,
                      const float* curve, float* img_out, float* neg_out, void* stream);
/* out = float32(in / 255) -- `torch.Tensor(img / 255)` :45,63 (transform=False path) */
int nbm_u8_to_unit(const uint8_t* in, int64_t n, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
