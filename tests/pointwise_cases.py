"""The cases of tests/test_gpu_pointwise_edges.py, as data: every case names the code path of csrc/pointwise.hip / csrc/pointwise_bwd.hip
it was chosen for (`path`), and tests/test_pointwise_ref_cpu.py recomputes that path from the host-side dispatch arithmetic, so a case
cannot drift off the path its comment claims.  Shapes are the smallest that reach each path."""

# ----- bilinear: (Hi, Wi, Ho, Wo, C), path = kernel of the backward ('fast' / 'general'), maxc = most contributors of one coarse index
# (rows, columns) under the kernels' own fp32 weights, minc = fewest
BILINEAR = [
    dict(shape=(8, 8, 24, 24, 4), path=dict(kernel='general', maxc=(7, 7))),            # 2/sh = 6.57 > 4.95, 7 contributors: one dropped by a list of 6
    dict(shape=(3, 4, 24, 32, 8), path=dict(kernel='general', maxc=(22, 20))),
    dict(shape=(6, 5, 24, 20, 4), path=dict(kernel='general', maxc=(9, 10))),
    dict(shape=(4, 4, 12, 12, 4), path=dict(kernel='general', maxc=(7, 7))),
    dict(shape=(1, 1, 8, 8, 4), path=dict(kernel='general', maxc=(8, 8), sh0=True, sw0=True)),   # sh == 0: every fine row contributes
    dict(shape=(1, 5, 1, 10, 4), path=dict(kernel='general', maxc=(1, 4), sh0=True, sw0=False)),  # Ho == 1: sh == 0 sends a 2x scale to the general kernel
    dict(shape=(5, 5, 11, 11, 4), path=dict(kernel='general', maxc=(5, 5), two_over_s=5.0)),       # 2/sh = 5.0 > 4.95: first scale past the boundary
    dict(shape=(5, 5, 10, 10, 4), path=dict(kernel='fast', maxc=(4, 4), two_over_s=4.5)),
    dict(shape=(5, 5, 12, 12, 4), path=dict(kernel='general', maxc=(6, 6))),             # exactly one full list
    dict(shape=(24, 32, 3, 4, 8), path=dict(kernel='fast', maxc=(1, 1), minc=(0, 0))),  # down-sampling: coarse rows / columns nobody reads
    dict(shape=(16, 32, 4, 8, 8), path=dict(kernel='fast', maxc=(1, 1), minc=(0, 0))),
    dict(shape=(7, 9, 7, 9, 4), path=dict(kernel='fast', maxc=(1, 1), minc=(1, 1), identity=True)),
    dict(shape=(5, 7, 10, 14, 128), path=dict(kernel='fast', maxc=(4, 4), share=True, ragged=True)),  # SHARE (C4 >= 32), 224 of 256 threads of the one workgroup
    dict(shape=(5, 7, 10, 14, 4), path=dict(kernel='fast', maxc=(4, 4), share=False, ragged=True)),
]
# the module-level case: SelfAttention(32, 32, downscale_factor=4, position_encoding=True) on a 16 x 32 map = down (16,32)->(4,8), up (4,8)->(16,32)
MODULE_CASE = dict(C=32, h=16, w=32, f=4, path=dict(down='fast', up='general', up_maxc=(9, 9)))
# the shape the general kernel is timed at (profiles/pointwise_edges.txt): general, and no index has more than 6 contributors
TIMED = dict(shape=(94, 256, 235, 640, 64), B=8, path=dict(kernel='general', maxc=(5, 5)))

# ----- softmax rows: (rows, cols); path: 'reg' (row in registers, cols <= 1536) / 'stream'; clamp = some lane's load is clamped
# (cols % 64 != 0 or cols < 64 * 24); sweeps = grid-stride iterations of a wave (8192 blocks x 4 rows)
SOFTMAX = [
    dict(rows=5, cols=1, path=dict(branch='reg', clamp=True, sweeps=1)),
    dict(rows=5, cols=63, path=dict(branch='reg', clamp=True, sweeps=1)),
    dict(rows=5, cols=64, path=dict(branch='reg', clamp=True, sweeps=1)),
    dict(rows=5, cols=65, path=dict(branch='reg', clamp=True, sweeps=1)),
    dict(rows=5, cols=1536, path=dict(branch='reg', clamp=False, sweeps=1)),
    dict(rows=5, cols=1537, path=dict(branch='stream', sweeps=1)),
    dict(rows=5, cols=1600, path=dict(branch='stream', sweeps=1)),
    dict(rows=5, cols=4099, path=dict(branch='stream', sweeps=1)),
    dict(rows=33001, cols=8, path=dict(branch='reg', clamp=True, sweeps=2)),             # 33 001 rows > 8192 * 4
]
SOFTMAX_PITCH = dict(rows=7, cols=37, pad=3)

# ----- LayerNorm: E x rows; path: slots = register slots of the backward in use (ceil(E / 64) of 16), idle = waves of the backward
# that meet no row, sweeps = rows a wave of the backward visits at most (256 blocks x 4 waves)
LAYERNORM_E = [1, 24, 64, 65, 1000, 1024]
LAYERNORM_ROWS = [1, 3, 1025]
LAYERNORM_PATH = {
    (1, 1): dict(slots=1, idle=3, sweeps=1), (1024, 1025): dict(slots=16, idle=0, sweeps=2), (65, 3): dict(slots=2, idle=1, sweeps=1),
    (1000, 1025): dict(slots=16, idle=0, sweeps=2), (24, 3): dict(slots=1, idle=1, sweeps=1), (64, 1): dict(slots=1, idle=3, sweeps=1),
}
LAYERNORM_REFUSED_E = 1025

# ----- element-wise sweeps: n items > 4096 * 256 = 1 048 576 (a second grid-stride iteration)
ELEMENTWISE_N = 1050000
ELEMENTWISE = dict(
    n=ELEMENTWISE_N, axpby_period=70, film_C=6, film_pix=175000,                          # 175 000 x 6 = 1 050 000
    pair_anchor=3, pair_ld=8, pair_pix=350000,                                            # 350 000 x 3 pairs, x_ld = 8 > 2 * 3
    init_conv=(2, 350, 500, 3),                                                           # B, H, W, C: 350 000 pixels x 3
)

# ----- weighted sum: raw weights, n; the backward's sweep is capped at 2048 x 256 vectors of 4
WEIGHTED_SUM_W = [(0.7, -0.3, 1.1), (0.0, 0.5), (-1.0, -2.0, -3.0)]
WEIGHTED_SUM_N = [dict(n=4, path=dict(bwd_sweeps=1)), dict(n=2100000, path=dict(bwd_sweeps=2))]      # 525 000 vectors > 524 288

# ----- column reductions (1024 blocks x 4 row lanes; 64 columns per block column)
COLSUM_M = [1, 3, 4099]
COLSUM_N = [1, 63, 65, 130]
COLSUM_PAD = 5
BN_M = [1, 2, 4099]
BN_C = [1, 63, 65, 256]
REDUCE_PATH = {1: dict(sweeps=1, idle_lanes=3), 2: dict(sweeps=1, idle_lanes=2), 3: dict(sweeps=1, idle_lanes=1), 4099: dict(sweeps=2, idle_lanes=0)}
BN_APPLY_SWEEPS = {(4099, 256): 2, (4099, 65): 1}                                         # 4099 x 256 = 1 049 344 > 1 048 576

# ----- max pooling: (B, H, W, C); sweeps of (forward, backward)
MAXPOOL_SMALL = [(1, 1), (1, 5), (2, 2), (3, 2), (2, 7)]
MAXPOOL_BIG = dict(shape=(2, 182, 182, 64), path=dict(fwd_sweeps=1, bwd_sweeps=2))       # backward: 2*182*182*16 = 1 059 968 vectors

# ----- depthwise 3x3: (B, H, W, Cin, mult, stride); path: fwd = 'vec' / 'scalar', fwd_fixed = weights cached across iterations,
# fwd_sweeps, bwd = template of the data kernel, bwd_fixed = its weights cached (w_fixed), row_sweeps = rows a blockIdx.y visits,
# wgrad = 'vec' / 'scalar'
DWCONV = [
    dict(cfg=(2, 96, 96, 128, 2, 1), path=dict(fwd='vec', fwd_fixed=True, fwd_sweeps=2, bwd='<2,hoist>', bwd_fixed=True, wgrad='vec')),
    dict(cfg=(2, 9, 11, 12, 2, 1), path=dict(fwd='vec', fwd_fixed=False, bwd='<2,hoist>', bwd_fixed=False)),
    dict(cfg=(2, 9, 11, 12, 2, 2), path=dict(fwd='vec', fwd_fixed=False, bwd='<2,hoist>', bwd_fixed=False)),
    dict(cfg=(2, 9, 11, 96, 2, 1), path=dict(fwd='vec', fwd_fixed=False, bwd='<2,hoist>', bwd_fixed=False)),
    dict(cfg=(2, 9, 11, 96, 2, 2), path=dict(fwd='vec', fwd_fixed=True, bwd='<2,hoist>', bwd_fixed=False)),   # 12 x 256 % 48 == 0 forward
    dict(cfg=(2, 9, 11, 6, 1, 1), path=dict(fwd='scalar', bwd=None, wgrad='scalar')),     # Cin % 4 != 0: no data gradient kernel (refused), weights only
    dict(cfg=(2, 9, 11, 4, 3, 1), path=dict(fwd='scalar', bwd='<0>', wgrad='scalar')),
    dict(cfg=(2, 1, 7, 8, 2, 1), path=dict(fwd='vec', bwd='<2,hoist>')),
    dict(cfg=(2, 5, 1, 8, 2, 2), path=dict(fwd='vec', bwd='<2,hoist>')),
    dict(cfg=(2, 2, 2, 8, 4, 1), path=dict(fwd='vec', bwd='<4>')),
    dict(cfg=(2, 33000, 2, 4, 2, 2), path=dict(fwd='vec', bwd='<2,hoist>', bwd_fixed=True, row_sweeps=2)),   # 66 000 rows > gridDim.y = 65 535
    dict(cfg=(1, 2, 2, 8, 2, 2), path=dict(fwd='vec', bwd='<2,hoist>', out_pixels=1, wgrad='vec')),
    dict(cfg=(1, 2, 2, 4, 3, 2), path=dict(fwd='scalar', bwd='<0>', out_pixels=1, wgrad='scalar')),
]

# ----- 2x2 average pooling / space to batch: (B, H, W, C) of the full-resolution map; vectors = B*H*W*C/4
AVGPOOL = [
    dict(shape=(2, 2, 2, 4), path=dict(full_sweeps=1)),
    dict(shape=(2, 64, 2052, 16), path=dict(full_sweeps=2)),                             # 1 050 624 vectors > 2^20
]

# ----- optimiser: sqnorm's sweep is capped at 2048 x 256
SQNORM_N = [dict(n=1, path=dict(sweeps=1)), dict(n=600001, path=dict(sweeps=2))]
ADAMW_STEPS = [1, 100000]
