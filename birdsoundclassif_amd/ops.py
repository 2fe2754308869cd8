"""Host-side operator layer: thin wrappers that hand raw device pointers of torch tensors to the
C ABI of libnbm_hip.so on torch's current HIP stream.  torch is plumbing here (HBM allocations,
streams); all arithmetic happens in the hand-written kernels.  Activations are NHWC fp32.

Every function raises if the tensor is not a contiguous float32 CUDA tensor -- there is no CPU path.
"""
import collections
import ctypes as C
import os
import math

import torch

from . import _lib
from ._lib import GconvBwdDesc, GconvDesc, GemmDesc, RoiHwDesc, check

ACT_NONE, ACT_RELU, ACT_SILU, ACT_LEAKY = 0, 1, 2, 3

# bench.py sets this to a list to time every implicit-GEMM launch with HIP events on the launch stream:
# entries are ((Cin, N, kh, H, W, B, groups, stride, label), start_event, end_event).
PROFILE = None
FLOPS = None                   # [float]: executed MFMA FLOPs of every GEMM launch since it was set (bench.py accounting)
FLOPS_DEFERRED = []             # (device counter, FLOPs per count): launches whose size is only known on the device


def flops_total():
    """Executed MFMA FLOPs since `FLOPS = [0.0]` was set (synchronises to read the device-side counts)."""
    tot = FLOPS[0] + sum(float(c.item()) * f for c, f in FLOPS_DEFERRED)
    FLOPS_DEFERRED.clear()
    return tot


_PROFILE_LABEL = None          # set by composite ops (Winograd) so that their GEMM launches can be told apart
PROFILE_ONLY = None             # None: every GEMM-type launch; 'fused': only the fused Winograd kernel; 'deepk': only the deep-K
                                # instantiation of the implicit-GEMM kernel, igemm_kernel<128,128,64,64,A_FAST,EPI_STD,2> (bench.py's
                                # timed loop: event pairs around all ~250 launches of a step cost it 2.5 %)


def _prof_all():
    return PROFILE is not None and PROFILE_ONLY is None


def _prof_fused():
    return PROFILE is not None and PROFILE_ONLY in (None, 'fused')


def is_deepk(Cin, N, kh, kw, rows=None):
    """Does nbm_gemm_conv dispatch this launch to igemm_kernel<128,128,64,64,A_FAST,EPI_STD,STAGES=2> (csrc/igemm.hip: N > 64,
    more than 8 K-steps of 32, channel count a multiple of 32, no row list)?"""
    return rows is None and N > 64 and Cin % 32 == 0 and kh * kw * Cin > 256



def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _chk(t, dtype=torch.float32, name='tensor'):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError(f'{name}: the NBM HIP path needs CUDA (ROCm) tensors; no CPU fallback exists')
    if t.dtype != dtype:
        raise TypeError(f'{name}: expected {dtype}, got {t.dtype}')
    if not t.is_contiguous():
        raise ValueError(f'{name}: must be contiguous')
    return t


def lib():
    return _lib.load()


# --------------------------------------------------------------------------- deterministic mode
# Entry points whose DEFAULT kernels sum with floating-point atomics, and the twin that replaces each of them while the mode is on.
# 'desc': the twin is selected inside the same entry point by descriptor fields (nbm_bwd_desc.workspace); None: no twin -- a call in
# deterministic mode raises.  Every call of these entry points goes through `_reduction`, so the table is the one place a new atomic
# kernel has to be entered (tests/test_deterministic_cpu.py checks the sources against tests/golden/atomic_sites.json).
ATOMIC_ENTRY_POINTS = {
    'nbm_conv_wgrad': 'desc',
    'nbm_stem7x7_wgrad': 'nbm_stem7x7_wgrad_det',
    'nbm_wino_outgrad': 'nbm_wino_outgrad_det',
    'nbm_wino23_outgrad_tiles': 'nbm_wino23_outgrad_tiles_det',
    'nbm_cell_outgrad': 'nbm_cell_outgrad_det',
    'nbm_cell_dgrad_output': 'nbm_cell_dgrad_output_det',
    'nbm_roi_pool_hw_bwd': 'nbm_roi_pool_hw_bwd_det',
    'nbm_roi_pool_bwd': None,                   # (the 2 x 2 alias; the op layer only calls nbm_roi_pool_hw_bwd)
    'nbm_roi_tiles': 'nbm_roi_tiles_det',
    'nbm_colsum': 'nbm_colsum_det',
    'nbm_weighted_sum_bwd': 'nbm_weighted_sum_bwd_det',
    'nbm_dwconv3x3_bwd': 'nbm_dwconv3x3_bwd_det',
    'nbm_bn_train_fwd': 'nbm_bn_train_fwd_det',
    'nbm_bn_train_bwd': 'nbm_bn_train_bwd_det',
    'nbm_sqnorm_accum': 'nbm_sqnorm_accum_det',
    'nbm_layernorm_bwd': 'nbm_layernorm_bwd_det',          # (an entry point of its own since the dropout path: `layernorm_bwd` routes)
    'nbm_tiles_upsample_bilinear_bwd_add': None,           # deterministic mode routes through the dense nbm_upsample_bilinear_bwd
}
DET_COLSUM, DET_SQNORM, DET_BN, DET_WEIGHTED_SUM, DET_DWCONV = range(5)      # nbm_det_workspace's `op`

_DET = {'on': False, 'torch': None, 'saved': None, 'ws': {}}


def deterministic():
    """Is the process in deterministic mode (`set_deterministic`)?"""
    return _DET['on']


def _det_refusals():
    """Options whose kernels have no deterministic twin: -> [(option, why)]."""
    bad = []
    if os.environ.get('NBM_SPLIT_BF16') == '1':
        bad.append(('NBM_SPLIT_BF16=1', 'the split-bf16 weight-gradient kernel (igemm_split_tn.hip) adds its pixel splits with atomics'))
    return bad


class _DetScope:
    """What `set_deterministic` returns: usable as a context manager that restores the previous state on exit."""

    def __init__(self, previous):
        self.previous = previous

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        set_deterministic(self.previous)


def set_deterministic(flag):
    """Switch the process-wide deterministic mode (train.py --deterministic).  On: every entry point of ATOMIC_ENTRY_POINTS runs
    its twin (no atomics, fixed summation order), the demand-driven routes whose kernels have none are routed densely
    (`ondemand.set_deterministic_routes`) and torch.use_deterministic_algorithms(True) holds; off: all of that is restored.  An option
    that is not covered is refused by name (ValueError).  -> a context manager restoring the previous state (`with
    set_deterministic(True): ...`); calling it plainly just switches."""
    flag = bool(flag)
    previous = _DET['on']
    if flag == previous:
        return _DetScope(previous)
    from . import ondemand
    if flag:
        bad = _det_refusals()
        if bad:
            raise ValueError('--deterministic does not cover ' + '; '.join(f'{o} ({why})' for o, why in bad))
        _DET['torch'] = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
        torch.use_deterministic_algorithms(True)
        _DET['saved'] = ondemand.set_deterministic_routes(True)
        _DET['on'] = True
    else:
        _DET['on'] = False
        ondemand.set_deterministic_routes(False, _DET['saved'])
        torch.use_deterministic_algorithms(_DET['torch'][0], warn_only=_DET['torch'][1])
        _DET['torch'] = _DET['saved'] = None
        _DET['ws'].clear()
    return _DetScope(previous)


def _det_workspace(nbytes, device=None):
    """The twins' slot workspace: one growing buffer per stream (launches on a stream are ordered, so consecutive twins share it); never
    zeroed, its contents are never read before they are written."""
    key = torch.cuda.current_stream().cuda_stream
    buf = _DET['ws'].get(key)
    if buf is None or buf.numel() < nbytes:
        buf = None
        _DET['ws'][key] = None
        buf = torch.empty((max(int(nbytes), 1 << 20),), device=device or 'cuda', dtype=torch.uint8)
        _DET['ws'][key] = buf
    return buf


def det_workspace_bytes():
    """Bytes currently held by the deterministic twins' workspaces (all streams)."""
    return sum(b.numel() for b in _DET['ws'].values() if b is not None)


def _det_bytes(op, rows, cols=1):
    n = C.c_int64(0)
    check(lib().nbm_det_workspace(int(op), int(rows), int(cols), C.byref(n)), 'nbm_det_workspace')
    return n.value


def _bias_ws_bytes(N):
    n = C.c_int64(0)
    check(lib().nbm_bias_grad_workspace(int(N), C.byref(n)), 'nbm_bias_grad_workspace')
    return n.value


def roi_tiles(*args):
    """nbm_roi_tiles on the current stream (args: everything but the stream; args[2] is the image count) -- in deterministic mode its
    twin, which places the 128-entry blocks by a prefix over the images instead of an atomic counter."""
    if not _DET['on']:
        return check(lib().nbm_roi_tiles(*args, _stream()), 'nbm_roi_tiles')
    counts = _det_workspace(4 * int(args[2]))
    return check(lib().nbm_roi_tiles_det(*args, _ptr(counts), _stream()), 'nbm_roi_tiles_det')


def _reduction(name, args, ws_bytes=None):
    """Call entry point `name` of ATOMIC_ENTRY_POINTS with `args` (everything but the stream) on the current stream -- in deterministic
    mode its twin, with `ws_bytes()` bytes of slot workspace appended where the twin takes one (ws_bytes None: it takes none)."""
    twin = ATOMIC_ENTRY_POINTS[name]
    if not _DET['on']:
        return check(getattr(lib(), name)(*args, _stream()), name)
    if twin == 'desc':
        raise TypeError(f'{name} selects its twin through descriptor fields: call it through its op-layer wrapper')
    if twin is None:
        raise RuntimeError(f'{name} is not reproducible under --deterministic')
    if ws_bytes is None:
        return check(getattr(lib(), twin)(*args, _stream()), twin)
    nbytes = int(ws_bytes())
    ws = _det_workspace(nbytes)
    return check(getattr(lib(), twin)(*args, _ptr(ws), nbytes, _stream()), twin)


# --------------------------------------------------------------------------- implicit GEMM
def gemm_conv(x, w, y, *, B, H, W, Cin, N, kh=1, kw=1, stride=1, pad=0, Ho=None, Wo=None,
              x_ld=None, w_ld=None, y_ld=None, scale=None, shift=None, residual=None, res_ld=None,
              groups=1, x_gs=0, w_gs=0, y_gs=0, res_gs=0, alpha=1.0, act=ACT_NONE, shift_per_row=False, up=None,
              rows=None, rows_mode=0, rows_count=0, rows_blocks=None, rows_thw=(0, 0), mask=None, mask_ld=None, bits_out=None):
    """Raw call of nbm_gemm_conv (see include/nbm_hip.h for the exact semantics).  `bits_out` (int32 [M * N / 32]): one bit per stored
    output element, (y > 0) -- the ReLU mask of the consumer's data gradient (`conv_dgrad(mask_bits=)`)."""
    Ho = (H + 2 * pad - kh) // stride + 1 if Ho is None else Ho
    Wo = (W + 2 * pad - kw) // stride + 1 if Wo is None else Wo
    d = GemmDesc()
    d.x, d.w, d.y = x.data_ptr(), w.data_ptr(), y.data_ptr()
    d.scale = scale.data_ptr() if scale is not None else None
    d.shift = shift.data_ptr() if shift is not None else None
    d.residual = residual.data_ptr() if residual is not None else None
    d.x_gs, d.w_gs, d.y_gs, d.res_gs = x_gs, w_gs, y_gs, res_gs
    d.groups = groups
    d.B, d.H, d.W, d.Cin, d.N = B, H, W, Cin, N
    d.kh, d.kw, d.stride, d.pad, d.Ho, d.Wo = kh, kw, stride, pad, Ho, Wo
    d.x_ld = Cin if x_ld is None else x_ld
    d.w_ld = kh * kw * Cin if w_ld is None else w_ld
    d.y_ld = N if y_ld is None else y_ld
    d.res_ld = (N if res_ld is None else res_ld) if residual is not None else 0
    d.alpha, d.act, d.shift_per_row = float(alpha), int(act), int(bool(shift_per_row))
    if up is not None:                       # [B, up_H, up_W, N] coarse map merged in the epilogue
        d.up, d.up_H, d.up_W = _chk(up, name='up').data_ptr(), up.shape[1], up.shape[2]
    if mask is not None:                     # producer mask: y = 0 where mask <= 0 (a 1x1 data gradient run as a forward GEMM)
        d.mask, d.mask_ld = mask.data_ptr(), int(N if mask_ld is None else mask_ld)
    if bits_out is not None:
        assert bits_out.dtype == torch.int32 and bits_out.is_contiguous() and bits_out.numel() * 32 >= B * Ho * Wo * N and N % 32 == 0
        d.bits_out = bits_out.data_ptr()
    if rows is not None:                     # listed pixels only (the lateral of a demand-driven FPN level)
        d.rows, d.rows_mode, d.rows_count = rows.data_ptr(), int(rows_mode), int(rows_count)
        d.rows_blocks = rows_blocks.data_ptr() if rows_blocks is not None else None
        d.rows_TH, d.rows_TW = rows_thw
    if FLOPS is not None:
        if rows is None:
            FLOPS[0] += 2.0 * B * Ho * Wo * N * kh * kw * Cin * groups
        elif rows_blocks is None:
            FLOPS[0] += 2.0 * rows_count * N * Cin
        else:
            FLOPS_DEFERRED.append((rows_blocks.clone(), 2.0 * 128 * (16 if rows_mode == 2 else 1) * N * Cin))
    if _prof_all() or (PROFILE is not None and PROFILE_ONLY == 'deepk' and is_deepk(Cin, N, kh, kw, rows)):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        check(lib().nbm_gemm_conv(C.byref(d), _stream()), 'nbm_gemm_conv')
        ev1.record()
        if rows is None:
            PROFILE.append(((Cin, N, kh, H, W, B, groups, stride, _PROFILE_LABEL), ev0, ev1))
        elif rows_blocks is None:                  # listed pixels: M = the list
            PROFILE.append(((Cin, N, kh, rows_count, 1, 1, groups, stride, ('rows', H, W)), ev0, ev1))
        else:                                      # device-side count
            PROFILE.append(((Cin, N, kh, 0, 1, 1, groups, stride, ('rows-rois', H, W)), ev0, ev1))
        return y
    check(lib().nbm_gemm_conv(C.byref(d), _stream()), 'nbm_gemm_conv')
    return y


def conv2d(x, w, kh=1, kw=1, stride=1, pad=0, scale=None, shift=None, residual=None, act=ACT_NONE,
           alpha=1.0, out=None, w_ld=None, up=None, bits_out=None):
    """x [B,H,W,Cin] NHWC, w [N, w_ld>=kh*kw*Cin] (KRSC rows) -> [B,Ho,Wo,N]; `up` [B,h,w,N]: + bilinear(up)."""
    _chk(x, name='x'), _chk(w, name='w')
    B, H, W, Cin = x.shape
    N = w.shape[0]
    Ho = (H + 2 * pad - kh) // stride + 1
    Wo = (W + 2 * pad - kw) // stride + 1
    y = out if out is not None else torch.empty((B, Ho, Wo, N), device=x.device, dtype=torch.float32)
    if residual is not None:
        _chk(residual, name='residual')
        assert residual.shape == y.shape
    gemm_conv(x, w, y, B=B, H=H, W=W, Cin=Cin, N=N, kh=kh, kw=kw, stride=stride, pad=pad, Ho=Ho, Wo=Wo,
              w_ld=w.shape[1] if w_ld is None else w_ld, scale=scale, shift=shift, residual=residual,
              alpha=alpha, act=act, up=up, bits_out=bits_out)
    return y


def gconv3x3(x, w_prepared, groups, stride=1, scale=None, shift=None, relu=False, out=None, kh=3, kw=3, pad=1):
    """Grouped 3x3 / pad 1 convolution (+ per-channel scale / shift, ReLU) of an NHWC map.  `w_prepared` = `_prep.gconv(weight, groups)`,
    [C / 16, 9, max(Cg, 16) / 16, 64, 4] with C = groups * Cg; x [B,H,W,x_ld >= C] (channels beyond C are pitch) -> [B,Ho,Wo,C], or into
    `out` [B,Ho,Wo,y_ld >= C] (its channels beyond C are left alone).  What the kernel does not implement raises (kh, kw and pad are
    only there to be refused): there is no slow path."""
    _chk(x, name='x'), _chk(w_prepared, name='w_prepared')
    if x.dim() != 4 or w_prepared.dim() != 5 or tuple(w_prepared.shape[1::2]) != (9, 64) or w_prepared.shape[4] != 4 or groups <= 0 \
            or (16 * w_prepared.shape[0]) % groups:
        raise ValueError('gconv3x3: x must be [B,H,W,C] and w_prepared the output of _prep.gconv for these groups')
    B, H, W, x_ld = x.shape
    n_ch = 16 * w_prepared.shape[0]
    Cg = n_ch // groups
    if max(Cg, 16) != 16 * w_prepared.shape[2]:
        raise ValueError(f'gconv3x3: w_prepared {tuple(w_prepared.shape)} does not belong to {groups} groups of {Cg} channels')
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    y = out if out is not None else torch.empty((B, Ho, Wo, n_ch), device=x.device, dtype=torch.float32)
    _chk(y, name='out')
    if y.dim() != 4 or tuple(y.shape[:3]) != (B, Ho, Wo) or y.shape[3] < n_ch or x_ld < n_ch:
        raise ValueError(f'gconv3x3: out must be [{B},{Ho},{Wo},>={n_ch}] and x at least {n_ch} channels wide')
    for v, nm in ((scale, 'scale'), (shift, 'shift')):
        if v is not None and _chk(v, name=nm).numel() != n_ch:
            raise ValueError(f'gconv3x3: {nm} must hold {n_ch} values')
    d = GconvDesc()
    d.x, d.w, d.y = x.data_ptr(), w_prepared.data_ptr(), y.data_ptr()
    d.scale = scale.data_ptr() if scale is not None else None
    d.shift = shift.data_ptr() if shift is not None else None
    d.B, d.H, d.W, d.groups, d.Cg = B, H, W, groups, Cg
    d.kh, d.kw, d.stride, d.pad, d.Ho, d.Wo = kh, kw, stride, pad, Ho, Wo
    d.x_ld, d.y_ld, d.relu = x_ld, y.shape[3], int(bool(relu))
    if FLOPS is not None:
        FLOPS[0] += 2.0 * 9 * Cg * n_ch * B * Ho * Wo         # algorithmic: the block-diagonal zeros of Cg < 16 are not counted
    if _prof_all():
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        check(lib().nbm_gconv3x3(C.byref(d), _stream()), 'nbm_gconv3x3')
        ev1.record()
        PROFILE.append(((Cg, n_ch, kh, H, W, B, groups, stride, 'gconv'), ev0, ev1))
        return y
    check(lib().nbm_gconv3x3(C.byref(d), _stream()), 'nbm_gconv3x3')
    return y


WINO_CHUNK_BYTES = 24 << 30          # cap of the transformed-domain scratch (V + M) per batch chunk
_WINO_SCRATCH = {}

# Lanes: detect steps that are IN FLIGHT TOGETHER on one GPU (parallel branches of one captured graph, one stream each:
# bulk.GraphedDetector(lanes=k)) fill each other's kernel tails.  Everything a step allocates through torch is its own; what is shared
# process-wide and WRITTEN by kernels -- the persistent transformed-domain scratch here, the RoI tile-list buffers of ondemand.py -- is
# keyed by the lane that is current while the step is issued (`with ops.lane(k)` around a branch's warm-up and capture).
LANE = 0


class lane:
    def __init__(self, k):
        self.k = int(k)

    def __enter__(self):
        global LANE
        self.prev, LANE = LANE, self.k

    def __exit__(self, *exc):
        global LANE
        LANE = self.prev


def _wino_scratch(device, n_v, n_m):
    """Two views (V: n_v floats, M: n_m floats) of ONE persistent per-device scratch allocation.  Every Winograd call on
    a device runs on the same stream, so reusing the buffer is stream-ordered; a fresh multi-GB torch.empty per call made
    the caching allocator fall back to hipMalloc / hipFree (100 ms host stalls per training step).  The buffer is sized to
    what the largest call so far needed (<= WINO_CHUNK_BYTES by construction of the batch chunks) and grows geometrically:
    a B = 1 detect process holds 0.4 GB, not the 24 GB a B = 64 step uses."""
    need = n_v + n_m
    key = (device, LANE)
    buf = _WINO_SCRATCH.get(key)
    if buf is None or buf.numel() < need:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('the persistent Winograd scratch would have to grow during a graph capture (the warm-up steps of the '
                               'capture must run the same shapes under the same ops.lane)')
        have = 0 if buf is None else buf.numel()
        _WINO_SCRATCH[key] = buf = None          # release before growing
        size = min(max(need, 2 * have), max(need, WINO_CHUNK_BYTES // 4))
        buf = _WINO_SCRATCH[key] = torch.empty((size,), device=device, dtype=torch.float32)
    return buf[:n_v], buf[n_v:need]


GRAPH_NODE_KINDS = ('kernel', 'memcpy', 'memset', 'host', 'empty', 'other')


def graph_census(raw_graph):
    """{node kind: count} of a captured hipGraph_t (`torch.cuda.CUDAGraph(keep_graph=True).raw_cuda_graph()`), nbm_graph_census."""
    counts = (C.c_longlong * 6)()
    check(_lib.load().nbm_graph_census(C.c_void_p(int(raw_graph)), C.byref(counts)), 'nbm_graph_census')
    return dict(zip(GRAPH_NODE_KINDS, (int(v) for v in counts)))


def lane_buffers(lanes):
    """The persistent scratch / tile-list tensors of the given lanes AS THEY ARE NOW: a captured graph bakes their raw addresses in, so
    its owner keeps these references -- a later growth (`_wino_scratch` drops the dict entry before it allocates the larger buffer) or
    `release_lane_scratch` then cannot hand the memory a live graph writes to to another tensor."""
    from . import ondemand
    held = [buf for key, buf in _WINO_SCRATCH.items() if key[1] in lanes and buf is not None]
    for key, bufs in ondemand._ROI_TILE_BUF.items():
        if key[2] in lanes:
            held.extend(bufs)
    return held


def release_lane_scratch(keep=(0,)):
    """Frees the persistent scratch and tile-list buffers of every lane not in `keep` (tens of GB at B = 64).  Only when no captured
    graph that was issued in those lanes is alive any more: a graph keeps the raw addresses."""
    from . import ondemand
    for key in [k for k in _WINO_SCRATCH if k[1] not in keep]:
        del _WINO_SCRATCH[key]
    for key in [k for k in ondemand._ROI_TILE_BUF if k[2] not in keep]:
        del ondemand._ROI_TILE_BUF[key]


def conv3x3_winograd(x, U, bias=None, m=2, scale=None, relu=False, mask=None, residual=None):
    """3x3 / stride 1 / pad 1 convolution through Winograd F(m x m, 3x3): x [B,H,W,C], U [(m+2)^2,N,C] from
    `_prep.wino23` -> [B,H,W,N].  m = 2 (the forward setting, error ~3e-6): row half of the input transform (2x the input
    in HBM), then ONE kernel that finishes the input transform while staging its operand, runs the 16 transformed-domain
    GEMMs on the fp32 MFMA and applies the output transform + epilogue in its accumulators (csrc/wino_fused.hip; neither
    the transformed input V nor the products M ever reach HBM).  m = 4 (backward only, ~2e-5, see csrc/winograd.hip): input
    transform, 36 grouped GEMMs, output transform.  2.25x / 4x fewer multiplies than the direct kernel.  The batch is cut
    so that the transformed operands stay within WINO_CHUNK_BYTES.  Epilogue: y = relu?((.) * scale + bias), zeroed where
    mask <= 0."""
    _chk(x, name='x'), _chk(U, name='U')
    B, H, W, C_ = x.shape
    N = U.shape[1]
    nxi = (m + 2) ** 2
    assert U.shape == (nxi, N, C_) and C_ % 32 == 0 and N % 4 == 0
    y = torch.empty((B, H, W, N), device=x.device, dtype=torch.float32)
    tiles = (-(-H // m)) * (-(-W // m))
    fused = m == 2 and C_ >= 64                  # the fused pipeline wants >= 2 K-steps per plane (every real layer has)
    assert residual is None or m == 4, 'residual: F(4x4,3x3) output transform only' 
    if fused:                                     # R: four row-combination images, 2 (TW + 1) columns per tile row
        per_img = 4 * (-(-H // 2)) * (2 * (-(-W // 2)) + 2) * C_ * 4
    else:
        per_img = nxi * tiles * (C_ + N) * 4
    chunk = max(1, min(B, WINO_CHUNK_BYTES // per_img))
    if fused:
        V, M = _wino_scratch(x.device, chunk * per_img // 4, 0)
    else:
        V, M = _wino_scratch(x.device, nxi * chunk * tiles * C_, nxi * chunk * tiles * N)
    st = _stream()
    if _prof_all():                       # whole-op bracket (transforms + GEMMs) next to the per-GEMM entries
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    for b0 in range(0, B, chunk):
        nb = min(chunk, B - b0)
        T = nb * tiles
        mk = _ptr(mask[b0:b0 + nb]) if mask is not None else None
        if fused:
            check(lib().nbm_wino23_rows(_ptr(x[b0:b0 + nb]), nb, H, W, C_, _ptr(V), st), 'nbm_wino23_rows')
            if FLOPS is not None:
                FLOPS[0] += 2.0 * nxi * T * C_ * N
            if _prof_fused():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            check(lib().nbm_wino23_conv_fused(_ptr(V), _ptr(U), _ptr(scale), _ptr(bias), mk, int(relu), nb, H, W, C_, N,
                                              _ptr(y[b0:b0 + nb]), 0, st), 'nbm_wino23_conv_fused')     # variant 0: automatic tile width
            if _prof_fused():
                e1.record()
                PROFILE.append(((C_, N, 1, T, 1, 1, nxi, 1, ('wino23', H, W)), e0, e1))
            continue
        check(lib().nbm_wino_input(_ptr(x[b0:b0 + nb]), nb, H, W, C_, _ptr(V), m, st), 'nbm_wino_input')
        global _PROFILE_LABEL
        _PROFILE_LABEL = ('wino23', H, W)
        try:
            gemm_conv(V, U, M, B=1, H=T, W=1, Cin=C_, N=N, groups=nxi, x_gs=T * C_, w_gs=N * C_, y_gs=T * N)
        finally:
            _PROFILE_LABEL = None
        check(lib().nbm_wino_output(_ptr(M), _ptr(scale), _ptr(bias), mk, int(relu), nb, H, W, N, _ptr(y[b0:b0 + nb]), m,
                                    _ptr(residual[b0:b0 + nb]) if residual is not None else None, st), 'nbm_wino_output')
    if _prof_all():
        ev[1].record()
        PROFILE.append((('wino23', C_, N, H, W, B), *ev))
    return y


def wino_weight(weight, transposed=False, m=2, scale=None):
    """[N,C,3,3] -> U [(m+2)^2, N', C'] = G g' G^T (float64 arithmetic on the device, rounded once); `transposed`: the
    data-gradient convolution's weights (rotated kernel, swapped channel roles, optional per-output-channel `scale`)."""
    _chk(weight, name='weight')
    N, C_ = weight.shape[:2]
    assert tuple(weight.shape[2:]) == (3, 3)
    No, Co = (C_, N) if transposed else (N, C_)
    U = torch.empty(((m + 2) ** 2, No, Co), device=weight.device, dtype=torch.float32)
    check(lib().nbm_wino_weight(_ptr(weight), _ptr(scale), N, C_, int(bool(transposed)), m, _ptr(U), _stream()),
          'nbm_wino_weight')
    return U


def wino_weight_grad(dU, m=2, row_scale=None):
    """dU [(m+2)^2, N, C] -> dW [N, C, 3, 3] = row_scale[n] * G^T dU G."""
    _chk(dU, name='dU')
    _, N, C_ = dU.shape
    dW = torch.empty((N, C_, 3, 3), device=dU.device, dtype=torch.float32)
    check(lib().nbm_wino_weight_grad(_ptr(dU), _ptr(row_scale), N, C_, m, _ptr(dW), _stream()), 'nbm_wino_weight_grad')
    return dW


def cell_weight(weight, forward=True, lateral=None, alpha=1.0, both=False):
    """Kernel side of the cell transforms (csrc/cellwino.hip, float64 on the device, one rounding): [N,C,3,3] -> U = E w E^T as
    [25][N][K] (`forward`: B operand of the forward plane GEMMs) or [25][K][N] (data-gradient GEMMs); `both`: (forward, transposed).
    `lateral` = KRSC weights [C][Cin] of a deferred lateral 1x1: K = C + Cin, the extra columns / rows hold alpha * U W_lat."""
    _chk(weight, name='weight')
    N, C_ = weight.shape[:2]
    assert tuple(weight.shape[2:]) == (3, 3)
    Cin = 0
    if lateral is not None:
        _chk(lateral, name='lateral')
        assert lateral.shape[0] == C_
        Cin = lateral.shape[1]
    K = C_ + Cin
    Unc = torch.empty((25, N, K), device=weight.device, dtype=torch.float32) if (forward or both) else None
    Ucn = torch.empty((25, K, N), device=weight.device, dtype=torch.float32) if (not forward or both) else None
    check(lib().nbm_cell_weight(_ptr(weight), N, C_, _ptr(Unc), K, _ptr(Ucn), K, _stream()), 'nbm_cell_weight')
    if lateral is not None:
        check(lib().nbm_cell_weight_fold(_ptr(weight), _ptr(lateral), lateral.stride(0), N, C_, Cin, float(alpha), _ptr(Unc), K,
                                         _ptr(Ucn), K, _stream()), 'nbm_cell_weight_fold')
    return (Unc, Ucn) if both else (Unc if forward else Ucn)


def copy_rect(strided, base_off, packed, n_outer, outer_pitch, n_rows, row_pitch, width, to_strided=False, zero=False):
    """nbm_copy_rect on a flat fp32 tensor `strided` (element offset `base_off` of the rectangle's first float) and a contiguous
    `packed` [n_outer * n_rows * width]; counts in floats."""
    assert strided.dtype == torch.float32 and packed.dtype == torch.float32 and packed.is_contiguous()
    assert packed.numel() >= n_outer * n_rows * width
    assert base_off + (n_outer - 1) * outer_pitch + (n_rows - 1) * row_pitch + width <= strided.numel()
    check(lib().nbm_copy_rect(C.c_void_p(strided.data_ptr() + 4 * base_off), _ptr(packed), n_outer, outer_pitch, n_rows, row_pitch, width,
                              int(bool(to_strided)), int(bool(zero)), _stream()), 'nbm_copy_rect')
    return packed


def cell_weight_grad(dU):
    """dU [25, N, K >= C] (columns beyond C ignored when `dU` is a [..., :C] view) -> dW [N, C, 3, 3] = E^T dU E."""
    assert dU.dim() == 3 and dU.shape[0] == 25 and dU.stride(2) == 1 and dU.stride(0) == dU.shape[1] * dU.stride(1)
    _, N, C_ = dU.shape
    dW = torch.empty((N, C_, 3, 3), device=dU.device, dtype=torch.float32)
    check(lib().nbm_cell_weight_grad(_ptr(dU), N, C_, dU.stride(1), _ptr(dW), _stream()), 'nbm_cell_weight_grad')
    return dW


def conv3x3_winograd_wgrad(x, g, want_bias=False, m=2):
    """Weight gradient of a 3x3 / s1 / p1 convolution in the Winograd domain: x [B,H,W,C] (forward input), g [B,H,W,N]
    (gradient wrt the output) -> (dU [(m+2)^2,N,C] with dU[xi] = dM[xi]^T V[xi], bias gradient [N] or None).  The caller
    maps dU back with dW = G^T dU G (`_prep.wino23_weight_grad`)."""
    _chk(x, name='x'), _chk(g, name='g')
    B, H, W, C_ = x.shape
    N = g.shape[-1]
    nxi = (m + 2) ** 2
    assert g.shape[:3] == x.shape[:3] and C_ % 4 == 0 and N % 4 == 0
    tiles = (-(-H // m)) * (-(-W // m))
    per_img = nxi * tiles * (C_ + N) * 4
    chunk = max(1, min(B, WINO_CHUNK_BYTES // per_img))
    V, dM = _wino_scratch(x.device, nxi * chunk * tiles * C_, nxi * chunk * tiles * N)
    dU = torch.zeros((nxi, N, C_), device=x.device, dtype=torch.float32)
    gb = torch.zeros((N,), device=x.device, dtype=torch.float32) if want_bias else None
    st = _stream()
    for b0 in range(0, B, chunk):
        nb = min(chunk, B - b0)
        T = nb * tiles
        check(lib().nbm_wino_input(_ptr(x[b0:b0 + nb]), nb, H, W, C_, _ptr(V), m, st), 'nbm_wino_input')
        _reduction('nbm_wino_outgrad', (_ptr(g[b0:b0 + nb]), nb, H, W, N, _ptr(dM), _ptr(gb), m), lambda: _bias_ws_bytes(N))
        conv_wgrad(dM, V, dU, B=1, H=T, W=1, Cin=C_, N=N, groups=nxi, g_gs=T * N, x_gs=T * C_, out_gs=N * C_)
    return dU, gb


def linear(x2d, w, bias=None, act=ACT_NONE, out=None, alpha=1.0, residual=None, y_ld=None):
    """x2d [M,K], w [N,K] -> [M,N] (= x @ w.T + bias)."""
    _chk(x2d, name='x'), _chk(w, name='w')
    M, K = x2d.shape
    N = w.shape[0]
    y = out if out is not None else torch.empty((M, N), device=x2d.device, dtype=torch.float32)
    gemm_conv(x2d, w, y, B=1, H=M, W=1, Cin=K, N=N, w_ld=w.shape[1], shift=bias, act=act, alpha=alpha,
              residual=residual, y_ld=y_ld)
    return y


def bgemm_nt(a, b, out=None, alpha=1.0, shift=None, shift_per_row=False, residual=None, act=ACT_NONE):
    """a [G,M,K] (or [M,K] shared by all groups), b [G,N,K] -> [G,M,N] = alpha * a @ b^T (+shift)(+residual)."""
    _chk(a, name='a'), _chk(b, name='b')
    G, N, K = b.shape
    M = a.shape[-2]
    assert a.shape[-1] == K
    a_gs = M * K if a.dim() == 3 else 0
    y = out if out is not None else torch.empty((G, M, N), device=b.device, dtype=torch.float32)
    gemm_conv(a, b, y, B=1, H=M, W=1, Cin=K, N=N, w_ld=K, groups=G, x_gs=a_gs, w_gs=N * K, y_gs=M * N,
              alpha=alpha, shift=shift, shift_per_row=shift_per_row, residual=residual,
              res_gs=M * N if residual is not None else 0, act=act)
    return y


# --------------------------------------------------------------------------- front end
def pcm16_to_wave(pcm, out_ld, lead, upsample, hq=None, reflect=False, first=0, count=None):
    """pcm int16 [batch, n] -> f32 [batch, out_ld]: `lead` padding samples, the piece [first, first + count) of the
    44.1 kHz signal (the input itself, or its 2x up-sampling when `upsample`; default: all of it), `lead` padding
    samples, zeros.  Padding = zeros (librosa >= 0.10 `pad_mode='constant'`) or the mirrored piece (`reflect`,
    librosa <= 0.9)."""
    _chk(pcm, torch.int16, 'pcm')
    batch, n = pcm.shape
    if count is None:
        count = (2 * n if upsample else n) - first
    out = torch.empty((batch, out_ld), device=pcm.device, dtype=torch.float32)
    if upsample:
        _chk(hq, torch.int32, 'hq')
    check(lib().nbm_pcm16_to_wave(_ptr(pcm), n, batch, n, int(bool(upsample)), _ptr(hq), first, count, _ptr(out), out_ld,
                                  lead, int(bool(reflect)), _stream()), 'nbm_pcm16_to_wave')
    return out


WAV_FORMATS = ((1, 8), (1, 16), (1, 24), (1, 32), (3, 32), (3, 64))      # (resolved format tag, bits) nbm_wav_decode takes
WAV_MAX_CHANNELS = 8


def wav_decode(raw, tag, bits, channels, n, out=None):
    """raw uint8 [batch, pitch] (device; every row the interleaved sample bytes of a wav `data` payload, n frames) ->
    f32 [batch, n] mono samples, bit for bit what `prepare_dataset.read_wav` returns for those bytes.  `tag` is the
    resolved format tag (`bulk.wav_header`).  `out`: f32 rows to write into (unit stride along a row, row pitch >= n;
    what lies behind the n samples of a row is left alone)."""
    if not (isinstance(raw, torch.Tensor) and raw.is_cuda):
        raise RuntimeError('raw: the NBM HIP path needs CUDA (ROCm) tensors; no CPU fallback exists')
    if raw.dtype != torch.uint8 or raw.dim() != 2 or raw.stride(1) != 1:
        raise TypeError('raw: expected uint8 [batch, pitch] rows with unit stride')
    if (int(tag), int(bits)) not in WAV_FORMATS or not 1 <= channels <= WAV_MAX_CHANNELS:
        raise NotImplementedError(f'wav format tag {tag} with {bits} bits per sample and {channels} channels')
    batch = raw.shape[0]
    if n < 1 or n * channels * (bits // 8) > raw.shape[1]:
        raise ValueError(f'{n} frames do not fit rows of {raw.shape[1]} bytes')
    if out is None:
        out = torch.empty((batch, n), device=raw.device, dtype=torch.float32)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] == batch and out.shape[1] >= n
              and out.stride(1) == 1):
        raise TypeError('out: expected f32 [batch, >= n] rows with unit stride on the device')
    check(lib().nbm_wav_decode(_ptr(raw), raw.stride(0) if batch > 1 else raw.shape[1], batch, int(tag), int(bits),
                               int(channels), int(n), _ptr(out), out.stride(0) if batch > 1 else out.shape[1], _stream()),
          'nbm_wav_decode')
    return out[:, :n]


INFLATE_STATUS = {1: 'bad zlib header', 2: 'bad block type', 3: 'stored block length check failed',
                  4: 'bad code lengths in a dynamic header', 5: 'over-subscribed or incomplete code set',
                  6: 'invalid code', 7: 'distance reaches before the start of the output',
                  8: 'inflated size differs from the image size', 9: 'payload ends before the stream does',
                  10: 'Adler-32 mismatch', 11: 'bad payload table row'}       # NBM_INFLATE_* of include/nbm_hip.h


def png_payload_pack(streams):
    """Host only.  list of bytes (one zlib stream each) -> (uint8 array holding them back to back, int64 [n, 2] table of
    (offset, length)).  Every stream starts on a 16-byte boundary and the array ends at least 8 bytes behind the last
    stream (zeros), so an 8-byte read at any payload byte stays inside it; its size is a multiple of 16."""
    import numpy as np
    table = np.zeros((len(streams), 2), dtype=np.int64)
    off = 0
    for i, s in enumerate(streams):
        table[i] = off, len(s)
        off += (len(s) + 15) // 16 * 16
    packed = np.zeros(((off + 8 + 15) // 16 * 16,), dtype=np.uint8)
    for (o, n), s in zip(table, streams):
        packed[o:o + n] = np.frombuffer(s, dtype=np.uint8)
    return packed, table


def png_inflate(payload, table, H, W, out=None, status=None):
    """payload uint8 [bytes] (device: `png_payload_pack`'s array), table int64 [n, 2] (host: numpy or CPU tensor) ->
    (raw uint8 [n, H * (W + 1)], status int32 [n]), both on the device: the filtered scanlines `zlib.decompress` returns
    for every stream whose status is 0 (`INFLATE_STATUS` names the others; this call does not read the status back).
    `raw` is a view of rows whose pitch is a multiple of 16: hand its stride(0) on.  `out`: such rows to write into
    (uint8 [>= n, pitch >= H * (W + 1)], unit stride along a row); `status`: int32 [n] on the device to write into."""
    if not (isinstance(payload, torch.Tensor) and payload.is_cuda):
        raise RuntimeError('payload: the NBM HIP path needs CUDA (ROCm) tensors; no CPU fallback exists')
    _chk(payload, torch.uint8, 'payload')
    table = torch.as_tensor(table)
    if table.is_cuda or table.dtype != torch.int64 or table.dim() != 2 or table.shape[1] != 2:
        raise ValueError('table: expected int64 [n, 2] (offset, length) rows on the host')
    n, expect = table.shape[0], int(H) * (int(W) + 1)
    if payload.dim() != 1 or n < 1 or H < 1 or W < 1 or expect > 1 << 30:
        raise ValueError(f'payload [{tuple(payload.shape)}], {n} streams, {H} x {W}: shapes that cannot be right')
    if payload.data_ptr() % 16:
        raise ValueError('payload: must start on a 16-byte boundary')
    off, length = table[:, 0], table[:, 1]
    if bool((off % 16 != 0).any()):
        raise ValueError('table: every stream must start on a 16-byte boundary of the payload')
    if bool((off < 0).any()) or bool((length < 0).any()) or bool((off + length > payload.numel()).any()):
        raise ValueError(f'table: a stream lies outside the payload of {payload.numel()} bytes')
    if out is None:
        out = torch.empty((n, (expect + 15) // 16 * 16), dtype=torch.uint8, device=payload.device)
    elif not (out.is_cuda and out.dtype == torch.uint8 and out.dim() == 2 and out.shape[0] >= n and out.shape[1] >= expect
              and out.stride(1) == 1 and out.data_ptr() % 16 == 0 and (n == 1 or out.stride(0) % 16 == 0)):
        raise ValueError('out: expected 16-byte aligned uint8 [>= n, >= H * (W + 1)] rows on the device, pitch a multiple of 16')
    if status is None:
        status = torch.empty((n,), dtype=torch.int32, device=payload.device)
    elif _chk(status, torch.int32, 'status').shape != (n,):
        raise ValueError(f'status: expected int32 [{n}]')
    table_dev = table.contiguous().pin_memory().to(payload.device, non_blocking=True)     # pinned: the copy may outlive `table`
    check(lib().nbm_png_inflate(_ptr(payload), payload.numel(), _ptr(table_dev), n, _ptr(out),
                                out.stride(0) if n > 1 else out.shape[1], expect, _ptr(status), _stream()), 'nbm_png_inflate')
    return out[:n, :expect], status


def resample_to_wave(x, out_ld, lead, L, M, taps, reflect=False, first=0, count=None, quant16=True):
    """x f32 [batch, n] at any rate -> f32 [batch, out_ld] laid out like `pcm16_to_wave`: the piece [first, first+count)
    of the 44.1 kHz signal = x itself (L = M = 1) or its rational L / M polyphase resampling with the float64 `taps`
    [L, T] (rounded to the 16-bit grid when `quant16`)."""
    _chk(x, torch.float32, 'x')
    batch, n = x.shape
    n_out = n if (L == 1 and M == 1) else -(-n * L // M)
    if count is None:
        count = n_out - first
    if taps is not None:
        _chk(taps, torch.float64, 'taps')
        assert taps.shape[0] == L
    out = torch.empty((batch, out_ld), device=x.device, dtype=torch.float32)
    check(lib().nbm_resample_to_wave(_ptr(x), n, batch, n, L, M, _ptr(taps), taps.shape[1] if taps is not None else 0, first,
                                     count, _ptr(out), out_ld, lead, int(bool(reflect)), int(bool(quant16)), _stream()),
          'nbm_resample_to_wave')
    return out


def stft_db(wave, n_frames, hop, n_fft, basis, n_bins, floor_amp, db_ld=None, out=None, col0=0):
    """wave f32 [batch, wave_ld] (already centre-padded) -> (db [batch, n_bins, db_ld], minmax u32 [batch,2]).
    `basis`: float64 [bin tiles, k steps, 64, 2] in MFMA fragment order (prepare_dataset.dft_basis_f64).
    `out=(db, minmax)` + `col0`: write the frames at column offset col0 of an existing spectrogram and keep accumulating
    its min/max (chunked STFT of a long file, reference prepare_dataset.py:234-237)."""
    _chk(wave, name='wave'), _chk(basis, torch.float64, 'basis')
    batch, wave_ld = wave.shape
    if out is None:
        db_ld = n_frames if db_ld is None else db_ld
        db = torch.empty((batch, n_bins, db_ld), device=wave.device, dtype=torch.float32)
        mm = torch.empty((batch, 2), device=wave.device, dtype=torch.int32)
        check(lib().nbm_minmax_init(_ptr(mm), batch, _stream()), 'nbm_minmax_init')
    else:
        db, mm = out
        db_ld = db.shape[-1]
        assert col0 + n_frames <= db_ld and db.shape[0] == batch
    check(lib().nbm_stft_db(_ptr(wave), wave_ld, batch, n_frames, hop, n_fft, _ptr(basis), basis.shape[0],
                            basis.shape[1], n_bins, float(floor_amp), C.c_void_p(db.data_ptr() + 4 * col0),
                            n_bins * db_ld, db_ld, _ptr(mm), _stream()), 'nbm_stft_db')
    return db, mm


def spec_windows(db, minmax, n_frames, n_img, w_pix, hop_img, last_cols):
    """db [batch, n_bins, db_ld] + min/max -> img [batch, n_img, n_bins, w_pix] normalised to [0,1]; the last window
    reads the columns `last_cols` (int32 [w_pix] on the device)."""
    _chk(db, name='db'), _chk(last_cols, torch.int32, 'last_cols')
    assert last_cols.numel() == w_pix
    batch, n_bins, db_ld = db.shape
    img = torch.empty((batch, n_img, n_bins, w_pix), device=db.device, dtype=torch.float32)
    check(lib().nbm_spec_windows(_ptr(db), n_bins * db_ld, db_ld, batch, n_bins, n_frames, _ptr(minmax), _ptr(img),
                                 n_img, w_pix, hop_img, _ptr(last_cols), _stream()), 'nbm_spec_windows')
    return img


WINDOW_ENTRY_WORDS = 5         # struct nbm_window_entry as int64 words: db, minmax, last_cols, (db_ld | n_frames << 32), (window | n_img << 32)


def window_entry(db, minmax, last_cols, window, n_img):
    """One row of a `spec_windows_table` table (np.int64 [5]) for window `window` of the file whose dB plane is db
    [n_bins, n_frames] (a contiguous view of its own storage, e.g. spectrogram_db(...)[0][0]), min/max int32 [2] and last-window
    columns int32 [w_pix] (all on the device).  The raw addresses go into the table: the caller keeps these tensors alive until
    every launch that reads the table has run."""
    import numpy as np
    _chk(db, name='db'), _chk(last_cols, torch.int32, 'last_cols')
    if db.dim() != 2 or db.stride(1) != 1 or minmax.dtype != torch.int32 or minmax.numel() != 2 or not minmax.is_contiguous():
        raise ValueError('window_entry: db [n_bins, n_frames] with unit column stride, minmax int32 [2]')
    if not 0 <= window < n_img:
        raise ValueError('window_entry: window index outside the file')
    lo = lambda a, b: (int(a) & 0xffffffff) | (int(b) << 32)
    return np.array([db.data_ptr(), minmax.data_ptr(), last_cols.data_ptr(), lo(db.stride(0), db.shape[1]), lo(window, n_img)],
                    dtype=np.int64)


def spec_windows_table(table, n_bins, w_pix, hop_img, out=None):
    """table int64 [B, WINDOW_ENTRY_WORDS] on the device (rows from `window_entry`; an all-zero row is a padding slot) ->
    img [B, n_bins, w_pix]: the windows nbm_spec_windows cuts, bit for bit, padding slots zeroed (nbm_spec_windows_table)."""
    _chk(table, torch.int64, 'table')
    if table.dim() != 2 or table.shape[1] != WINDOW_ENTRY_WORDS:
        raise ValueError(f'window table of shape {tuple(table.shape)}: expected (B, {WINDOW_ENTRY_WORDS})')
    B = table.shape[0]
    img = out if out is not None else torch.empty((B, n_bins, w_pix), device=table.device, dtype=torch.float32)
    _chk(img, name='img')
    assert tuple(img.shape) == (B, n_bins, w_pix)
    check(lib().nbm_spec_windows_table(_ptr(table), B, n_bins, _ptr(img), w_pix, hop_img, _stream()), 'nbm_spec_windows_table')
    return img


# --------------------------------------------------------------------------- point-wise stages
def init_conv(x, w, b):
    """x [B,H,W,1] -> [B,H,W,C]."""
    _chk(x, name='x')
    C_ = w.numel()
    y = torch.empty(x.shape[:3] + (C_,), device=x.device, dtype=torch.float32)
    check(lib().nbm_init_conv(_ptr(x), x.numel(), _ptr(_chk(w.reshape(-1))), _ptr(_chk(b)), C_, _ptr(y), _stream()),
          'nbm_init_conv')
    return y


def stem7x7(img, weff, wb, wb_full, scale, shift):
    """img [B,H,W,1] (or [B,H,W]) -> relu(scale * conv7x7/s2/p3(init_conv(img)) + shift) [B,Ho,Wo,64]; the folded operands
    come from `_prep.stem_fold`."""
    _chk(img, name='img')
    B, H, W = img.shape[:3]
    assert img.numel() == B * H * W and tuple(weff.shape) == (56, 64)
    y = torch.empty((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64), device=img.device, dtype=torch.float32)
    if FLOPS is not None:
        FLOPS[0] += 2.0 * y.numel() * 56
    if _prof_all():
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    check(lib().nbm_stem7x7(_ptr(img), B, H, W, _ptr(_chk(weff)), _ptr(_chk(wb)), _ptr(_chk(wb_full)), _ptr(_chk(scale)),
                            _ptr(_chk(shift)), _ptr(y), _stream()), 'nbm_stem7x7')
    if _prof_all():
        ev[1].record()
        PROFILE.append(((1, 64, 7, H, W, B, 1, 2, None), *ev))
    return y


def stem7x7_wgrad(img, g):
    """img [B,H,W,1], g [B,Ho,Wo,64] (ReLU-masked output gradient) -> (U [64,7,7], V [64,7,7]): sums of g times the image sample /
    the inside-the-image indicator under every tap (csrc/stem.hip)."""
    _chk(img, name='img'), _chk(g, name='g')
    B, H, W = img.shape[:3]
    assert g.shape == (B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64)
    D = torch.empty((64, 64), device=img.device, dtype=torch.float32)
    Cb = torch.empty((64, 49), device=img.device, dtype=torch.float32)
    def ws_bytes():
        n = C.c_int64(0)
        check(lib().nbm_stem7x7_wgrad_workspace(B, H, W, C.byref(n)), 'nbm_stem7x7_wgrad_workspace')
        return n.value
    _reduction('nbm_stem7x7_wgrad', (_ptr(img), _ptr(g), B, H, W, _ptr(D), _ptr(Cb)), ws_bytes)
    U = D[:, :56].view(64, 7, 8)[:, :, :7]
    V = D[:, 56].view(64, 1, 1) - Cb.view(64, 7, 7)
    return U, V


def maxpool3x3s2(x, with_index=False):
    """-> y, or (y, idx uint8 [B,Ho,Wo,C]: window position of each maximum, for `maxpool3x3s2_bwd`)."""
    _chk(x, name='x')
    B, H, W, C_ = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty((B, Ho, Wo, C_), device=x.device, dtype=torch.float32)
    idx = torch.empty((B, Ho, Wo, C_), device=x.device, dtype=torch.uint8) if with_index else None
    check(lib().nbm_maxpool3x3s2(_ptr(x), B, H, W, C_, _ptr(y), Ho, Wo, _ptr(idx), _stream()), 'nbm_maxpool3x3s2')
    return (y, idx) if with_index else y


def space_to_batch2(x, inverse=False):
    """x [B,H,W,C] (H, W even) -> [4B,H/2,W/2,C]: the four parity classes of the pixels as four images (class 2a+b major); `inverse`:
    [4B,h,w,C] -> [B,2h,2w,C].  A 3x3 / dilation-2 / pad-2 convolution on x is the ordinary 3x3 / pad-1 convolution on this form."""
    _chk(x, name='x')
    if inverse:
        B4, h, w, C_ = x.shape
        assert B4 % 4 == 0
        B, H, W = B4 // 4, 2 * h, 2 * w
        y = torch.empty((B, H, W, C_), device=x.device, dtype=torch.float32)
    else:
        B, H, W, C_ = x.shape
        if (H | W) & 1:
            raise NotImplementedError('space_to_batch2 needs even map sizes (the dilated ResNet stage at 24 x 64)')
        y = torch.empty((4 * B, H // 2, W // 2, C_), device=x.device, dtype=torch.float32)
    check(lib().nbm_space_to_batch2(_ptr(x), B, H, W, C_, _ptr(y), int(bool(inverse)), _stream()), 'nbm_space_to_batch2')
    return y


def avgpool2x2(x):
    """x [B,2h,2w,C] -> [B,h,w,C]: mean of each 2x2 block (nn.AdaptiveAvgPool2d to half the size)."""
    _chk(x, name='x')
    B, H, W, C_ = x.shape
    assert H % 2 == 0 and W % 2 == 0
    y = torch.empty((B, H // 2, W // 2, C_), device=x.device, dtype=torch.float32)
    check(lib().nbm_avgpool2x2(_ptr(x), B, H // 2, W // 2, C_, _ptr(y), _stream()), 'nbm_avgpool2x2')
    return y


def avgpool2x2_bwd(gy):
    _chk(gy, name='gy')
    B, Ho, Wo, C_ = gy.shape
    gx = torch.empty((B, 2 * Ho, 2 * Wo, C_), device=gy.device, dtype=torch.float32)
    check(lib().nbm_avgpool2x2_bwd(_ptr(gy), B, Ho, Wo, C_, _ptr(gx), _stream()), 'nbm_avgpool2x2_bwd')
    return gx


def upsample_bilinear_add(src, Ho, Wo, add=None):
    _chk(src, name='src')
    B, Hi, Wi, C_ = src.shape
    if add is not None:
        _chk(add, name='add')
        assert tuple(add.shape) == (B, Ho, Wo, C_)
    y = torch.empty((B, Ho, Wo, C_), device=src.device, dtype=torch.float32)
    check(lib().nbm_upsample_bilinear_add(_ptr(src), B, Hi, Wi, C_, _ptr(add), _ptr(y), Ho, Wo, _stream()),
          'nbm_upsample_bilinear_add')
    return y


def softmax_rows_(x2d):
    _chk(x2d, name='x')
    rows, cols = x2d.shape
    check(lib().nbm_softmax_rows(_ptr(x2d), rows, cols, cols, _stream()), 'nbm_softmax_rows')
    return x2d


def dwconv3x3(x, w, bias, mult, stride=1, film=None):
    """x [B,H,W,Cin], w [Cin*mult,1,3,3] (reference layout) -> [B,Ho,Wo,Cin*mult]; film [B*Ho*Wo, 2*Cout]."""
    _chk(x, name='x'), _chk(w, name='w')
    B, H, W, Cin = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    y = torch.empty((B, Ho, Wo, Cin * mult), device=x.device, dtype=torch.float32)
    film_ld = 0
    if film is not None:
        _chk(film, name='film')
        film_ld = film.shape[-1]
    check(lib().nbm_dwconv3x3(_ptr(x), B, H, W, Cin, mult, stride, _ptr(w), _ptr(bias), _ptr(film), film_ld, _ptr(y),
                              Ho, Wo, _stream()), 'nbm_dwconv3x3')
    return y


def dwconv_pool_slots(C_, Ho, Wo):
    """Slots per image of the pool partials `dwconv_bn_act(pool=True)` writes for an output map of Ho x Wo x C."""
    n = lib().nbm_dwconv_pool_slots(int(C_), int(Ho), int(Wo))
    if n <= 0:
        check(n, 'nbm_dwconv_pool_slots')
    return n


def dwconv_bn_act(x, w_taps, k, stride=1, scale=None, shift=None, act=ACT_NONE, pool=False):
    """Depthwise k x k / stride / pad (k - 1) / 2 convolution of x [B,H,W,C] (k in {3, 5}, stride in {1, 2}, C % 4 == 0; what the kernel
    does not implement raises: there is no slow path), y = act(conv * scale + shift).  `w_taps` [k * k, C] = `_prep.dw_taps(weight)`.
    -> y [B,Ho,Wo,C], or with `pool` (y, part [B, slots, C]): every slot holds one workgroup's sum of y per channel (`se_gate` adds the
    slots in a fixed order; a fresh tensor per call, fully written by the kernel)."""
    _chk(x, name='x'), _chk(w_taps, name='w_taps')
    if x.dim() != 4 or tuple(w_taps.shape) != (k * k, x.shape[3]):
        raise ValueError(f'dwconv_bn_act: x must be [B,H,W,C] and w_taps [{k * k}, C], got {tuple(x.shape)} and {tuple(w_taps.shape)}')
    B, H, W, C_ = x.shape
    p = (k - 1) // 2
    Ho, Wo = (H + 2 * p - k) // stride + 1, (W + 2 * p - k) // stride + 1
    for v, nm in ((scale, 'scale'), (shift, 'shift')):
        if v is not None and _chk(v, name=nm).numel() != C_:
            raise ValueError(f'dwconv_bn_act: {nm} must hold {C_} values')
    y = torch.empty((B, Ho, Wo, C_), device=x.device, dtype=torch.float32)
    part = torch.empty((B, dwconv_pool_slots(C_, Ho, Wo), C_), device=x.device, dtype=torch.float32) if pool and C_ % 4 == 0 else None
    check(lib().nbm_dwconv_bn_act(_ptr(x), B, H, W, C_, int(k), int(stride), _ptr(w_taps), _ptr(scale), _ptr(shift), int(act), _ptr(y),
                                  Ho, Wo, _ptr(part), _stream()), 'nbm_dwconv_bn_act')
    return (y, part) if pool else y


def se_gate(part, hw, w1, b1, w2, b2, wproj=None, w_ld=None, out=None):
    """Squeeze-and-excitation gate from the pool partials of `dwconv_bn_act`: part [B, slots, C], hw = Ho * Wo of the pooled map, w1
    [Csq, C], b1 [Csq], w2 [C, Csq], b2 [C] -> gate [B, C] = sigmoid(w2 silu(w1 mean + b1) + b2).  With `wproj` [N, >= C] (KRSC rows of the
    project 1x1): (gate, wb [B, N, w_ld]) with wb[b, n, c] = wproj[n, c] * gate[b, c], w_ld = C rounded up to 32 (pad columns zero); `out`:
    write wb there instead of into a fresh tensor."""
    for t, nm in ((part, 'part'), (w1, 'w1'), (b1, 'b1'), (w2, 'w2'), (b2, 'b2')):
        _chk(t, name=nm)
    B, n_slots, C_ = part.shape
    Csq = b1.numel()
    if w1.numel() != Csq * C_ or w2.numel() != Csq * C_ or b2.numel() != C_:
        raise ValueError(f'se_gate: weights do not fit {C_} channels squeezed to {Csq}')
    gate = torch.empty((B, C_), device=part.device, dtype=torch.float32)
    wb, N, wp_ld = None, 0, 0
    if wproj is not None:
        _chk(wproj, name='wproj')
        N, wp_ld = wproj.shape
        w_ld = (C_ + 31) // 32 * 32 if w_ld is None else int(w_ld)
        wb = torch.empty((B, N, w_ld), device=part.device, dtype=torch.float32) if out is None else _chk(out, name='out')
        if tuple(wb.shape) != (B, N, w_ld):
            raise ValueError(f'se_gate: out must be [{B}, {N}, {w_ld}]')
    check(lib().nbm_se_gate(_ptr(part), B, n_slots, C_, 1.0 / float(hw), _ptr(w1), _ptr(b1), Csq, _ptr(w2), _ptr(b2), _ptr(gate),
                            _ptr(wproj), wp_ld, N, _ptr(wb), int(w_ld or 0), _stream()), 'nbm_se_gate')
    return (gate, wb) if wproj is not None else gate


def conv1x1_per_image(x, wb, N, scale=None, shift=None, residual=None, act=ACT_NONE):
    """1x1 convolution with ONE WEIGHT MATRIX PER IMAGE: x [B,H,W,C], wb [B, N, w_ld] (`se_gate`) -> [B,H,W,N] =
    act(x_b wb_b^T * scale + shift + residual): nbm_gemm_conv with groups = B (scale / shift are not strided by group)."""
    _chk(x, name='x'), _chk(wb, name='wb')
    B, H, W, C_ = x.shape
    if wb.dim() != 3 or wb.shape[0] != B or wb.shape[1] != N or wb.shape[2] < C_:
        raise ValueError(f'conv1x1_per_image: wb must be [{B}, {N}, >= {C_}], got {tuple(wb.shape)}')
    y = torch.empty((B, H, W, N), device=x.device, dtype=torch.float32)
    if residual is not None:
        _chk(residual, name='residual')
        assert residual.shape == y.shape
    gemm_conv(x, wb, y, B=1, H=H, W=W, Cin=C_, N=N, w_ld=wb.shape[2], scale=scale, shift=shift, residual=residual, act=act,
              groups=B, x_gs=H * W * C_, w_gs=N * wb.shape[2], y_gs=H * W * N, res_gs=H * W * N if residual is not None else 0)
    return y


def silu(x):
    _chk(x, name='x')
    y = torch.empty_like(x)
    check(lib().nbm_silu(_ptr(x), _ptr(y), x.numel(), _stream()), 'nbm_silu')
    return y


def layernorm(x2d, w, b, eps=1e-5):
    _chk(x2d, name='x')
    rows, E = x2d.shape
    y = torch.empty_like(x2d)
    check(lib().nbm_layernorm(_ptr(x2d), rows, E, _ptr(_chk(w)), _ptr(_chk(b)), float(eps), _ptr(y), _stream()), 'nbm_layernorm')
    return y


def mha_small(q, k, v, S, N, nhead, seq_stride, batch_stride, n_valid=None):
    """q, k, v: 2-D row views [S*N, >= E] (column slices of a fused projection are fine) -> out [S*N, E].  S <= MHA_SLONG; any
    head dim E // nhead <= 512.  csrc/mha.hip: up to MHA_SMAX tokens one lane per column for head dims up to 64 and the chunked
    wide kernels above; MHA_SMAX < S <= MHA_SLONG the long kernels (K and V through LDS in blocks of 128 keys, plain softmax
    over the whole row) -- the choice follows S, never *n_valid, and `mha_plan` reports it.  The same holds for `mha_small_drop`,
    the two backwards and `mha_segments` in MHA_ACROSS_ROIS."""
    E = q.shape[1]
    hd = E // nhead
    for t in (q, k, v):
        assert t.dim() == 2 and t.stride(1) == 1 and t.is_cuda and t.dtype == torch.float32
    out = torch.zeros((q.shape[0], E), device=q.device, dtype=torch.float32)
    check(lib().nbm_mha_small(_ptr(q), _ptr(k), _ptr(v), q.stride(0), k.stride(0), v.stride(0), _ptr(out), E, S, N, nhead,
                              hd, seq_stride, batch_stride, _ptr(n_valid), 1.0 / math.sqrt(hd), _stream()), 'nbm_mha_small')
    return out


MHA_SMAX = 128                  # csrc/mha.hip: longest sequence of the short kernels, and of a segment in MHA_ACROSS_IMAGES
MHA_SLONG = 1024                # csrc/mha.hip: longest sequence of nbm_mha_small* and of nbm_mha_segments_wide in MHA_ACROSS_ROIS
MHA_ACROSS_ROIS, MHA_ACROSS_IMAGES = 0, 1

MhaPlan = collections.namedtuple('MhaPlan', 'family lds_bytes lds_bytes_bwd rows row_blocks workspace_bytes')


def mha_plan(S, hd, N=1, nhead=1):
    """What `mha_small`, `mha_small_drop` and their backwards run on for sequences of S tokens and head dim hd (nbm_mha_plan,
    include/nbm_hip.h): family 'narrow' / 'wide' / 'long', the static LDS bytes of the forward and of the backward's pass 1, the
    query rows per workgroup, the workgroups per (batch entry, head) and the bytes of the backward's workspace for N entries of
    nhead heads.  Nothing is launched; works without a GPU.  A geometry the entry points refuse raises NbmHipError (NBM_EINVAL)."""
    p = _lib.MhaPlan()
    check(lib().nbm_mha_plan(int(S), int(hd), int(N), int(nhead), C.byref(p)), 'nbm_mha_plan')
    return MhaPlan(('narrow', 'wide', 'long')[p.family], p.lds_bytes, p.lds_bytes_bwd, p.rows, p.row_blocks, p.workspace_bytes)


def mha_segments(q, k, v, R, nhead, mode, segments, n_roi, max_count=None):
    """`mha_small` for a batch that is several model calls (evaluation only): q, k, v 2-D row views [B*R, >= E], token (b, r) =
    row b*R + r; `segments` the int32 [2, B] device table (`segment_table`), `n_roi` int32 [B] device counts (equal within a
    segment) -> out [B*R, E].  MHA_ACROSS_ROIS: attention over the RoIs r < n_roi[b] of each image, R <= MHA_SLONG (above
    MHA_SMAX slots through the long kernels, as `mha_small` with S = R); MHA_ACROSS_IMAGES: for every slot r < n_roi of a segment,
    over the segment's images, at most MHA_SMAX of them, any R.  Every row is written by the kernel -- zeros where there
    is no token -- so `out` is not pre-filled; valid rows equal `mha_small` on the segment alone bit for bit.
    `max_count`: largest segment of the table (default: the most a table of B images can hold, capped at MHA_SMAX -- the
    rows of a longer segment come out zero)."""
    E = q.shape[1]
    hd = E // nhead
    for t in (q, k, v):
        assert t.dim() == 2 and t.stride(1) == 1 and t.is_cuda and t.dtype == torch.float32
    if q.shape[0] % R:
        raise ValueError(f'{q.shape[0]} token rows are not images of {R} RoI slots')
    B = q.shape[0] // R
    _chk_segments(segments, B)
    _chk_counts(n_roi, B, 'n_roi')
    max_count = min(B, MHA_SMAX) if max_count is None else int(max_count)
    out = torch.empty((B * R, E), device=q.device, dtype=torch.float32)
    check(lib().nbm_mha_segments_wide(_ptr(q), _ptr(k), _ptr(v), q.stride(0), k.stride(0), v.stride(0), _ptr(out), E, B, R, nhead, hd,
                                      int(mode), _ptr(segments), _ptr(n_roi), max_count, 1.0 / math.sqrt(hd), _stream()),
          'nbm_mha_segments_wide')
    return out


# --------------------------------------------------------------------------- dropout (Transformer_RCNN head, training mode)
_PHILOX_M0, _PHILOX_M1, _PHILOX_W0, _PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter, key):
    """Philox4x32-10 in NumPy (host only): `counter` four and `key` two uint32 values or arrays of one shape -> uint32 [..., 4].
    csrc/nbm_philox.h is the same function on the device."""
    import numpy as np
    c = [np.asarray(v).astype(np.uint64) for v in counter]
    k = [np.asarray(v).astype(np.uint64) for v in key]
    lo32 = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(_PHILOX_M0) * c[0], np.uint64(_PHILOX_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & lo32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & lo32]
        k = [(k[0] + np.uint64(_PHILOX_W0)) & lo32, (k[1] + np.uint64(_PHILOX_W1)) & lo32]
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


def dropout_params(p):
    """-> (threshold, scale): an element is kept iff its mask word >= threshold = round(p * 2^32) (as a uint32), and a kept element
    is multiplied by scale = float32(1) / float32(1 - p).  0 <= p < 1."""
    import numpy as np
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f'--dropout must lie in [0, 1), got {p}')
    return min(int(round(p * 2.0 ** 32)), 0xffffffff), float(np.float32(1) / np.float32(1.0 - p))


def dropout_keep_reference(seed, call, site_id, n, p):
    """The dropout mask as a specification (host only, NumPy; no library call): bool [n], element i is kept iff output word i & 3 of
    Philox4x32-10 at counter (q & 0xffffffff, q >> 32, site_id, call), q = i >> 2, key = (low, high) half of the 64-bit `seed`, is
    >= round(p * 2^32).  The kernels (`dropout`, `mha_small_drop`) agree with it bit for bit."""
    import numpy as np
    threshold, _ = dropout_params(p)
    seed = int(seed) & 0xffffffffffffffff
    q = np.arange((int(n) + 3) // 4, dtype=np.uint64)
    words = philox4x32_10((q & np.uint64(0xffffffff), q >> np.uint64(32), int(site_id) & 0xffffffff, int(call) & 0xffffffff),
                          (seed & 0xffffffff, seed >> 32))
    return words.reshape(-1)[:int(n)] >= np.uint32(threshold)


def _drop_args(p, seed, call, site_id):
    threshold, scale = dropout_params(p)
    return (C.c_uint32(threshold), C.c_float(scale), C.c_uint64(int(seed) & 0xffffffffffffffff), C.c_uint32(int(call) & 0xffffffff),
            C.c_uint32(int(site_id) & 0xffffffff))


def dropout(x, p, seed, call, site_id, residual=None):
    """y = (residual or 0) + where(keep, x * scale, 0) with the mask of `dropout_keep_reference(seed, call, site_id, x.numel(), p)`
    over x's elements in memory order; each product and sum is one float32 operation.  With residual=None it is also its own
    backward pass (x = the incoming gradient)."""
    _chk(x, name='x')
    if residual is not None and _chk(residual, name='residual').shape != x.shape:
        raise ValueError(f'dropout: residual {tuple(residual.shape)} does not match x {tuple(x.shape)}')
    y = torch.empty_like(x)
    check(lib().nbm_dropout(_ptr(x), _ptr(residual), _ptr(y), x.numel(), *_drop_args(p, seed, call, site_id), _stream()),
          'nbm_dropout')
    return y


def mha_small_drop(q, k, v, S, N, nhead, seq_stride, batch_stride, n_valid, p, seed, call, site_id):
    """`mha_small` with dropout on the softmax probabilities: the mask is `dropout_keep_reference(seed, call, site_id,
    N * nhead * S * S, p)` read as a dense [N, nhead, S, S] tensor (query row, key column)."""
    E = q.shape[1]
    hd = E // nhead
    for t in (q, k, v):
        assert t.dim() == 2 and t.stride(1) == 1 and t.is_cuda and t.dtype == torch.float32
    out = torch.zeros((q.shape[0], E), device=q.device, dtype=torch.float32)
    check(lib().nbm_mha_small_drop(_ptr(q), _ptr(k), _ptr(v), q.stride(0), k.stride(0), v.stride(0), _ptr(out), E, S, N, nhead,
                                   hd, seq_stride, batch_stride, _ptr(n_valid), 1.0 / math.sqrt(hd),
                                   *_drop_args(p, seed, call, site_id), _stream()), 'nbm_mha_small_drop')
    return out


def mha_small_drop_bwd(q, k, v, go, S, N, nhead, seq_stride, batch_stride, n_valid, p, seed, call, site_id):
    """Gradients of `mha_small_drop` wrt q, k, v (the mask is evaluated again) -> contiguous [S*N, E] each.  S <= MHA_SLONG;
    workspace as `mha_small_bwd`."""
    E = q.shape[1]
    hd = E // nhead
    gq, gk, gv = (torch.zeros((q.shape[0], E), device=q.device, dtype=torch.float32) for _ in range(3))
    ws = torch.empty((N * nhead, 2, S, S), device=q.device, dtype=torch.float32)
    go = _chk(go)
    check(lib().nbm_mha_small_drop_bwd(_ptr(q), _ptr(k), _ptr(v), _ptr(go), q.stride(0), k.stride(0), v.stride(0), go.stride(0),
                                       _ptr(gq), _ptr(gk), _ptr(gv), E, E, E, _ptr(ws), S, N, nhead, hd, seq_stride, batch_stride,
                                       _ptr(n_valid), 1.0 / math.sqrt(hd), *_drop_args(p, seed, call, site_id), _stream()),
          'nbm_mha_small_drop_bwd')
    return gq, gk, gv


def layernorm_bwd_det(x2d, w, g2d, eps=1e-5):
    """`layernorm_bwd` with gw / gb summed in a fixed order (no atomics): the same inputs give the same bits -> (gx, gw, gb)."""
    rows, E = x2d.shape
    gx = torch.empty_like(x2d)
    gwb = torch.empty((2, E), device=x2d.device, dtype=torch.float32)
    ws = torch.empty((min((rows + 3) // 4, 256) * 8 * E,), device=x2d.device, dtype=torch.float32)
    check(lib().nbm_layernorm_bwd_det(_ptr(_chk(x2d)), _ptr(_chk(w)), _ptr(_chk(g2d)), rows, E, float(eps), _ptr(gx), _ptr(gwb[0]),
                                      _ptr(gwb[1]), _ptr(ws), ws.numel(), _stream()), 'nbm_layernorm_bwd_det')
    return gx, gwb[0], gwb[1]


def pair_softmax(x, n_anchor):
    """x [..., 2*n_anchor] -> softmax over each (bg, fg) pair."""
    _chk(x, name='x')
    ld = x.shape[-1]
    y = torch.empty_like(x)
    check(lib().nbm_pair_softmax(_ptr(x), x.numel() // ld, n_anchor, ld, _ptr(y), ld, _stream()), 'nbm_pair_softmax')
    return y


# --------------------------------------------------------------------------- proposal / RoI / detection
def rpn_decode(cls, reg, anchors, n_anchor, img_w, img_h, min_size):
    """cls [B,K,2A] softmaxed, reg [B,K,4A], anchors [K*A,4] -> boxes [B,KA,4], keys u32 [B,KA], keep_count [B]."""
    _chk(cls, name='cls'), _chk(reg, name='reg'), _chk(anchors, name='anchors')
    B = cls.shape[0]
    KA = anchors.shape[0]
    boxes = torch.empty((B, KA, 4), device=cls.device, dtype=torch.float32)
    keys = torch.empty((B, KA), device=cls.device, dtype=torch.int32)
    cnt = torch.empty((B,), device=cls.device, dtype=torch.int32)
    check(lib().nbm_rpn_decode(_ptr(cls), _ptr(reg), _ptr(anchors), B, KA, n_anchor, img_w, img_h, int(min_size),
                               _ptr(boxes), _ptr(keys), _ptr(cnt), _stream()), 'nbm_rpn_decode')
    return boxes, keys, cnt


def nan_images_fail(images, keep_count):
    """images [B, ...] (contiguous fp32), keep_count int32 [B] of `rpn_decode` (in place): an image that holds a NaN keeps no
    anchor, as in the reference, where the NaN reaches every RPN output and no comparison with it is true."""
    _chk(images, name='images')
    B = images.shape[0]
    _chk_counts(keep_count, B, 'keep_count')
    check(lib().nbm_nan_images(_ptr(images), B, images.numel() // B, _ptr(keep_count), _stream()), 'nbm_nan_images')
    return keep_count


def proposal_iou(rois, gt, n_gt):
    """rois [B,R,4], gt [B,G,4] (padded), n_gt int32 [B] -> (mx [B,R+G] best IoU of every proposal / ground-truth box with the
    image's ground-truth boxes, asg int32 [B,R+G] index of the first best box): reference layers.py:320-330."""
    _chk(rois, name='rois'), _chk(gt, name='gt')
    B, R, _ = rois.shape
    G = gt.shape[1]
    if n_gt.dtype != torch.int32 or n_gt.numel() != B or gt.shape[0] != B:
        raise ValueError('proposal_iou: n_gt must be int32 [B], gt [B,G,4]')
    mx = torch.empty((B, R + G), device=rois.device, dtype=torch.float32)
    asg = torch.empty((B, R + G), device=rois.device, dtype=torch.int32)
    check(lib().nbm_proposal_iou(_ptr(rois), _ptr(gt), _ptr(n_gt), B, R, G, _ptr(mx), _ptr(asg), _stream()), 'nbm_proposal_iou')
    return mx, asg


def anchor_targets(anchors, gt, n_gt, neg_t, pos_t):
    """anchors [n_in,4] (inside the image), gt [B,G,4] (padded), n_gt int32 [B] -> (lab int8 [B,n_in]: the label of every anchor
    before the random subsampling, amx int16 [B,n_in]: first best box, flag int32 [B]: recompute on the host): reference
    layers.py:150-179."""
    _chk(anchors, name='anchors'), _chk(gt, name='gt')
    B, G = gt.shape[:2]
    n_in = anchors.shape[0]
    if n_gt.dtype != torch.int32 or n_gt.numel() != B:
        raise ValueError('anchor_targets: n_gt must be int32 [B]')
    lab = torch.empty((B, n_in), device=gt.device, dtype=torch.int8)
    amx = torch.empty((B, n_in), device=gt.device, dtype=torch.int16)
    flag = torch.empty((B,), device=gt.device, dtype=torch.int32)
    check(lib().nbm_anchor_targets(_ptr(anchors), n_in, _ptr(gt), _ptr(n_gt), B, G, float(neg_t), float(pos_t), _ptr(lab), _ptr(amx),
                                   _ptr(flag), _stream()), 'nbm_anchor_targets')
    return lab, amx, flag


def segment_table(sizes, device='cuda'):
    """Segment sizes (contiguous, in batch order) -> the int32 [2, B] table of nbm_rpn_select / nbm_nms_batched: row 0 the
    first image of each image's segment, row 1 the segment's image count (on `device`; 'cpu' for a pinned staging copy)."""
    first, count = [], []
    b = 0
    for n in sizes:
        n = int(n)
        if n <= 0:
            raise ValueError('segments hold at least one image')
        first += [b] * n
        count += [n] * n
        b += n
    t = torch.tensor([first, count], dtype=torch.int32)
    return t if device == 'cpu' else t.to(device)


_BATCH_SEGMENTS = {}


def batch_segments(B, size=None, device='cuda'):
    """Read-only device table (`segment_table`) of B images in contiguous segments of `size` images each: None = the whole
    batch is one segment (the reference's coupling for one model call on it), 1 = every image a model call of its own.
    Cached per (device, B, size) and never evicted, because captured graphs hold these addresses.  A missing table is filled
    by a blocking copy, so it is on the device before any stream reads it; that copy cannot happen during a graph capture
    (the capture's warm-up steps fill the cache)."""
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device(dev.type, torch.cuda.current_device())
    size = B if size is None else int(size)
    key = (dev, B, size)
    t = _BATCH_SEGMENTS.get(key)
    if t is None:
        if size <= 0 or B % size:
            raise ValueError(f'a batch of {B} does not split into segments of {size}')
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f'the segment table for a batch of {B} in segments of {size} would be created during a graph capture '
                               '(the warm-up steps of the capture must run the same batch and coupling)')
        t = _BATCH_SEGMENTS[key] = segment_table([size] * (B // size), dev)
    return t


def _chk_segments(segments, B):
    _chk(segments, torch.int32, 'segments')
    if tuple(segments.shape) != (2, B):
        raise ValueError(f'segment table of shape {tuple(segments.shape)} for a batch of {B}: expected (2, {B})')
    return segments


def _chk_counts(n, B, name):
    _chk(n, torch.int32, name)
    if n.numel() != B:
        raise ValueError(f'{name}: one count per image, got {n.numel()} for a batch of {B}')
    return n


def roi_counts(n, B, name='n_roi'):
    """RoI counts of the RoI stages -> int32 [B], one count per image.  A single count is the same count for every image
    (RoI tensors of R real rows per image); it is broadcast here, so the kernels always read n[b]."""
    _chk(n, torch.int32, name)
    if n.numel() == 1 and B > 1:
        return n.expand(B).contiguous()
    return _chk_counts(n, B, name)


PROPOSAL_SMALL_CAP = 4096     # nbm_rpn_select / nbm_nms_batched: sort in LDS, one wave of removed words
PROPOSAL_BIG_CAP = 65536      # nbm_rpn_select_big / nbm_nms_big


def _pow2_cap(n):
    c = 64
    while c < n:
        c <<= 1
    return c


def proposal_plan(pre, KA):
    """Host-only: the pre-NMS budget `pre` (--pre_nms_topN / --pre_nms_topN_eval) on a map of KA anchors -> (top_n, cap,
    route).  Up to 4096 the budget is taken as it is, on the kernels that sort in LDS ('small').  A larger one is first cut to
    KA, which changes no result (an image keeps at most its KA anchors), and goes to the global-memory kernels ('big') when
    its capacity still exceeds 4096."""
    pre, KA = int(pre), int(KA)
    if pre <= PROPOSAL_SMALL_CAP:
        return pre, _pow2_cap(pre), 'small'
    top_n = min(pre, KA)
    cap = _pow2_cap(top_n)
    if cap <= PROPOSAL_SMALL_CAP:
        return top_n, cap, 'small'
    if cap > PROPOSAL_BIG_CAP:
        raise ValueError(f'--pre_nms_topN / --pre_nms_topN_eval = {pre} on {KA} anchors: the proposal kernels take up to '
                         f'{PROPOSAL_BIG_CAP} boxes per image')
    return top_n, cap, 'big'


def _workspace(query, B, cap, device, name):
    nbytes = C.c_int64()
    check(query(B, cap, C.byref(nbytes)), name)
    return torch.empty((nbytes.value,), device=device, dtype=torch.uint8), nbytes.value


def rpn_select(boxes, keys, keep_count, top_n, fail_below, cap, segments=None, force_big=False):
    """-> sel_boxes [B,cap,4], sel_scores [B,cap], n_sel int32 [B].  The counts are coupled within each segment of `segments`
    (int32 [2, B] on the device, `segment_table`; None: `batch_segments(B)`, the whole batch).  cap above 4096 (up to 65536)
    runs nbm_rpn_select_big; `force_big` sends a smaller cap there too (tests and benchmarks: the results are the same)."""
    B, KA = keys.shape
    _chk_counts(keep_count, B, 'keep_count')
    segments = batch_segments(B, device=boxes.device) if segments is None else _chk_segments(segments, B)
    sel_boxes = torch.empty((B, cap, 4), device=boxes.device, dtype=torch.float32)
    sel_scores = torch.empty((B, cap), device=boxes.device, dtype=torch.float32)
    n_sel = torch.empty((B,), device=boxes.device, dtype=torch.int32)
    if cap > PROPOSAL_SMALL_CAP or force_big:
        ws, ws_bytes = _workspace(lib().nbm_rpn_select_big_workspace, B, cap, boxes.device, 'nbm_rpn_select_big_workspace')
        check(lib().nbm_rpn_select_big(_ptr(boxes), _ptr(keys), _ptr(keep_count), B, KA, top_n, fail_below, cap, _ptr(ws),
                                       ws_bytes, _ptr(sel_boxes), _ptr(sel_scores), _ptr(n_sel), _ptr(segments), _stream()),
              'nbm_rpn_select_big')
        return sel_boxes, sel_scores, n_sel
    check(lib().nbm_rpn_select(_ptr(boxes), _ptr(keys), _ptr(keep_count), B, KA, top_n, fail_below, cap,
                               _ptr(sel_boxes), _ptr(sel_scores), _ptr(n_sel), _ptr(segments), _stream()), 'nbm_rpn_select')
    return sel_boxes, sel_scores, n_sel


def nms_batched(boxes, scores, n_in, thresh, post_n, segments=None, force_big=False):
    """boxes [B,cap,4] in walk order, n_in int32 [B] -> rois [B,post_n,4], scores [B,post_n], n_out int32 [B].  The post-NMS
    truncation is coupled within each segment (see rpn_select).  cap above 4096 (up to 65536) runs nbm_nms_big, which stores
    no IoU mask; `force_big` as in rpn_select."""
    _chk(boxes, name='boxes'), _chk(scores, name='scores')
    B, cap = scores.shape
    _chk_counts(n_in, B, 'n_in')
    segments = batch_segments(B, device=boxes.device) if segments is None else _chk_segments(segments, B)
    rois = torch.empty((B, post_n, 4), device=boxes.device, dtype=torch.float32)
    rs = torch.empty((B, post_n), device=boxes.device, dtype=torch.float32)
    n_out = torch.empty((B,), device=boxes.device, dtype=torch.int32)
    if cap > PROPOSAL_SMALL_CAP or force_big:
        ws, ws_bytes = _workspace(lib().nbm_nms_big_workspace, B, cap, boxes.device, 'nbm_nms_big_workspace')
        check(lib().nbm_nms_big(_ptr(boxes), _ptr(scores), _ptr(n_in), B, cap, float(thresh), post_n, _ptr(ws), ws_bytes,
                                _ptr(rois), _ptr(rs), _ptr(n_out), _ptr(segments), _stream()), 'nbm_nms_big')
        return rois, rs, n_out
    words = cap // 64
    mask_ws = torch.empty((B * cap * words,), device=boxes.device, dtype=torch.int64)
    keep_ws = torch.empty((B * (cap + 1),), device=boxes.device, dtype=torch.int32)
    check(lib().nbm_nms_batched(_ptr(boxes), _ptr(scores), _ptr(n_in), B, cap, float(thresh), post_n, _ptr(mask_ws),
                                _ptr(keep_ws), _ptr(rois), _ptr(rs), _ptr(n_out), _ptr(segments), _stream()), 'nbm_nms_batched')
    return rois, rs, n_out


# The pool size the demand-driven FPN maps and the persistent gradient maps serve: the tile lists (nbm_roi_tiles) and the
# footprint re-zeroing (nbm_zero_roi_windows) are built on its windows.
ONDEMAND_POOL_HW = (2, 2)


def roi_pool_plan(ph, pw, fmap_hw):
    """What a `--roi_pool_h` x `--roi_pool_w` pool on maps of the sizes `fmap_hw` [(h, w), ...] may read and write
    -> 'ondemand' (ONDEMAND_POOL_HW: demand-driven maps, persistent gradient maps) or 'dense' (dense maps only); the kernels
    are the same.  Host-only; refuses the two pool sizes the reference itself cannot run."""
    ph, pw = int(ph), int(pw)
    if ph < 2 or pw < 2:
        raise ValueError(f'--roi_pool_h {ph} / --roi_pool_w {pw}: a pool below 2 x 2 is no configuration of the reference -- its '
                         'positional-encoding slice pe_frequency[s*y1 : s*y2] is empty for a one-row window (layers.py:484), '
                         'and the average of an empty slice is NaN')
    mh, mw = min(int(h) for h, _ in fmap_hw), min(int(w) for _, w in fmap_hw)
    if ph > mh or pw > mw:
        raise ValueError(f'--roi_pool_h {ph} / --roi_pool_w {pw} exceeds the smallest pyramid map ({mh} x {mw}): the '
                         "reference's growth loop (layers.py:459-465) does not terminate when a window cannot reach the pool size")
    return 'ondemand' if (ph, pw) == ONDEMAND_POOL_HW else 'dense'


def roi_pool(fmaps, rois, n_roi, pe_f, pe_t, img_h, img_w, pool_hw=ONDEMAND_POOL_HW):
    """fmaps: list of NHWC [B,h,w,C]; rois [B,cap,4]; n_roi device int32 [B] (or [1], `roi_counts`) -> pool,
    pe [B*cap,ph,pw,C], level [B,cap].  Rows of slots past n_roi, and of RoIs whose window has no pixel in the map, stay zero."""
    B, cap = rois.shape[:2]
    ph, pw = int(pool_hw[0]), int(pool_hw[1])
    roi_pool_plan(ph, pw, [tuple(f.shape[1:3]) for f in fmaps])
    n_roi = roi_counts(n_roi, B)
    C_ = fmaps[0].shape[-1]
    d = RoiHwDesc()
    for i, f in enumerate(fmaps):
        _chk(f, name=f'fmap{i}')
        d.fmap[i] = f.data_ptr()
        d.fh[i], d.fw[i] = f.shape[1], f.shape[2]
    d.n_levels, d.C = len(fmaps), C_
    d.rois, d.n_roi, d.B, d.roi_cap = _chk(rois).data_ptr(), n_roi.data_ptr(), B, cap
    d.pe_f, d.pe_t, d.img_h, d.img_w = _chk(pe_f).data_ptr(), _chk(pe_t).data_ptr(), img_h, img_w
    pool = torch.zeros((B * cap, ph, pw, C_), device=rois.device, dtype=torch.float32)
    pe = torch.zeros((B * cap, ph, pw, C_), device=rois.device, dtype=torch.float32)
    level = torch.zeros((B, cap), device=rois.device, dtype=torch.int32)
    d.pool, d.pe, d.level = pool.data_ptr(), pe.data_ptr(), level.data_ptr()
    d.pool_h, d.pool_w = ph, pw
    check(lib().nbm_roi_pool_hw(C.byref(d), _stream()), 'nbm_roi_pool_hw')
    return pool, pe, level


def rcnn_post(rois, n_roi, bbox_reg, bbox_cls, img_w, img_h, nms_thresh, min_score, proposal_number):
    """n_roi int32 [B] (or [1], `roi_counts`) -> det [B,cap,6] rows {class,x1,y1,x2,y2,score} sorted by
    (class, score desc), n_det [B]."""
    B, cap = rois.shape[:2]
    n_roi = roi_counts(n_roi, B)
    n_cls1 = bbox_cls.shape[-1]
    det = torch.zeros((B, cap, 6), device=rois.device, dtype=torch.float32)
    n_det = torch.zeros((B,), device=rois.device, dtype=torch.int32)
    check(lib().nbm_rcnn_post(_ptr(_chk(rois)), _ptr(n_roi), B, cap, _ptr(_chk(bbox_reg)), _ptr(_chk(bbox_cls)),
                              n_cls1, img_w, img_h, float(nms_thresh), float(min_score), int(proposal_number),
                              _ptr(det), _ptr(n_det), _stream()), 'nbm_rcnn_post')
    return det, n_det


# --------------------------------------------------------------------------- per-file merge (run_detection.merge_images)
MERGE_MAX_N = 131072          # NBM_MERGE_MAX_N


def merge_collect(det, n_det, w_pix, hop, spectrogram_length, num_classes):
    """det [n_img,cap,6] (rcnn_post rows of the file's windows in order), n_det int32 [n_img] -> boxes [n_img*cap,4] (shifted),
    scores [n_img*cap], species int32 [n_img*cap], n int32 [1]: the first n rows in the reference's collected order."""
    _chk(det, name='det'), _chk(n_det, torch.int32, 'n_det')
    n_img, cap = det.shape[:2]
    dev = det.device
    cells = torch.empty((n_img * num_classes,), device=dev, dtype=torch.int32)
    boxes = torch.empty((n_img * cap, 4), device=dev, dtype=torch.float32)
    scores = torch.empty((n_img * cap,), device=dev, dtype=torch.float32)
    species = torch.empty((n_img * cap,), device=dev, dtype=torch.int32)
    n = torch.empty((1,), device=dev, dtype=torch.int32)
    check(lib().nbm_merge_collect(_ptr(det), _ptr(n_det), n_img, cap, int(num_classes), int(w_pix), int(hop),
                                  int(spectrogram_length), _ptr(cells), _ptr(boxes), _ptr(scores), _ptr(species), _ptr(n),
                                  _stream()), 'nbm_merge_collect')
    return boxes, scores, species, n


def merge_nms_workspace_bytes(cap):
    if not 0 <= cap <= MERGE_MAX_N:
        raise ValueError(f'merge NMS: {cap} boxes is above the limit of {MERGE_MAX_N}')
    nbytes = C.c_int64()
    check(lib().nbm_merge_nms_workspace(int(cap), C.byref(nbytes)), 'nbm_merge_nms_workspace')
    return nbytes.value


def merge_nms(boxes, n, thresh, cap=None):
    """Greedy NMS in the given order over the first n (device int32 [1]) of boxes [>=cap,4]; cap (default len(boxes)) <=
    MERGE_MAX_N -> keep int32 [cap] (first n_keep valid), n_keep int32 [1]."""
    _chk(boxes, name='boxes'), _chk(n, torch.int32, 'n')
    cap = boxes.shape[0] if cap is None else int(cap)
    if cap > boxes.shape[0]:
        raise ValueError('merge NMS: cap exceeds the box buffer')
    ws_bytes = merge_nms_workspace_bytes(cap)
    ws = torch.empty((ws_bytes,), device=boxes.device, dtype=torch.uint8)
    keep = torch.empty((max(cap, 1),), device=boxes.device, dtype=torch.int32)
    n_keep = torch.empty((1,), device=boxes.device, dtype=torch.int32)
    check(lib().nbm_merge_nms(_ptr(boxes), _ptr(n), cap, float(thresh), _ptr(ws), ws_bytes, _ptr(keep), _ptr(n_keep),
                              _stream()), 'nbm_merge_nms')
    return keep, n_keep


def merge_gather(boxes, scores, species, keep, n_keep, cap):
    """-> one float32 tensor [1 + 6*cap]: word 0 holds the row count (int32 bits), then rows {species,x1,y1,x2,y2,score} in the
    kept order -- a single device-to-host copy brings back the whole merge."""
    _chk(boxes, name='boxes'), _chk(scores, name='scores'), _chk(species, torch.int32, 'species')
    _chk(keep, torch.int32, 'keep'), _chk(n_keep, torch.int32, 'n_keep')
    out = torch.empty((1 + 6 * cap,), device=boxes.device, dtype=torch.float32)
    check(lib().nbm_merge_gather(_ptr(boxes), _ptr(scores), _ptr(species), _ptr(keep), _ptr(n_keep), int(cap), _ptr(out[1:]),
                                 _ptr(out[:1].view(torch.int32)), _stream()), 'nbm_merge_gather')
    return out


def unpack_merged(out):
    """Host side of merge_gather's buffer -> float32 rows [n,6]."""
    out = out.cpu() if out.is_cuda else out
    n = int(out[:1].view(torch.int32)[0])
    return out[1:1 + 6 * n].view(n, 6)


# =========================================================================== training path
from ._lib import BwdDesc  # noqa: E402


class _timed:
    """HIP-event bracket around one launch, recorded in PROFILE_BWD when that is a list (scripts/trainlayers.py)."""

    def __init__(self, tag):
        self.tag = tag

    def __enter__(self):
        if PROFILE_BWD is not None:
            self.ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            self.ev[0].record()

    def __exit__(self, *exc):
        if PROFILE_BWD is not None:
            self.ev[1].record()
            PROFILE_BWD.append((self.tag, *self.ev))


PROFILE_BWD = None


def _bwd_desc(g, *, B, H, W, Cin, N, kh, kw, stride, pad, g_ld, groups=1, alpha=1.0):
    d = BwdDesc()
    d.g = g.data_ptr()
    d.groups = groups
    d.B, d.H, d.W, d.Cin, d.N = B, H, W, Cin, N
    d.kh, d.kw, d.stride, d.pad = kh, kw, stride, pad
    d.Ho = (H + 2 * pad - kh) // stride + 1
    d.Wo = (W + 2 * pad - kw) // stride + 1
    d.g_ld = g_ld
    d.alpha = float(alpha)
    return d


GemmPlan = collections.namedtuple('GemmPlan', 'rc kernel grid block m_tiles n_tiles vec_epi fast slices phased ph_tiles splits k_chunk '
                                              'plain b_generic narrow_m halves')


def gemm_plan(kind, desc):
    """What nbm_gemm_conv (kind 0, a GemmDesc), nbm_conv_dgrad (1) or nbm_conv_wgrad (2, a BwdDesc) would do with `desc` under the current
    environment switches: the kernel instantiation by name, its grid and the tiling values (nbm_gemm_plan, include/nbm_hip.h).  Nothing is
    launched; works without a GPU.  rc != 0: the entry point's NBM_E* code, the other fields are unset."""
    p = _lib.GemmPlan()
    lib().nbm_gemm_plan(int(kind), C.byref(desc), C.byref(p))
    return GemmPlan(p.rc, (p.name or b'').decode(), tuple(p.grid), p.block, p.m_tiles, p.n_tiles, p.vec_epi, p.fast, p.slices, p.phased,
                    tuple(p.ph_tiles), p.splits, p.k_chunk, p.plain, p.b_generic, p.narrow_m, p.halves)


def split_nn():
    """Deep-K 1x1 data gradients through nbm_gemm_conv's split-bf16 kernel (opt-in with NBM_SPLIT_BF16=1; NBM_SPLIT_NN=0 keeps them on
    the fp32 data-gradient kernel)."""
    return os.environ.get('NBM_SPLIT_BF16') == '1' and os.environ.get('NBM_SPLIT_NN', '1') != '0'


def conv_dgrad(g, w, out, *, B, H, W, Cin, N, kh=1, kw=1, stride=1, pad=0, g_ld=None, w_ld=None, out_ld=None,
               a_scale=None, residual=None, mask=None, alpha=1.0, groups=1, g_gs=0, w_gs=0, out_gs=0, res_gs=0, residual2=None,
               mask_bits=None):
    """Raw nbm_conv_dgrad: out[B*H*W][Cin] = gather(g)[..][N] x W (see include/nbm_hip.h).  `residual2` [B, ceil(H/2), ceil(W/2),
    Cin]: added at the pixels with even row and column (a stride-2 shortcut's data gradient at its own resolution)."""
    if (kh == 1 and kw == 1 and stride == 1 and pad == 0 and residual2 is None and N > 256 and N % 32 == 0 and Cin > 64 and Cin % 4 == 0 and
            (groups == 1 or (mask is None and a_scale is None)) and split_nn()):
        # opt-in (NBM_SPLIT_BF16=1): a deep-K 1x1 data gradient IS the forward GEMM of the incoming gradient with the
        # transposed weights (FrozenBN scale folded in), so it takes nbm_gemm_conv's split-bf16 kernel; shortcut gradient and ReLU mask
        # ride in that kernel's epilogue (`residual`, `mask`).  The transposed copy is rebuilt per call ([N][Cin] -> [Cin][N], a few MB).
        # The rule names the LAYER (K = N, the channel counts, the operands), never the number of rows or groups: the P V product of the
        # attention (one group per image) takes the same kernel whatever the batch.
        wl = kh * kw * Cin if w_ld is None else w_ld
        wv = w.as_strided((groups, N, Cin), (w_gs, wl, 1))         # (`w` may be a row / column slice of a wider matrix: only its pitches count)
        wt = (wv * a_scale[None, :N, None] if a_scale is not None else wv).transpose(1, 2).contiguous()
        with _timed(('dgrad', B, H, W, Cin, N, kh, stride, groups)):
            gemm_conv(g, wt, out, B=B, H=H, W=W, Cin=N, N=Cin, x_ld=N if g_ld is None else g_ld, w_ld=N,
                      y_ld=Cin if out_ld is None else out_ld, residual=residual, res_ld=Cin if residual is not None else None, alpha=alpha,
                      mask=mask, mask_ld=Cin if mask is not None else None, groups=groups, x_gs=g_gs, w_gs=Cin * N, y_gs=out_gs, res_gs=res_gs)
        return out
    d = _bwd_desc(g, B=B, H=H, W=W, Cin=Cin, N=N, kh=kh, kw=kw, stride=stride, pad=pad,
                  g_ld=N if g_ld is None else g_ld, groups=groups, alpha=alpha)
    d.w, d.out = w.data_ptr(), out.data_ptr()
    d.w_ld = kh * kw * Cin if w_ld is None else w_ld
    d.out_ld = Cin if out_ld is None else out_ld
    d.a_scale = a_scale.data_ptr() if a_scale is not None else None
    d.residual = residual.data_ptr() if residual is not None else None
    d.res_ld = Cin if residual is not None else 0
    d.mask = mask.data_ptr() if mask is not None else None
    d.mask_ld = Cin if mask is not None else 0
    if mask_bits is not None and groups == 1 and Cin % 32 == 0:
        # the same mask as one bit per element (written by the producer's epilogue, `gemm_conv(bits_out=)`): 1/32 of the bytes
        assert mask_bits.dtype == torch.int32 and mask_bits.numel() * 32 >= B * H * W * Cin
        d.mask_bits, d.mask, d.mask_ld = mask_bits.data_ptr(), None, 0
    if residual2 is not None:
        if groups != 1 or tuple(residual2.shape) != (B, (H + 1) // 2, (W + 1) // 2, Cin) or kh != 1 or stride != 1:
            raise ValueError('conv_dgrad: residual2 must be [B, ceil(H/2), ceil(W/2), Cin] of a 1x1 / stride-1 data gradient')
        d.residual2, d.res2_ld = _chk(residual2, name='residual2').data_ptr(), Cin
    d.g_gs, d.w_gs, d.out_gs, d.res_gs = g_gs, w_gs, out_gs, res_gs
    if FLOPS is not None:          # executed: the stride-2 kernels visit only the taps that reach each parity class
        FLOPS[0] += 2.0 * B * d.Ho * d.Wo * N * kh * kw * Cin * groups
    with _timed(('dgrad', B, H, W, Cin, N, kh, stride, groups)):
        check(lib().nbm_conv_dgrad(C.byref(d), _stream()), 'nbm_conv_dgrad')
    return out


def conv_wgrad(g, x, out, *, B, H, W, Cin, N, kh=1, kw=1, stride=1, pad=0, g_ld=None, x_ld=None, out_ld=None,
               row_scale=None, alpha=1.0, groups=1, g_gs=0, x_gs=0, out_gs=0, bias_grad=None):
    """Raw nbm_conv_wgrad: out[N][kh*kw*Cin] += g^T x im2col(x); `out` must be zeroed (or hold a partial sum)."""
    d = _bwd_desc(g, B=B, H=H, W=W, Cin=Cin, N=N, kh=kh, kw=kw, stride=stride, pad=pad,
                  g_ld=N if g_ld is None else g_ld, groups=groups, alpha=alpha)
    d.x, d.out = x.data_ptr(), out.data_ptr()
    d.x_ld = Cin if x_ld is None else x_ld
    d.out_ld = kh * kw * Cin if out_ld is None else out_ld
    d.row_scale = row_scale.data_ptr() if row_scale is not None else None
    d.g_gs, d.x_gs, d.out_gs = g_gs, x_gs, out_gs
    deferred_bias = None
    if bias_grad is not None and groups == 1:
        # the split-bf16 weight-gradient kernel (opt-in) does not sum the columns of G: where the library takes it for this launch without
        # a bias gradient, the bias gradient comes from nbm_colsum (one group's sums) instead of riding along
        if gemm_plan(2, d).kernel.startswith('igemm_split_tn_kernel'):
            deferred_bias, bias_grad = bias_grad, None
    d.bias_grad = bias_grad.data_ptr() if bias_grad is not None else None       # [N] zeros: += column sums of g
    if deterministic():
        bad = _det_refusals()              # (an option switched on after the mode was: refused here, not run on its atomics)
        if bad:
            raise ValueError('--deterministic does not cover ' + '; '.join(f'{o} ({why})' for o, why in bad))
        # the twin: every pixel split stores its slice of the workspace, an ordered reduction adds them (nbm_bwd_desc.workspace).
        # (A slice beyond the workspace ceiling is refused by the query: NBM_EUNSUPPORTED.)
        nbytes, stride = wgrad_workspace(d)
        if nbytes:
            ws = _det_workspace(nbytes)
            d.workspace, d.ws_split_stride, d.workspace_bytes = ws.data_ptr(), stride, nbytes
    if FLOPS is not None:
        FLOPS[0] += 2.0 * B * d.Ho * d.Wo * N * kh * kw * Cin * groups
    with _timed(('wgrad', B, H, W, Cin, N, kh, stride, groups)):
        check(lib().nbm_conv_wgrad(C.byref(d), _stream()), 'nbm_conv_wgrad')
    if deferred_bias is not None:
        gl = N if g_ld is None else g_ld
        deferred_bias += colsum(g.reshape(-1)[:B * H * W * gl].view(B * H * W, gl), N)
    return out


def wgrad_workspace(desc):
    """(bytes, floats between the slices of consecutive splits) of the deterministic twin of nbm_conv_wgrad for a BwdDesc
    (nbm_conv_wgrad_workspace: host only, works without a GPU); bytes = 0: one split and no bias gradient, nothing to order."""
    nbytes, stride = C.c_int64(0), C.c_int64(0)
    check(lib().nbm_conv_wgrad_workspace(C.byref(desc), C.byref(nbytes), C.byref(stride)), 'nbm_conv_wgrad_workspace')
    return nbytes.value, stride.value


def _gconv_bwd_desc(B, H, W, groups, Cg, stride, kh=3, kw=3, pad=1, splits=0):
    d = GconvBwdDesc()
    d.B, d.H, d.W, d.groups, d.Cg = int(B), int(H), int(W), int(groups), int(Cg)
    d.kh, d.kw, d.stride, d.pad = int(kh), int(kw), int(stride), int(pad)
    d.Ho, d.Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    d.splits = int(splits)
    return d


def _gconv_bwd_operands(name, g, y, groups, C_):
    """Common checks of the two grouped gradients: g (and y) [B,Ho,Wo,ld >= C], contiguous fp32 on the device."""
    _chk(g, name='g')
    if g.dim() != 4 or groups <= 0 or C_ % groups or g.shape[3] < C_:
        raise ValueError(f'{name}: g must be [B,Ho,Wo,>={C_}] for {groups} groups')
    if y is not None and (_chk(y, name='y').dim() != 4 or tuple(y.shape[:3]) != tuple(g.shape[:3]) or y.shape[3] < C_):
        raise ValueError(f'{name}: y must be [{g.shape[0]},{g.shape[1]},{g.shape[2]},>={C_}], the forward output')


def gconv_wgrad_plan(B, Ho, Wo, groups, Cg, stride):
    """Host-only (no GPU needed): what `gconv3x3_wgrad(splits=None)` does for a launch whose gradient map is [B,Ho,Wo,groups * Cg] ->
    (splits, workspace_bytes).  The library picks the split count (nbm_gconv3x3_wgrad_workspace with splits = 0: two workgroups per
    CU, at most one per pixel tile, the workspace within the bytes of the two operands); the workspace is linear in it.  The choice
    depends on the gradient map alone, so the input map is taken as the smallest that gives (Ho, Wo) at this stride."""
    H, W = (int(Ho) - 1) * int(stride) + 1, (int(Wo) - 1) * int(stride) + 1
    total, one = C.c_longlong(), C.c_longlong()
    check(lib().nbm_gconv3x3_wgrad_workspace(C.byref(_gconv_bwd_desc(B, H, W, groups, Cg, stride)), C.byref(total)),
          'nbm_gconv3x3_wgrad_workspace')
    check(lib().nbm_gconv3x3_wgrad_workspace(C.byref(_gconv_bwd_desc(B, H, W, groups, Cg, stride, splits=1)), C.byref(one)),
          'nbm_gconv3x3_wgrad_workspace')
    return int(total.value // one.value), int(total.value)


def gconv3x3_dgrad(g, w_prepared, groups, H, W, stride=1, y=None, out=None, kh=3, kw=3, pad=1):
    """Data gradient of `gconv3x3` (+ scale + ReLU): g = dL/dy [B,Ho,Wo,g_ld >= C], `w_prepared` = `_prep.gconv_dgrad(weight, groups,
    scale)`, H x W the forward input map -> gx [B,H,W,C], or into `out` [B,H,W,out_ld >= C] (channels beyond C are left alone).  `y`
    (the forward output): g counts only where y > 0, applied inside the kernel.  What the kernel does not implement raises (kh, kw and
    pad are only there to be refused): there is no slow path."""
    _chk(w_prepared, name='w_prepared')
    if w_prepared.dim() != 5 or tuple(w_prepared.shape[1::2]) != (9, 64) or w_prepared.shape[4] != 4 or groups <= 0 \
            or (16 * w_prepared.shape[0]) % groups:
        raise ValueError('gconv3x3_dgrad: w_prepared must be the output of _prep.gconv_dgrad for these groups')
    n_ch = 16 * w_prepared.shape[0]
    Cg = n_ch // groups
    if max(Cg, 16) != 16 * w_prepared.shape[2]:
        raise ValueError(f'gconv3x3_dgrad: w_prepared {tuple(w_prepared.shape)} does not belong to {groups} groups of {Cg} channels')
    _gconv_bwd_operands('gconv3x3_dgrad', g, y, groups, n_ch)
    B = g.shape[0]
    d = _gconv_bwd_desc(B, H, W, groups, Cg, stride, kh, kw, pad)
    if tuple(g.shape[1:3]) != (d.Ho, d.Wo):
        raise ValueError(f'gconv3x3_dgrad: g is {tuple(g.shape)}, a {H} x {W} input at stride {stride} gives [{B},{d.Ho},{d.Wo},.]')
    gx = out if out is not None else torch.empty((B, H, W, n_ch), device=g.device, dtype=torch.float32)
    _chk(gx, name='out')
    if gx.dim() != 4 or tuple(gx.shape[:3]) != (B, H, W) or gx.shape[3] < n_ch:
        raise ValueError(f'gconv3x3_dgrad: out must be [{B},{H},{W},>={n_ch}]')
    d.g, d.w, d.out = g.data_ptr(), w_prepared.data_ptr(), gx.data_ptr()
    d.g_ld, d.out_ld = g.shape[3], gx.shape[3]
    if y is not None:
        d.y, d.y_ld = y.data_ptr(), y.shape[3]
    if FLOPS is not None:
        FLOPS[0] += 2.0 * 9 * Cg * n_ch * B * d.Ho * d.Wo         # algorithmic, as gconv3x3
    with _timed(('gconv_dgrad', B, H, W, Cg, n_ch, kh, stride, groups)):
        check(lib().nbm_gconv3x3_dgrad(C.byref(d), _stream()), 'nbm_gconv3x3_dgrad')
    return gx


_GCONV_WS = {}


def _gconv_workspace(device, nbytes):
    """One persistent workspace per device and lane (every launch overwrites what it reads; launches of a stream are ordered)."""
    key = (device, LANE)
    buf = _GCONV_WS.get(key)
    if buf is None or buf.numel() < nbytes:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('the grouped weight-gradient workspace would have to grow during a graph capture')
        _GCONV_WS[key] = buf = None
        buf = _GCONV_WS[key] = torch.empty((nbytes,), device=device, dtype=torch.uint8)
    return buf


def gconv3x3_wgrad(g, x, groups, stride=1, scale=None, y=None, out=None, accumulate=False, splits=None, workspace=None,
                   channels=None, kh=3, kw=3, pad=1):
    """Weight gradient of `gconv3x3` (+ scale + ReLU): g = dL/dy [B,Ho,Wo,g_ld >= C], x [B,H,W,x_ld >= C] the forward input ->
    dW [C, Cg, 3, 3] (the parameter's layout), or into `out` (C * Cg * 9 contiguous floats; `accumulate`: added to what is there).
    `scale` [C] multiplies row n; `y` (the forward output): g counts only where y > 0.  `splits`: workgroups the pixel sum is split over
    per 64 channels; None takes the library's choice (`gconv_wgrad_plan`), an explicit value (1 .. 4096) is for tests and benchmarks --
    the result is bitwise reproducible for a given count.  `workspace`: a uint8 tensor for the partial sums (tests); default: a
    persistent one.  `channels`: C; required where the operands are pitched and neither `out` [C,Cg,3,3] nor `scale` tells it.  What the kernels do
    not implement raises: there is no slow path."""
    _chk(x, name='x')
    if x.dim() != 4 or groups <= 0:
        raise ValueError('gconv3x3_wgrad: x must be [B,H,W,>=C]')
    B, H, W, x_ld = x.shape
    _chk(g, name='g')
    # C: `channels`, else what `out` [C,Cg,3,3] or `scale` [C] say; unpitched operands of equal width tell it themselves
    if channels is not None:
        n_ch = int(channels)
    elif out is not None and out.dim() == 4:
        n_ch = out.shape[0]
    elif scale is not None:
        n_ch = scale.numel()
    elif g.shape[-1] == x_ld:
        n_ch = x_ld
    else:
        raise ValueError(f'gconv3x3_wgrad: g and x are {g.shape[-1]} and {x_ld} floats wide: pass `channels` (or `out` [C,Cg,3,3] / `scale`)')
    _gconv_bwd_operands('gconv3x3_wgrad', g, y, groups, n_ch)
    Cg = n_ch // groups
    if x_ld < n_ch or g.shape[0] != B:
        raise ValueError(f'gconv3x3_wgrad: x {tuple(x.shape)} and g {tuple(g.shape)} do not belong to {n_ch} channels of one batch')
    d = _gconv_bwd_desc(B, H, W, groups, Cg, stride, kh, kw, pad, splits=0 if splits is None else splits)
    if splits is not None and not 1 <= int(splits) <= 4096:
        raise ValueError(f'gconv3x3_wgrad: splits = {splits} (1 .. 4096, or None)')
    if tuple(g.shape[1:3]) != (d.Ho, d.Wo):
        raise ValueError(f'gconv3x3_wgrad: g is {tuple(g.shape)}, x {tuple(x.shape)} at stride {stride} gives [{B},{d.Ho},{d.Wo},.]')
    if scale is not None and _chk(scale, name='scale').numel() != n_ch:
        raise ValueError(f'gconv3x3_wgrad: scale must hold {n_ch} values')
    if out is None:
        if accumulate:
            raise ValueError('gconv3x3_wgrad: accumulate needs `out`')
        out = torch.empty((n_ch, Cg, 3, 3), device=x.device, dtype=torch.float32)
    if _chk(out, name='out').numel() != n_ch * Cg * 9:
        raise ValueError(f'gconv3x3_wgrad: out must hold [{n_ch},{Cg},3,3]')
    d.g, d.x, d.out = g.data_ptr(), x.data_ptr(), out.data_ptr()
    d.g_ld, d.x_ld = g.shape[3], x_ld
    d.scale = scale.data_ptr() if scale is not None else None
    if y is not None:
        d.y, d.y_ld = y.data_ptr(), y.shape[3]
    d.accumulate = int(bool(accumulate))
    need = C.c_longlong()
    check(lib().nbm_gconv3x3_wgrad_workspace(C.byref(d), C.byref(need)), 'nbm_gconv3x3_wgrad_workspace')
    ws = _gconv_workspace(x.device, need.value) if workspace is None else workspace
    if not (ws.is_cuda and ws.dtype == torch.uint8 and ws.is_contiguous() and ws.numel() >= need.value):
        raise ValueError(f'gconv3x3_wgrad: workspace must be a contiguous uint8 device tensor of at least {need.value} bytes')
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    if FLOPS is not None:
        FLOPS[0] += 2.0 * 9 * Cg * n_ch * B * d.Ho * d.Wo
    with _timed(('gconv_wgrad', B, H, W, Cg, n_ch, kh, stride, groups)):
        check(lib().nbm_gconv3x3_wgrad(C.byref(d), _stream()), 'nbm_gconv3x3_wgrad')
    return out


def relu_bwd(gy, y):
    out = torch.empty_like(gy)
    check(lib().nbm_relu_bwd(_ptr(_chk(gy)), _ptr(_chk(y)), _ptr(out), gy.numel(), _stream()), 'nbm_relu_bwd')
    return out


def leaky_relu_bwd(gy, y, slope=0.01):
    out = torch.empty_like(gy)
    check(lib().nbm_leaky_relu_bwd(_ptr(_chk(gy)), _ptr(_chk(y)), _ptr(out), float(slope), gy.numel(), _stream()),
          'nbm_leaky_relu_bwd')
    return out


def layernorm_bwd(x2d, w, g2d, eps=1e-5):
    """-> (gx [rows,E], gw [E], gb [E])."""
    if deterministic():
        return layernorm_bwd_det(x2d, w, g2d, eps)
    rows, E = x2d.shape
    gx = torch.empty_like(x2d)
    gwb = torch.zeros((2, E), device=x2d.device, dtype=torch.float32)
    check(lib().nbm_layernorm_bwd(_ptr(_chk(x2d)), _ptr(_chk(w)), _ptr(_chk(g2d)), rows, E, float(eps), _ptr(gx), _ptr(gwb[0]),
                                  _ptr(gwb[1]), _stream()), 'nbm_layernorm_bwd')
    return gx, gwb[0], gwb[1]


def mha_small_bwd(q, k, v, go, S, N, nhead, seq_stride, batch_stride, n_valid=None):
    """Gradients of `mha_small` wrt q, k, v (2-D row views, any row pitch) -> contiguous [S*N, E] each.  S <= MHA_SLONG.  The
    workspace is 8 * N * nhead * S * S bytes (`mha_plan(...).workspace_bytes`), allocated here for the call: 8 MiB per (entry,
    head) at S = 1024."""
    E = q.shape[1]
    hd = E // nhead
    gq, gk, gv = (torch.zeros((q.shape[0], E), device=q.device, dtype=torch.float32) for _ in range(3))
    ws = torch.empty((N * nhead, 2, S, S), device=q.device, dtype=torch.float32)
    go = _chk(go)
    check(lib().nbm_mha_small_bwd(_ptr(q), _ptr(k), _ptr(v), _ptr(go), q.stride(0), k.stride(0), v.stride(0), go.stride(0),
                                  _ptr(gq), _ptr(gk), _ptr(gv), E, E, E, _ptr(ws), S, N, nhead, hd, seq_stride, batch_stride,
                                  _ptr(n_valid), 1.0 / math.sqrt(hd), _stream()), 'nbm_mha_small_bwd')
    return gq, gk, gv


def silu_bwd(gy, x):
    out = torch.empty_like(gy)
    check(lib().nbm_silu_bwd(_ptr(_chk(gy)), _ptr(_chk(x)), _ptr(out), gy.numel(), _stream()), 'nbm_silu_bwd')
    return out


def axpby(a, b=None, alpha=1.0, beta=1.0):
    """alpha*a + beta*b; a smaller `b` is repeated along the leading axes (its size must divide a's)."""
    out = torch.empty_like(a)
    period = 0
    if b is not None and b.numel() != a.numel():
        assert a.numel() % b.numel() == 0
        period = b.numel()
    check(lib().nbm_axpby(_ptr(_chk(a)), _ptr(b), _ptr(out), float(alpha), float(beta), a.numel(), period, _stream()),
          'nbm_axpby')
    return out


def weighted_sum(xs, weights):
    """BiFPN fusion of 2 or 3 same-shaped tensors with ReLU'd learnable weights [len(xs)] (device)."""
    x2 = xs[2] if len(xs) == 3 else None
    out = torch.empty_like(xs[0])
    check(lib().nbm_weighted_sum(_ptr(_chk(xs[0])), _ptr(_chk(xs[1])), _ptr(x2), _ptr(_chk(weights)), _ptr(out), out.numel(),
                                 _stream()), 'nbm_weighted_sum')
    return out


def weighted_sum_bwd(xs, weights, g, need):
    """-> ([gx_i or None], gw [len(xs)])."""
    x2 = xs[2] if len(xs) == 3 else None
    gxs = [torch.empty_like(x) if nd else None for x, nd in zip(xs, need)] + [None] * (3 - len(xs))
    gw = torch.zeros((len(xs),), device=g.device, dtype=torch.float32)
    _reduction('nbm_weighted_sum_bwd', (_ptr(_chk(xs[0])), _ptr(_chk(xs[1])), _ptr(x2), _ptr(_chk(weights)), _ptr(_chk(g)),
                                        _ptr(gxs[0]), _ptr(gxs[1]), _ptr(gxs[2]), _ptr(gw), g.numel()),
               lambda: _det_bytes(DET_WEIGHTED_SUM, g.numel()))
    return gxs[:len(xs)], gw


def colsum(g2d, n=None):
    """g2d [M, ld] -> [n] column sums (n defaults to ld)."""
    _chk(g2d, name='g')
    M, ld = g2d.shape
    n = ld if n is None else n
    out = torch.empty((n,), device=g2d.device, dtype=torch.float32)
    _reduction('nbm_colsum', (_ptr(g2d), M, n, ld, _ptr(out)), lambda: _det_bytes(DET_COLSUM, M, n))
    return out


def maxpool3x3s2_bwd(idx, gy, H, W, residual=None, mask=None):
    """`residual` [B,H,W,C]: added to the result (the gradient another consumer of the pooled tensor has produced); `mask`
    [B,H,W,C]: result *= (mask > 0) after that addition."""
    B, Ho, Wo, C_ = gy.shape
    gx = torch.empty((B, H, W, C_), device=gy.device, dtype=torch.float32)
    check(lib().nbm_maxpool3x3s2_bwd(_ptr(idx), _ptr(_chk(gy)), _ptr(gx), B, H, W, C_, Ho, Wo, _ptr(residual),
                                     _ptr(_chk(mask, name='mask')) if mask is not None else None, _stream()),
          'nbm_maxpool3x3s2_bwd')
    return gx


def upsample_bilinear_bwd(gy, Hi, Wi, pattern_stride=0, tiles_share=()):
    """d/d(coarse map) of the bilinear top-down merge.  `pattern_stride` = S: gy is zero outside the 5x5 patches around the 3x3 /
    stride-S pattern, only those are read; `tiles_share`: (compact [n][2][2][C], tile list, first image, images) entries whose
    bilinear backward is ADDED on top (the RoI share of a demand-driven level's gradient, kept out of gy -- ondemand.UPBWD_SPLIT)."""
    B, Ho, Wo, C_ = gy.shape
    gs = torch.empty((B, Hi, Wi, C_), device=gy.device, dtype=torch.float32)
    check(lib().nbm_upsample_bilinear_bwd(_ptr(_chk(gy)), B, Hi, Wi, C_, _ptr(gs), Ho, Wo, int(pattern_stride), _stream()),
          'nbm_upsample_bilinear_bwd')
    if tiles_share and deterministic():       # (ondemand.UPBWD_SPLIT is off in deterministic mode: nothing should get here)
        raise RuntimeError('nbm_tiles_upsample_bilinear_bwd_add is not reproducible under --deterministic')
    for compact, tiles, b0, nb in tiles_share:
        if compact.shape != (tiles.numel() * 4, C_) or b0 < 0 or b0 + nb > B:
            raise ValueError('upsample_bilinear_bwd: compact operand / tile list / image range do not fit the map')
        check(lib().nbm_tiles_upsample_bilinear_bwd_add(_ptr(_chk(compact)), nb, Ho, Wo, C_, _ptr(tiles), tiles.numel(), None,
                                                        C.c_void_p(gs.data_ptr() + b0 * Hi * Wi * C_ * 4), Hi, Wi, _stream()),
              'nbm_tiles_upsample_bilinear_bwd_add')
    return gs


def softmax_rows_bwd(p2d, gp2d, alpha=1.0):
    rows, cols = p2d.shape
    out = torch.empty_like(p2d)
    check(lib().nbm_softmax_rows_bwd(_ptr(_chk(p2d)), _ptr(_chk(gp2d)), _ptr(out), rows, cols, float(alpha), _stream()),
          'nbm_softmax_rows_bwd')
    return out


def pair_softmax_bwd(y, gy):
    gx = torch.empty_like(y)
    check(lib().nbm_pair_softmax_bwd(_ptr(_chk(y)), _ptr(_chk(gy)), _ptr(gx), y.numel() // 2, _stream()),
          'nbm_pair_softmax_bwd')
    return gx


def dwconv3x3_bwd(x, g, w, mult, stride, need_gx=True, need_gw=True, has_bias=True):
    B, H, W, Cin = x.shape
    Ho, Wo = g.shape[1], g.shape[2]
    gx = torch.empty_like(x) if need_gx else None
    gw = torch.empty((Cin * mult, 1, 3, 3), device=x.device, dtype=torch.float32) if need_gw else None
    gb = torch.empty((Cin * mult,), device=x.device, dtype=torch.float32) if (need_gw and has_bias) else None
    _reduction('nbm_dwconv3x3_bwd', (_ptr(_chk(x)), _ptr(_chk(g)), _ptr(_chk(w)), B, H, W, Cin, mult, stride, _ptr(gx),
                                     _ptr(gw), _ptr(gb), Ho, Wo), lambda: _det_bytes(DET_DWCONV, B * Ho * Wo, Cin * mult))
    return gx, gw, gb


def dwconv3x3_bwd_acc(g, w, mult, stride, gx):
    """gx [B,H,W,Cin] += data gradient of the depthwise 3x3 (only the pixels a tap reaches are touched)."""
    B, H, W, Cin = gx.shape
    check(lib().nbm_dwconv3x3_bwd_acc(_ptr(_chk(g)), _ptr(_chk(w)), B, H, W, Cin, mult, stride, _ptr(_chk(gx)), g.shape[1], g.shape[2],
                                      _stream()), 'nbm_dwconv3x3_bwd_acc')


def film_fwd(z, film):
    y = torch.empty_like(z)
    C_ = z.shape[-1]
    check(lib().nbm_film_fwd(_ptr(_chk(z)), _ptr(_chk(film)), _ptr(y), z.numel() // C_, C_, _stream()), 'nbm_film_fwd')
    return y


def film_bwd(gy, z, film):
    gz, gf = torch.empty_like(z), torch.empty_like(film)
    C_ = z.shape[-1]
    check(lib().nbm_film_bwd(_ptr(_chk(gy)), _ptr(_chk(z)), _ptr(_chk(film)), _ptr(gz), _ptr(gf), z.numel() // C_, C_,
                             _stream()), 'nbm_film_bwd')
    return gz, gf


def bn_train_fwd(x2d, w, b, eps, momentum, run_mean, run_var):
    """x2d [M,C] -> (y, mean, invstd); running stats updated in place."""
    M, C_ = x2d.shape
    ws = torch.empty((2 * C_,), device=x2d.device, dtype=torch.float64)
    mean = torch.empty((C_,), device=x2d.device, dtype=torch.float32)
    invstd = torch.empty_like(mean)
    y = torch.empty_like(x2d)
    _reduction('nbm_bn_train_fwd', (_ptr(_chk(x2d)), M, C_, _ptr(_chk(w)), _ptr(_chk(b)), float(eps), float(momentum),
                                    _ptr(run_mean), _ptr(run_var), _ptr(ws), _ptr(mean), _ptr(invstd), _ptr(y)),
               lambda: _det_bytes(DET_BN, M, C_))
    return y, mean, invstd


def bn_train_bwd(g2d, x2d, mean, invstd, w):
    M, C_ = x2d.shape
    ws = torch.empty((2 * C_,), device=x2d.device, dtype=torch.float64)
    gx = torch.empty_like(x2d)
    gw = torch.empty((C_,), device=x2d.device, dtype=torch.float32)
    gb = torch.empty_like(gw)
    _reduction('nbm_bn_train_bwd', (_ptr(_chk(g2d)), _ptr(_chk(x2d)), M, C_, _ptr(mean), _ptr(invstd), _ptr(_chk(w)), _ptr(ws),
                                    _ptr(gx), _ptr(gw), _ptr(gb)), lambda: _det_bytes(DET_BN, M, C_))
    return gx, gw, gb


def bn_act_plan(M, C_):
    """Host-only (no GPU needed): (partial-sum slots, workspace bytes) of `bn_act_train_fwd` / `bn_act_train_bwd` on [M, C] rows -- a
    function of (M, C) alone (nbm_bn_act_plan)."""
    parts, nbytes = C.c_int(0), C.c_int64(0)
    check(lib().nbm_bn_act_plan(int(M), int(C_), C.byref(parts), C.byref(nbytes)), 'nbm_bn_act_plan')
    return parts.value, nbytes.value


def _bn_act_workspace(M, C_, workspace, device):
    nbytes = bn_act_plan(M, C_)[1]
    if workspace is None:          # its previous contents are never read
        return torch.empty((nbytes,), device=device, dtype=torch.uint8), nbytes
    if not (workspace.is_cuda and workspace.is_contiguous() and workspace.numel() * workspace.element_size() >= nbytes):
        raise ValueError(f'bn_act: the workspace must be a contiguous device tensor of at least {nbytes} bytes')
    return workspace, nbytes


def bn_act_train_fwd(z2d, gamma, beta, eps, momentum, run_mean=None, run_var=None, residual=None, relu=False, workspace=None):
    """nn.BatchNorm2d in training mode over rows z2d [M, C] (+ residual [M, C]) (+ ReLU) -> (y, mean, invstd); the running statistics
    (both or neither) are updated in place (csrc/bnorm.hip)."""
    M, C_ = z2d.shape
    ws, nbytes = _bn_act_workspace(M, C_, workspace, z2d.device)
    mean = torch.empty((C_,), device=z2d.device, dtype=torch.float32)
    invstd = torch.empty_like(mean)
    y = torch.empty_like(z2d)
    if residual is not None and _chk(residual, name='residual').shape != z2d.shape:
        raise ValueError('bn_act_train_fwd: the residual must have the shape of z')
    for t, nm in ((gamma, 'gamma'), (beta, 'beta'), (run_mean, 'run_mean'), (run_var, 'run_var')):
        if t is not None and _chk(t, name=nm).numel() != C_:
            raise ValueError(f'bn_act_train_fwd: {nm} must hold {C_} values')
    check(lib().nbm_bn_act_train_fwd(_ptr(_chk(z2d, name='z')), M, C_, _ptr(gamma), _ptr(beta), float(eps), float(momentum),
                                     _ptr(run_mean), _ptr(run_var), _ptr(residual), int(bool(relu)), _ptr(ws), nbytes, _ptr(mean),
                                     _ptr(invstd), _ptr(y), _stream()), 'nbm_bn_act_train_fwd')
    return y, mean, invstd


def bn_act_train_bwd(gy2d, y2d, z2d, mean, invstd, gamma, relu=False, want_gres=False, workspace=None):
    """Gradients of `bn_act_train_fwd` -> (gz, ggamma, gbeta, gres or None).  `y2d`: the forward output (the ReLU mask; None without
    relu); `want_gres`: also write the masked gradient, which is the residual's."""
    M, C_ = z2d.shape
    ws, nbytes = _bn_act_workspace(M, C_, workspace, z2d.device)
    if relu and y2d is None:
        raise ValueError('bn_act_train_bwd: relu needs the forward output y')
    for t, nm in ((gy2d, 'gy'), (y2d, 'y')):
        if t is not None and _chk(t, name=nm).shape != z2d.shape:
            raise ValueError(f'bn_act_train_bwd: {nm} must have the shape of z')
    for t, nm in ((mean, 'mean'), (invstd, 'invstd'), (gamma, 'gamma')):
        if _chk(t, name=nm).numel() != C_:
            raise ValueError(f'bn_act_train_bwd: {nm} must hold {C_} values')
    gz = torch.empty_like(z2d)
    gw = torch.empty((C_,), device=z2d.device, dtype=torch.float32)
    gb = torch.empty_like(gw)
    gres = torch.empty_like(z2d) if want_gres else None
    check(lib().nbm_bn_act_train_bwd(_ptr(gy2d), _ptr(y2d if relu else None), _ptr(_chk(z2d, name='z')), M, C_, _ptr(mean), _ptr(invstd),
                                     _ptr(gamma), int(bool(relu)), _ptr(ws), nbytes, _ptr(gz), _ptr(gw), _ptr(gb), _ptr(gres),
                                     _stream()), 'nbm_bn_act_train_bwd')
    return gz, gw, gb, gres


def roi_pool_bwd(gpool, rois, level, fmap_shapes, pooled=None, bases=None):
    """gpool [B*R,ph,pw,C] -> list of zero-initialised-then-accumulated gradient maps (NHWC) for the FPN levels.
    `pooled` {level index: stride of the RPN's depthwise convolution on that map}: those maps come from the persistent pool of
    `ondemand.zero_acquire` (demand-driven levels: the consumer of the gradient recycles them) instead of a fresh fill.
    The pool size is gpool's; a 'dense' one (roi_pool_plan) takes no persistent map: the footprint re-zeroing knows the
    windows of ONDEMAND_POOL_HW alone."""
    B, R = rois.shape[:2]
    ph, pw, C_ = gpool.shape[1:]
    dense = roi_pool_plan(ph, pw, [s[1:3] for s in fmap_shapes]) == 'dense'
    if dense and (pooled or any(e is not None for _, e in (bases or {}).values())):
        raise NotImplementedError('roi_pool_bwd: persistent (demand-driven) gradient maps exist for the 2 x 2 pool only')
    gf = []
    for i, s in enumerate(fmap_shapes):
        buf = None
        if bases and i in bases:             # another consumer's share of this map's gradient (Fn._PARKED): scatter into it
            base, e = bases[i]
            if e is not None:                # a persistent map: the RoI windows join its footprint
                from . import ondemand
                ondemand.zero_note(e, lambda b_=base, s_=s, i_=i: check(lib().nbm_zero_roi_windows(
                    _ptr(b_), s_[1], s_[2], s_[3], _ptr(rois), _ptr(level), B, R, i_, _stream()), 'nbm_zero_roi_windows'))
                if ondemand.ZERO_POOL_CHECK:
                    e['check'] = _check_all_zero
            gf.append(base)
            continue
        if pooled and i in pooled:
            from . import ondemand
            buf, e = ondemand.zero_acquire(s, gpool.device, ('map-grad', pooled[i]))
        if buf is not None:
            # footprints: the RoI windows of this level, and the 3x3 blocks the strided taps add to (Fn.DwConv.backward)
            ondemand.zero_note(e, lambda b_=buf, s_=s, i_=i: check(lib().nbm_zero_roi_windows(
                _ptr(b_), s_[1], s_[2], s_[3], _ptr(rois), _ptr(level), B, R, i_, _stream()), 'nbm_zero_roi_windows'))
            ondemand.zero_note(e, lambda b_=buf, s_=s, st_=pooled[i]: check(lib().nbm_zero_pattern(
                _ptr(b_), s_[0], s_[1], s_[2], s_[3], st_, _stream()), 'nbm_zero_pattern'))
            if ondemand.ZERO_POOL_CHECK:
                e['check'] = _check_all_zero
            gf.append(buf)
        else:
            gf.append(torch.zeros(s, device=gpool.device, dtype=torch.float32))
    n = len(gf)
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in gf])
    fh = (C.c_int * n)(*[s[1] for s in fmap_shapes])
    fw = (C.c_int * n)(*[s[2] for s in fmap_shapes])
    _reduction('nbm_roi_pool_hw_bwd', (ptrs, fh, fw, n, C_, _ptr(_chk(rois)), _ptr(level), B, R, ph, pw, _ptr(_chk(gpool))))
    return gf


def zero_pattern(buf, stride):
    B, H, W, C_ = buf.shape
    check(lib().nbm_zero_pattern(_ptr(buf), B, H, W, C_, int(stride), _stream()), 'nbm_zero_pattern')


def _check_all_zero(buf):
    bad = float(buf.abs().max())
    if bad != 0.0:
        raise RuntimeError(f'persistent RoI-gradient map not clean after its recycle: {bad}')


def sqnorm_accum(g, out):
    _reduction('nbm_sqnorm_accum', (_ptr(g), g.numel(), _ptr(out)), lambda: _det_bytes(DET_SQNORM, g.numel()))


def adamw_step(p, g, m, v, lr, beta1, beta2, eps, wd, step, sqnorm=None, max_norm=0.0):
    check(lib().nbm_adamw_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), float(lr), float(beta1), float(beta2),
                               float(eps), float(wd), int(step), _ptr(sqnorm), float(max_norm), _stream()), 'nbm_adamw_step')
