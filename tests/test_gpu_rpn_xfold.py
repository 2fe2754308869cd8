"""GPU: the level-0 RPN operand without its horizontal interpolation (`nbm_cell_patches_up_cols`, the grouped links of
`ondemand.rpn_composite`, `_prep.rpn_composite_xfold`) -- the kernel bit for bit against its fp32 expression, the folded route against
the route through the 25-plane patches and against float64 of the reference's chain of layers (layers.py:13-46 behind fpn.py:137-145),
and one captured detect step with the fold on."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from birdsoundclassif_amd import ondemand, ops, synth                                  # noqa: E402
from birdsoundclassif_amd.nets import _prep                                            # noqa: E402
from helpers import filler_state_dict                                                  # noqa: E402


def rnd(key, *shape, scale=1.0):
    return torch.from_numpy((synth.normal(key, int(np.prod(shape))) * scale).astype(np.float32).reshape(shape))


def test_column_window_kernel_equals_its_fp32_expression_bit_for_bit():
    """Every plane 4 j + s of every cell: (hy * x1[y0][xb + s] + ly * x1[y1][xb + s]) + bias, op by op in numpy float32; exactly 0 where
    the patch row lies outside the image or no in-image pixel reads the column; nothing else written (NaN poison), layout
    [OW][20][B * OH][C]."""
    B, H, W, Hc, Wc, S, Ch = 3, 21, 33, 11, 17, 8, 32
    OH, OW = (H - 1) // S + 1, (W - 1) // S + 1
    x1 = rnd('xf-x1', B, Hc, Wc, Ch)
    bias = rnd('xf-b', Ch)
    V = torch.full((OW, 20, B * OH, Ch), float('nan'), device='cuda')
    guard = torch.full((4096,), float('nan'), device='cuda')
    buf = torch.cat([V.reshape(-1), guard])                        # the kernel's output followed by poison it must not touch
    x1d, bd = x1.cuda(), bias.cuda()
    rc = ops.lib().nbm_cell_patches_up_cols(C.c_void_p(x1d.data_ptr()), C.c_void_p(bd.data_ptr()), B, H, W, Ch, Hc, Wc, S,
                                            C.c_void_p(buf.data_ptr()), ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[V.numel():]).all())
    got = buf[:V.numel()].view(OW, 20, B, OH, Ch).cpu().numpy()
    xbase, used, _ = _prep.xfold_columns(W, Wc, S)
    f32 = np.float32
    sh = f32(Hc - 1) / f32(H - 1)
    a, bn = x1.numpy(), bias.numpy()
    want = np.zeros_like(got)
    unused = np.ones(got.shape[:4], dtype=bool)
    for oy in range(OH):
        for j in range(5):
            y = S * oy - 2 + j
            if not 0 <= y < H:
                continue
            fy = f32(sh * f32(y))
            y0 = int(fy)
            y1 = y0 + (1 if y0 < Hc - 1 else 0)
            ly = f32(min(max(f32(fy - f32(y0)), f32(0.0)), f32(1.0)))
            hy = f32(f32(1.0) - ly)
            for ox in range(OW):
                for s in range(4):
                    if used[ox, s]:
                        xs = int(xbase[ox]) + s
                        want[ox, 4 * j + s, :, oy] = (hy * a[:, y0, xs] + ly * a[:, y1, xs]) + bn[None, :]
                        unused[ox, 4 * j + s, :, oy] = False
    assert want.dtype == np.float32 and 0 < int(unused.sum()) < unused.size
    assert not np.isnan(got).any()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not got[unused].view(np.uint32).any()                   # +0.0, bit for bit
    # a ratio the 20 planes cannot hold is refused, not computed
    rc = ops.lib().nbm_cell_patches_up_cols(C.c_void_p(x1d.data_ptr()), C.c_void_p(bd.data_ptr()), 1, 11, 17, Ch, Hc, Wc, S,
                                            C.c_void_p(buf.data_ptr()), ops._stream())
    assert rc != 0


def _composite(shape, fold):
    """The existing composite test's set-up (test_gpu_lazy.py): block(y) on a demand-driven map with a pending pattern pass.
    -> (f, float64 reference, number of batch chunks that took the folded route)."""
    import torch.nn.functional as F
    from birdsoundclassif_amd.nets.layers import DepthwiseSepConv2d
    B, H, W, Cin, Ch, N, S, deferred = shape
    wo = rnd(('xwo', shape), N, Ch, 3, 3, scale=0.05).cuda()
    bo = rnd(('xbo', shape), N).cuda()
    blk = DepthwiseSepConv2d(N, N, stride=S, expansion_fact=2).cuda().eval()
    with torch.no_grad():
        for k_, p_ in blk.named_parameters():
            p_.copy_(rnd(('xblk', k_, shape), *p_.shape, scale=0.3 if p_.dim() > 1 else 0.5).cuda())
        blk.norm.weight.add_(1.0)
        blk.norm.running_mean.copy_(rnd(('xbm', shape), N, scale=0.2).cuda())
        blk.norm.running_var.copy_(rnd(('xbv', shape), N).abs().cuda() + 0.5)
    if deferred:
        t = rnd(('xt', shape), B, H, W, Cin).cuda()
        wl = rnd(('xwl', shape), Ch, Cin, 1, 1, scale=0.1).cuda()
        bl = rnd(('xbl', shape), Ch).cuda()
        up = rnd(('xup', shape), B, (H + 1) // 2, (W + 1) // 2, Ch).cuda()
        alpha = 2.0
        merged = ops.conv2d(t, _prep.krsc(wl), shift=bl, alpha=alpha, up=up)
    else:
        merged = rnd(('xx', shape), B, H, W, Ch).cuda()
    with torch.no_grad():
        md = merged.double().permute(0, 3, 1, 2)
        o = F.conv2d(md, wo.double(), bo.double(), padding=1)
        d = F.conv2d(o, blk.depth_wise.weight.double(), blk.depth_wise.bias.double(), stride=S, padding=1, groups=N)
        p = F.conv2d(d, blk.pt_wise.weight.double(), blk.pt_wise.bias.double())
        p = (p - blk.norm.running_mean.double()[None, :, None, None]) / \
            torch.sqrt(blk.norm.running_var.double() + blk.norm.eps)[None, :, None, None] \
            * blk.norm.weight.double()[None, :, None, None] + blk.norm.bias.double()[None, :, None, None]
        ref = (p * torch.sigmoid(p)).permute(0, 2, 3, 1)
    keep, calls = ondemand.XFOLD, ondemand.XFOLD_CALLS[0]
    ondemand.XFOLD, ondemand.LAZY_POISON = fold, True
    try:
        with torch.no_grad():
            x = ondemand.conv1x1_lazy(t, _prep.krsc(wl), bl, alpha, up, S, defer=True) if deferred else merged
            y, st = ondemand.conv3x3_winograd_lazy(x, _prep.wino23(wo), bo, S, _prep.cell_weight(wo, forward=True),
                                                   fold=lambda wk, a_, transposed=False: _prep.cell_weight_folded(wo, wk, a_, transposed),
                                                   raw=(wo, bo))
            assert st.pending is not None
            f = blk(y)
            assert st.pending is not None and bool(torch.isnan(y).all()), 'the composite route wrote pattern pixels'
    finally:
        ondemand.XFOLD, ondemand.LAZY_POISON = keep, False
    torch.cuda.synchronize()
    return f, ref, ondemand.XFOLD_CALLS[0] - calls


def test_folded_route_against_the_patch_route_and_float64():
    """B = 3 on the 21 x 33 map: 3 x 5 cells per image, groups of 9 rows (far from a tile multiple), a right-most cell column with a
    depthwise tap AND patch pixels outside the image, the clamped last source column.  The folded route must not be the less accurate
    one: its rms error against float64 at most 1.05 x that of the patch route on the same inputs (the criterion of the composite's own
    test); the top row, the left column and the corner cell, whose weights differ, within that test's bound on their own."""
    shape = (3, 21, 33, 32, 64, 32, 8, True)
    f_on, ref, n_on = _composite(shape, True)
    f_off, _, n_off = _composite(shape, False)
    assert (n_on, n_off) == (1, 0)
    assert tuple(f_on.shape) == tuple(ref.shape) == tuple(f_off.shape) and bool(torch.isfinite(f_on).all())
    e1, e2 = (f_on.double() - ref).abs(), (f_off.double() - ref).abs()
    scale_ = max(1.0, float(ref.abs().max()))
    r1, r2 = float((e1 ** 2).mean().sqrt()), float((e2 ** 2).mean().sqrt())
    print(f'rms error against float64: folded {r1:.3e}, patch route {r2:.3e}; max {float(e1.max()):.3e} / {float(e2.max()):.3e}; '
          f'top row {float(e1[:, 0].max()):.3e}, left column {float(e1[:, :, 0].max()):.3e}, corner {float(e1[:, 0, 0].max()):.3e}, '
          f'right column {float(e1[:, :, -1].max()):.3e}')
    assert float(e1.max()) <= 2e-5 * scale_
    assert float(e1[:, 0].max()) <= 2e-5 * scale_ and float(e1[:, :, 0].max()) <= 2e-5 * scale_ and float(e1[:, 0, 0].max()) <= 2e-5 * scale_
    assert float(e1[:, :, -1].max()) <= 2e-5 * scale_
    assert r1 <= 1.05 * r2, f'folded rms error {r1:.3e} vs patch route {r2:.3e}'


def test_a_level_without_deferred_lateral_keeps_its_route_and_its_bits():
    shape = (2, 33, 41, 0, 64, 64, 4, False)
    f_on, _, n_on = _composite(shape, True)
    f_off, _, n_off = _composite(shape, False)
    assert (n_on, n_off) == (0, 0) and torch.equal(f_on, f_off)


def test_captured_detect_step_with_the_fold_replays_to_the_eager_result():
    """One GraphedDetector at B = 2: the folded weights are built in the warm-up steps, the capture holds kernel nodes only (the detector
    refuses anything else) and its replay gives the eager step's detections bit for bit."""
    from birdsoundclassif_amd import bulk
    from birdsoundclassif_amd.nbm_datasets.prepare_dataset import SpectrogramFrontEnd
    from birdsoundclassif_amd.nets import build_model
    from birdsoundclassif_amd.train import default_args
    assert ondemand.XFOLD
    model, _ = build_model(default_args(device='cuda'))
    model.load_state_dict(filler_state_dict())
    model = model.cuda().eval()
    pcm = torch.from_numpy(synth.clip_batch_pcm16(300, 2)).cuda()
    calls = ondemand.XFOLD_CALLS[0]
    with torch.no_grad():
        imgs, _ = SpectrogramFrontEnd('cuda')(pcm, 22050)
        det, n = model.detect_calls(imgs[:, 0][:, None].contiguous(), None, 0.3, 0.05)
        det, n = det.clone(), n.clone()
    assert ondemand.XFOLD_CALLS[0] > calls and int(n.sum()) > 0
    g = bulk.GraphedDetector(model, 2, 66150, 22050, min_score=0.05)
    try:
        assert g.census['kernel'] > 0 and not any(v for k, v in g.census.items() if k not in ('kernel', 'empty'))
        g.pcm.copy_(pcm)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(g.n_det, n) and torch.equal(g.det, det)
    finally:
        g.close()
