"""CPU: the horizontal half of the top-down interpolation folded into the composed RPN weights -- `_prep.xfold_columns` /
`xfold64` / `rpn_composite_xfold`.  The five pixels of a patch row of up(x1) are fixed combinations of at most four source columns per
cell column; the weights of the columns reproduce, in float64, what the weights of the pixels give on the interpolated row, and the
whole folded route (column classes in the group weights, one delta per border row, the lateral's input on the gathered border route)
reproduces the reference's chain of layers on every cell."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from birdsoundclassif_amd import ondemand
from birdsoundclassif_amd.nets import _prep

# (W, Wc, S): the production levels, odd sizes, a clamped last column (x0 == Wc - 1: 41 / 21, 33 / 17) and a right-most cell with patch
# pixels outside the image (33 / 17 at stride 8: pixels 33 and 34 of cell column 4)
GEOMS = [(512, 256, 8), (188, 94, 8), (512, 256, 4), (100, 50, 8), (37, 19, 8), (64, 33, 8), (21, 11, 3), (41, 21, 8), (33, 17, 8)]


def _rnd(seed, *shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def _pixel_taps(W, Wc, x):
    """(x0, x1, hx, lx) of pixel x, op by op in float32 as the kernels evaluate them."""
    f32 = np.float32
    sw = f32(Wc - 1) / f32(W - 1)
    fx = f32(sw * f32(min(max(x, 0), W - 1)))
    x0 = int(fx)
    x1 = x0 + (1 if x0 < Wc - 1 else 0)
    lx = f32(min(max(f32(fx - f32(x0)), f32(0.0)), f32(1.0)))
    return x0, x1, float(f32(f32(1.0) - lx)), float(lx)


@pytest.mark.parametrize('geom', GEOMS)
def test_weights_of_the_columns_equal_weights_of_the_interpolated_pixels(geom):
    W, Wc, S = geom
    got = _prep.xfold_columns(W, Wc, S)
    assert got is not None
    xbase, used, cx = got
    OW = (W - 1) // S + 1
    assert xbase.shape == (OW,) and used.shape == (OW, 4) and cx.shape == (OW, 5, 4)
    N, C = 6, 8
    we = _rnd(1, N, 5, 5, C)                                      # [N][patch row][pixel][C]
    wf = _prep.xfold64(we, torch.from_numpy(cx))                  # [OW][N][5][4][C]
    src = _rnd(2, 5, Wc, C)                                       # a patch row's source values, per patch row: [j][column][C]
    saw_clamped = saw_outside = False
    for ox in range(OW):
        patch = torch.zeros(5, 5, C, dtype=torch.float64)
        cols = set()
        for l in range(5):
            x = S * ox - 2 + l
            if not 0 <= x < W:
                saw_outside = saw_outside or x >= W
                continue
            x0, x1, hx, lx = _pixel_taps(W, Wc, x)
            saw_clamped = saw_clamped or x0 == x1
            patch[:, l] = hx * src[:, x0] + lx * src[:, x1]
            cols |= {x0, x1}
        # the window: consecutive columns from the first one read, at most four, and `used` names exactly the columns read
        assert min(cols) == xbase[ox] and max(cols) - min(cols) < 4
        assert {int(xbase[ox]) + s for s in range(4) if used[ox, s]} == cols
        window = torch.zeros(5, 4, C, dtype=torch.float64)
        for s in range(4):
            if used[ox, s]:
                window[:, s] = src[:, xbase[ox] + s]
            else:
                assert not wf[ox][:, :, s].any()                  # an unused slot has no weight (and the kernel writes 0 there)
        want = torch.einsum('njlc,jlc->n', we, patch)
        have = torch.einsum('njsc,jsc->n', wf[ox], window)
        assert float((want - have).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), (ox, float((want - have).abs().max()))
    if geom == (33, 17, 8):
        assert saw_clamped and saw_outside
    if geom == (41, 21, 8):
        assert saw_clamped


def test_a_ratio_far_from_one_half_has_no_window():
    assert _prep.xfold_columns(64, 64, 8) is None                 # ratio 1: five pixels read six columns
    assert _prep.xfold_columns(64, 48, 8) is None
    assert _prep.rpn_composite_xfold(*[torch.zeros(4, 4, 3, 3)] * 7, 64, 64, 8, (7,) * 8) is None


@pytest.mark.parametrize('geom', [(2, 21, 33, 8, 8), (1, 17, 41, 8, 4), (2, 17, 21, 3, 4)])
def test_folded_route_reproduces_the_chain_of_layers(geom):
    """The launches of `ondemand.rpn_composite`'s folded route restated in float64 torch, against the reference's layers with the merged
    map formed by torch's own align-corners bilinear upsampling."""
    B, H, W, S, Cin = geom
    C, N, mult = 8, 8, 2
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    out_w, out_b = _rnd(1, N, C, 3, 3, scale=0.2).float(), _rnd(2, N).float()
    dw_w, dw_b = _rnd(3, mult * N, 1, 3, 3, scale=0.4).float(), _rnd(4, mult * N).float()
    pt_w, pt_b = _rnd(5, N, mult * N, 1, 1, scale=0.3).float(), _rnd(6, N).float()
    bn_w, bn_b, bn_m, bn_v = 1 + _rnd(7, N, scale=0.1).float(), _rnd(8, N, scale=0.1).float(), _rnd(9, N, scale=0.2).float(), \
        _rnd(10, N).abs().float() + 0.5
    t, wl, bl, alpha = _rnd(11, B, Cin, H, W), _rnd(12, C, Cin, scale=0.3).float(), _rnd(13, C), 2.0
    x1 = _rnd(14, B, C, Hc, Wc)
    x = alpha * torch.einsum('ck,bkhw->bchw', wl.double(), t) + bl[None, :, None, None] + \
        F.interpolate(x1, size=(H, W), mode='bilinear', align_corners=True)
    o = F.conv2d(x, out_w.double(), out_b.double(), padding=1)
    d = F.conv2d(o, dw_w.double(), dw_b.double(), stride=S, padding=1, groups=N)
    p = F.conv2d(d, pt_w.double(), pt_b.double())
    scale, shift = _prep.bn_affine(bn_w, bn_b, bn_m, bn_v, 1e-5, conv_bias=pt_b)
    ref = (p - pt_b.double()[None, :, None, None]) * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]
    wargs = (out_w, out_b, dw_w, dw_b, pt_w, scale, shift)
    wkw = dict(lat_wk=wl, alpha=alpha)
    K = C + Cin
    OH, OW = (H - 1) // S + 1, (W - 1) // S + 1
    rm, sm = ondemand._tap_masks(H, W, S)
    xbase, used, _ = _prep.xfold_columns(W, Wc, S)
    # the operand of nbm_cell_patches_up_cols: D[b][oy][ox][j][s][c]
    D = torch.zeros(B, OH, OW, 5, 4, C, dtype=torch.float64)
    for oy in range(OH):
        for j in range(5):
            y = S * oy - 2 + j
            if not 0 <= y < H:
                continue
            fy = y * (Hc - 1) / (H - 1)
            y0 = min(int(fy), Hc - 1)
            y1 = min(y0 + 1, Hc - 1)
            row = (1 - (fy - y0)) * x1[:, :, y0] + (fy - y0) * x1[:, :, y1] + bl[None, :, None]          # [B, C, Wc]
            for ox in range(OW):
                for s in range(4):
                    if used[ox, s]:
                        D[:, oy, ox, j, s] = row[:, :, xbase[ox] + s]
    wf = _prep.rpn_composite_xfold(*wargs, W, Wc, S, sm, **wkw)
    assert tuple(wf.shape) == (OW, N, 20 * C)
    (_, w_t), sc, sh = _prep.rpn_composite(*wargs, **wkw, parts=((0, C), (C, K)))
    pre = torch.einsum('gnk,bogk->bnog', wf.double(), D.reshape(B, OH, OW, 20 * C))
    pre = pre + F.conv2d(t, w_t.double().reshape(N, 5, 5, Cin).permute(0, 3, 1, 2), stride=S, padding=2)
    pre = pre * sc.double()[None, :, None, None] + sh.double()[None, :, None, None]
    flat = pre.reshape(B, N, OH * OW).clone()
    patches = F.unfold(t, 5, padding=2, stride=S).reshape(B, Cin, 25, OH * OW)
    for rmask, smask, taps, _, idx, _ in ondemand._border_classes(B, H, W, S, 'cpu'):
        dwt, dsh = _prep.rpn_composite_delta_part(*wargs, rmask, smask, taps, C, K, **wkw)
        cells = idx[: idx.numel() // B]
        pv = patches[:, :, list(taps)][..., cells]
        flat[:, :, cells] += torch.einsum('ntk,bktc->bnc', dwt.double().reshape(N, len(taps), Cin), pv) + dsh.double()[None, :, None]
    got = flat.reshape(B, N, OH, OW)
    rows_seen = 0
    for oy in range(OH):
        if rm[oy] == 7:
            continue
        a_rows = tuple(a for a in range(5) if 0 <= S * oy - 2 + a < H and any(0 <= a - r <= 2 for r in range(3) if not (rm[oy] >> r) & 1))
        dwf = _prep.rpn_composite_xfold(*wargs, W, Wc, S, sm, rows=(rm[oy], a_rows), **wkw)
        assert tuple(dwf.shape) == (len(a_rows), OW, N, 4 * C)
        for i, a in enumerate(a_rows):
            got[:, :, oy] += torch.einsum('gnk,bgk->bng', dwf[i].double(), D[:, oy, :, a].reshape(B, OW, 4 * C))
        rows_seen += 1
    assert rows_seen >= 1 and len(set(sm)) >= 2                   # a border row and a border column class took part
    err = float((got - ref).abs().max())
    assert err < 5e-6 * max(1.0, float(ref.abs().max())), err     # (weights rounded to fp32 once; fp32 interpolation coefficients)
    # the border cells need their terms: the top row, the left column and the corner on their own
    for sl in ((slice(None), slice(None), 0), (slice(None), slice(None), slice(None), 0), (slice(None), slice(None), 0, 0)):
        assert float((got[sl] - ref[sl]).abs().max()) < 5e-6 * max(1.0, float(ref.abs().max()))
