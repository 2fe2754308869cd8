"""GPU: `nbm_gconv3x3_dgrad` / `nbm_gconv3x3_wgrad` (csrc/gconv_bwd.hip), the gradients of the grouped 3x3 convolution of the ResNeXt
bottleneck, against float64 autograd through F.conv2d(groups=...) (tests/gconv_bwd_ref.py), with the shapes and rules of
tests/test_gpu_gconv.py (pixel tiles: 8 x 16 / 4 x 16 gradient pixels for the data gradient at stride 1 / 2, 4 x 16 / 2 x 16 for the
weight gradient; a workgroup takes 64 channels):

* integer operands (|x|, |w|, |g| <= 3, scale a signed power of two, y a random sign pattern): every partial sum is exact in fp32
  (data gradient: K <= 576 terms of at most 18; weight gradient: at most 273 pixels of at most 9, then the scale) -> BIT equality in
  any summation order, so also for every split count;
* randn operands -> |got - ref64| <= 8 sqrt(K) 2^-24 abs_ref + 1e-30 per element, K = 9 Cg (data) / B Ho Wo (weights), abs_ref the same
  gradient of the absolute values."""
import math

import pytest
import torch

import gconv_bwd_ref
from birdsoundclassif_amd import _lib, ops
from birdsoundclassif_amd.nets import _prep

pytestmark = pytest.mark.gpu

GROUPS = [(32, 4), (32, 8), (32, 16), (32, 32), (32, 64), (64, 4)]          # (G, Cg)
# forward INPUT maps, those of test_gpu_gconv.py plus (1,4,6): even H and W at stride 2
MAPS = {1: [(1, 1, 3), (2, 5, 7), (3, 7, 13), (1, 9, 17), (1, 4, 6)], 2: [(1, 1, 3), (2, 5, 7), (3, 7, 13), (1, 9, 33), (1, 4, 6)]}
PREC_C, TINY = 8.0, 1e-30


def _gen(seed):
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    return g


def _out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def _operands(G, Cg, shape, stride, gen, randn):
    """-> x [B,H,W,C], w [C,Cg,3,3], g [B,Ho,Wo,C], scale [C], y [B,Ho,Wo,C] (a random sign pattern)."""
    C = G * Cg
    B, H, W = shape
    Ho, Wo = _out_hw(H, W, stride)
    y = torch.randn(B, Ho, Wo, C, generator=gen, device='cuda')
    if randn:
        mk = lambda *s: torch.randn(*s, generator=gen, device='cuda')
        return mk(B, H, W, C), mk(C, Cg, 3, 3), mk(B, Ho, Wo, C), mk(C), y
    ri = lambda *s: torch.randint(-3, 4, s, generator=gen, device='cuda').float()
    scale = torch.tensor([0.5, 1.0, 2.0, -1.0], device='cuda')[torch.randint(0, 4, (C,), generator=gen, device='cuda')]
    return ri(B, H, W, C), ri(C, Cg, 3, 3), ri(B, Ho, Wo, C), scale, y


def _close(got, ref, abs_ref, K, what):
    bound = PREC_C * math.sqrt(K) * 2.0 ** -24 * abs_ref + TINY
    worst = float(((got.double().cpu() - ref).abs() / bound).max())
    print(f'{what}: max err / bound = {worst:.3f}')
    assert worst <= 1.0, f'{what}: error is {worst:.2f} x the bound'


def _exact(got, ref, what):
    got = got.double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.equal(got, ref), f'{what}: {int((got != ref).sum())} of {ref.numel()} elements differ'


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('G,Cg', GROUPS)
def test_every_group_width_at_the_edges(G, Cg, stride):
    gen = _gen(100 * Cg + G + stride)
    for shape in MAPS[stride]:
        B, H, W = shape
        Ho, Wo = _out_hw(H, W, stride)
        for randn in (False, True):
            x, w, g, scale, y = _operands(G, Cg, shape, stride, gen, randn)
            for masked in (False, True):
                s, ym = (scale, y) if masked else (None, None)
                what = f'G={G} Cg={Cg} stride={stride} map={shape} y+scale={masked} randn={randn}'
                ref_gx, ref_gw = gconv_bwd_ref.gconv_grads(x, w, G, g, stride, s, ym)
                gx = ops.gconv3x3_dgrad(g, _prep.gconv_dgrad(w, G, s), G, H, W, stride=stride, y=ym)
                assert tuple(gx.shape) == (B, H, W, G * Cg)
                plan = ops.gconv_wgrad_plan(B, Ho, Wo, G, Cg, stride)[0]
                gws = {sp: ops.gconv3x3_wgrad(g, x, G, stride=stride, scale=s, y=ym, splits=sp) for sp in (1, 2, 5, None)}
                assert all(tuple(v.shape) == (G * Cg, Cg, 3, 3) for v in gws.values())
                if not randn:
                    _exact(gx, ref_gx, 'dgrad ' + what)
                    for sp, v in gws.items():
                        _exact(v, ref_gw, f'wgrad splits={sp} ' + what)
                    prefill = torch.randint(-5, 6, ref_gw.shape, generator=gen, device='cuda').float()
                    out = prefill.clone()
                    ret = ops.gconv3x3_wgrad(g, x, G, stride=stride, scale=s, y=ym, out=out, accumulate=True, splits=2)
                    assert ret is out
                    _exact(out, prefill.double().cpu() + ref_gw, 'wgrad accumulate ' + what)
                else:
                    abs_gx, abs_gw = gconv_bwd_ref.gconv_grads_abs(x, w, G, g, stride, s, ym)
                    _close(gx, ref_gx, abs_gx, 9 * Cg, 'dgrad ' + what)
                    for sp, v in gws.items():
                        _close(v, ref_gw, abs_gw, B * Ho * Wo, f'wgrad splits={sp} (plan {plan}) ' + what)


@pytest.mark.parametrize('stride', [1, 2])
def test_pixel_pitches_wider_than_the_channels(stride):
    """g_ld, x_ld, y_ld, out_ld > C: the pad columns of the inputs (1e30) are not read as channels, those of gx keep their sentinel."""
    G, Cg = 32, 4
    C = G * Cg
    gen = _gen(7 + stride)
    shape = (2, 5, 7)
    B, H, W = shape
    for randn in (False, True):
        x, w, g, scale, y = _operands(G, Cg, shape, stride, gen, randn)

        def wide(t, pad):
            out = torch.full((*t.shape[:3], C + pad), 1e30, device='cuda')
            out[..., :C] = t
            return out
        xw, gw_, yw = wide(x, 12), wide(g, 8), wide(y, 4)
        out = torch.full((B, H, W, C + 20), -777.0, device='cuda')
        ret = ops.gconv3x3_dgrad(gw_, _prep.gconv_dgrad(w, G, scale), G, H, W, stride=stride, y=yw, out=out)
        assert ret is out
        assert bool((out[..., C:] == -777.0).all()), 'pad columns of gx were written'
        dw = ops.gconv3x3_wgrad(gw_, xw, G, stride=stride, scale=scale, y=yw)
        dw_c = ops.gconv3x3_wgrad(gw_, xw, G, stride=stride, y=yw, channels=C)
        ref_gx, ref_gw = gconv_bwd_ref.gconv_grads(x, w, G, g, stride, scale, y)
        _, ref_gw_c = gconv_bwd_ref.gconv_grads(x, w, G, g, stride, None, y)
        if not randn:
            _exact(out[..., :C], ref_gx, f'pitched dgrad stride={stride}')
            _exact(dw, ref_gw, f'pitched wgrad stride={stride}')
            _exact(dw_c, ref_gw_c, f'pitched wgrad without scale stride={stride}')
        else:
            abs_gx, abs_gw = gconv_bwd_ref.gconv_grads_abs(x, w, G, g, stride, scale, y)
            _close(out[..., :C], ref_gx, abs_gx, 9 * Cg, f'pitched dgrad stride={stride}')
            _close(dw, ref_gw, abs_gw, B * ref_gx.shape[1] * ref_gx.shape[2], f'pitched wgrad stride={stride}')


@pytest.mark.parametrize('stride', [1, 2])
def test_wgrad_is_reproducible_and_ignores_what_the_workspace_held(stride):
    G, Cg = 32, 8
    gen = _gen(31 + stride)
    shape = (3, 7, 13)
    x, w, g, scale, y = _operands(G, Cg, shape, stride, gen, True)
    Ho, Wo = _out_hw(7, 13, stride)
    for sp in (None, 5):
        nbytes = (ops.gconv_wgrad_plan(3, Ho, Wo, G, Cg, stride)[0] if sp is None else sp) * G * Cg * 9 * 16 * 4
        ws_nan = torch.full((nbytes // 4,), float('nan'), device='cuda').view(torch.uint8)
        ws_zero = torch.zeros(nbytes, dtype=torch.uint8, device='cuda')
        a = ops.gconv3x3_wgrad(g, x, G, stride=stride, scale=scale, y=y, splits=sp, workspace=ws_nan)
        b = ops.gconv3x3_wgrad(g, x, G, stride=stride, scale=scale, y=y, splits=sp, workspace=ws_zero)
        c = ops.gconv3x3_wgrad(g, x, G, stride=stride, scale=scale, y=y, splits=sp)
        d = ops.gconv3x3_wgrad(g, x, G, stride=stride, scale=scale, y=y, splits=sp)
        assert torch.isfinite(a).all()
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(c, d), f'splits={sp}: two runs differ'
    with pytest.raises(ValueError, match='workspace'):
        ops.gconv3x3_wgrad(g, x, G, stride=stride, splits=5, workspace=torch.zeros(64, dtype=torch.uint8, device='cuda'))


def test_small_launch_after_a_large_one_touches_only_its_output():
    """A small launch into the front of a buffer that a large launch filled changes nothing behind its own output; the same for the
    weight gradient's workspace."""
    G, Cg = 32, 8
    C = G * Cg
    gen = _gen(11)
    x, w, g, _, _ = _operands(G, Cg, (2, 19, 37), 1, gen, False)
    wp = _prep.gconv_dgrad(w, G)
    buf = torch.empty(2 * 19 * 37 * C, device='cuda')
    big = ops.gconv3x3_dgrad(g, wp, G, 19, 37, out=buf.view(2, 19, 37, C))
    _exact(big, gconv_bwd_ref.gconv_grads(x, w, G, g)[0], 'large dgrad')
    before = buf.clone()
    gs = g[:1, :3, :5].contiguous()
    n = 3 * 5 * C
    small = ops.gconv3x3_dgrad(gs, wp, G, 3, 5, out=buf[:n].view(1, 3, 5, C))
    xs = x[:1, :3, :5].contiguous()
    _exact(small, gconv_bwd_ref.gconv_grads(xs, w, G, gs)[0], 'small dgrad')
    assert torch.equal(buf[n:], before[n:]), 'the small data gradient wrote outside its output'
    # weight gradient: the large launch fills a workspace, the small one (one split) writes its front only
    per_split = C * 9 * 16 * 4
    ws = torch.zeros(8 * per_split, dtype=torch.uint8, device='cuda')
    ops.gconv3x3_wgrad(g, x, G, splits=8, workspace=ws)
    held = ws.clone()
    out = torch.full((C * Cg * 9 + 64,), -777.0, device='cuda')
    ops.gconv3x3_wgrad(gs, xs, G, splits=1, workspace=ws, out=out[:C * Cg * 9], channels=C)
    _exact(out[:C * Cg * 9].view(C, Cg, 3, 3), gconv_bwd_ref.gconv_grads(xs, w, G, gs)[1], 'small wgrad')
    assert bool((out[C * Cg * 9:] == -777.0).all()), 'the small weight gradient wrote behind its output'
    assert torch.equal(ws[per_split:], held[per_split:]), 'the small weight gradient wrote behind its split of the workspace'


def test_unsupported_descriptors_raise_and_launch_nothing():
    gen = _gen(3)
    # Cg = 12: the prepared shape is what such a weight would take
    g12 = torch.randn(1, 4, 4, 32 * 12, generator=gen, device='cuda')
    out12 = torch.full((1, 4, 4, 32 * 12), -777.0, device='cuda')
    dw12 = torch.full((32 * 12, 12, 3, 3), -777.0, device='cuda')
    with pytest.raises(_lib.NbmHipError, match='NBM_EUNSUPPORTED'):
        ops.gconv3x3_dgrad(g12, torch.zeros(32 * 12 // 16, 9, 1, 64, 4, device='cuda'), 32, 4, 4, out=out12)
    with pytest.raises(_lib.NbmHipError, match='NBM_EUNSUPPORTED'):
        ops.gconv3x3_wgrad(g12, g12, 32, out=dw12)
    # stride 3
    x, w, _, _, _ = _operands(32, 4, (1, 6, 6), 1, gen, True)
    g3 = torch.randn(1, 2, 2, 128, generator=gen, device='cuda')
    out = torch.full((1, 6, 6, 128), -777.0, device='cuda')
    dw = torch.full((128, 4, 3, 3), -777.0, device='cuda')
    with pytest.raises(_lib.NbmHipError, match='NBM_EUNSUPPORTED'):
        ops.gconv3x3_dgrad(g3, _prep.gconv_dgrad(w, 32), 32, 6, 6, stride=3, out=out)
    with pytest.raises(_lib.NbmHipError, match='NBM_EUNSUPPORTED'):
        ops.gconv3x3_wgrad(g3, x, 32, stride=3, out=dw)
    # a pointer that is not 16-byte aligned (a view one float into a buffer)
    flat = torch.zeros(6 * 6 * 128 + 4, device='cuda')
    mis = flat[1:1 + 6 * 6 * 128].view(1, 6, 6, 128)
    with pytest.raises(_lib.NbmHipError, match='NBM_EUNSUPPORTED'):
        ops.gconv3x3_dgrad(mis, _prep.gconv_dgrad(w, 32), 32, 6, 6, out=out)
    with pytest.raises(_lib.NbmHipError, match='NBM_EUNSUPPORTED'):
        ops.gconv3x3_wgrad(mis, x, 32, out=dw)
    with pytest.raises(_lib.NbmHipError, match='NBM_EUNSUPPORTED'):
        ops.gconv3x3_wgrad(x, mis, 32, out=dw)
    torch.cuda.synchronize()
    for t in (out12, dw12, out, dw):
        assert bool((t == -777.0).all()), 'a refused call wrote its output'
