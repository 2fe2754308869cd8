"""GPU: `nbm_gconv3x3` (csrc/gconv.hip), the grouped 3x3 convolution of the ResNeXt bottleneck, against the float64 reference
tests/gconv_ref.py at the smallest shapes at which the kernel can go wrong (its pixel tile is 8 x 16 outputs at stride 1 and 4 x 16 at
stride 2, a workgroup takes 64 channels):

* integer operands small enough that every partial sum is exact in fp32 (|x|, |w| <= 3, K <= 576: below 2^13; scale a signed power of
  two, shift an integer) -> BIT equality in any summation order: groups, taps, borders, strides and pitches;
* randn operands -> |got - ref64| <= 8 sqrt(K) 2^-24 abs_ref + 1e-30 per element, K = 9 Cg, abs_ref the same convolution of the absolute
  values (PREC_C / _prec_bound of test_gpu_train_geometry.py, restated)."""
import math

import pytest
import torch

import gconv_ref
from birdsoundclassif_amd import _lib, ops
from birdsoundclassif_amd.nets import _prep

pytestmark = pytest.mark.gpu

GROUPS = [(32, 4), (32, 8), (32, 16), (32, 32), (32, 64), (64, 4)]          # (G, Cg)
# (1,1,3): taps mostly outside; (2,5,7): odd, stride 2 rounds up; (3,7,13): 273 pixels, no multiple of any tile; the last: one pixel
# more than a pixel tile in each direction (stride 1: 8 x 16 outputs; stride 2: 4 x 16 outputs = 8 x 32 inputs), the halo crosses a seam
MAPS = {1: [(1, 1, 3), (2, 5, 7), (3, 7, 13), (1, 9, 17)], 2: [(1, 1, 3), (2, 5, 7), (3, 7, 13), (1, 9, 33)]}
PREC_C, TINY = 8.0, 1e-30


def _gen(seed):
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    return g


def _operands(G, Cg, shape, gen, randn):
    C = G * Cg
    if randn:
        mk = lambda *s: torch.randn(*s, generator=gen, device='cuda')
        return mk(*shape, C), mk(C, Cg, 3, 3), mk(C), mk(C)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen, device='cuda').float()
    scale = torch.tensor([0.5, 1.0, 2.0, -1.0], device='cuda')[torch.randint(0, 4, (C,), generator=gen, device='cuda')]
    return ri(-3, 3, *shape, C), ri(-3, 3, C, Cg, 3, 3), scale, ri(-4, 4, C)


def _check(got, x, w, G, stride, scale, shift, relu, randn, what):
    ref = gconv_ref.gconv(x, w, G, stride=stride, scale=scale, shift=shift, relu=relu)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not randn:
        assert torch.equal(got.double(), ref), f'{what}: {int((got.double() != ref).sum())} of {ref.numel()} elements differ'
        return
    K = 9 * w.shape[1]
    bound = PREC_C * math.sqrt(K) * 2.0 ** -24 * gconv_ref.gconv_abs(x, w, G, stride=stride, scale=scale, shift=shift, relu=relu) + TINY
    err = (got.double() - ref).abs()
    worst = float((err / bound).max())
    print(f'{what}: max err / bound = {worst:.3f}')
    assert worst <= 1.0, f'{what}: error is {worst:.2f} x the bound'


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('G,Cg', GROUPS)
def test_every_group_width_at_the_edges(G, Cg, stride):
    gen = _gen(100 * Cg + G + stride)
    for shape in MAPS[stride]:
        for randn in (False, True):
            x, w, scale, shift = _operands(G, Cg, shape, gen, randn)
            wp = _prep.gconv(w, G)
            assert tuple(wp.shape) == (G * Cg // 16, 9, max(Cg, 16) // 16, 64, 4)
            for epi in (False, True):
                s, b = (scale, shift) if epi else (None, None)
                got = ops.gconv3x3(x, wp, G, stride=stride, scale=s, shift=b, relu=epi)
                _check(got, x, w, G, stride, s, b, epi, randn, f'G={G} Cg={Cg} stride={stride} map={shape} epilogue={epi} randn={randn}')


@pytest.mark.parametrize('stride', [1, 2])
def test_pixel_pitches_wider_than_the_channels(stride):
    """x_ld > C and y_ld > C: the pad columns of the input are not read as channels, those of the output keep their sentinel."""
    G, Cg, pad_x, pad_y = 32, 4, 12, 20
    C = G * Cg
    gen = _gen(7 + stride)
    for randn in (False, True):
        x, w, scale, shift = _operands(G, Cg, (2, 5, 7), gen, randn)
        xw = torch.full((2, 5, 7, C + pad_x), 1e30, device='cuda')
        xw[..., :C] = x
        Ho, Wo = (5 - 1) // stride + 1, (7 - 1) // stride + 1
        out = torch.full((2, Ho, Wo, C + pad_y), -777.0, device='cuda')
        ret = ops.gconv3x3(xw, _prep.gconv(w, G), G, stride=stride, scale=scale, shift=shift, relu=True, out=out)
        assert ret is out
        assert bool((out[..., C:] == -777.0).all()), 'pad columns of the output were written'
        _check(out[..., :C].contiguous(), x, w, G, stride, scale, shift, True, randn, f'pitched stride={stride} randn={randn}')


def test_unsupported_descriptors_raise_and_launch_nothing():
    gen = _gen(3)
    # Cg = 12: no checkpoint of the supported architectures has it; the prepared shape is what such a weight would take
    x = torch.randn(1, 4, 4, 32 * 12, generator=gen, device='cuda')
    out = torch.full((1, 4, 4, 32 * 12), -777.0, device='cuda')
    with pytest.raises(_lib.NbmHipError, match='NBM_EUNSUPPORTED'):
        ops.gconv3x3(x, torch.zeros(32 * 12 // 16, 9, 1, 64, 4, device='cuda'), 32, out=out)
    with pytest.raises(ValueError):
        _prep.gconv(torch.zeros(32 * 12, 12, 3, 3, device='cuda'), 32)
    # a 5x5 kernel, another padding, stride 3
    x, w, _, _ = _operands(32, 4, (1, 6, 6), gen, True)
    out2 = torch.full((1, 6, 6, 128), -777.0, device='cuda')
    for kw in (dict(kh=5, kw=5, pad=2), dict(pad=0, out=None), dict(stride=3, out=None)):
        with pytest.raises(_lib.NbmHipError, match='NBM_EUNSUPPORTED'):
            ops.gconv3x3(x, _prep.gconv(w, 32), 32, **{'out': out2, **kw})
    # a pointer that is not 16-byte aligned (a view one float into a buffer)
    flat = torch.zeros(1 * 6 * 6 * 128 + 4, device='cuda')
    with pytest.raises(_lib.NbmHipError, match='NBM_EUNSUPPORTED'):
        ops.gconv3x3(flat[1:1 + 6 * 6 * 128].view(1, 6, 6, 128), _prep.gconv(w, 32), 32, out=out2)
    torch.cuda.synchronize()
    assert bool((out == -777.0).all()) and bool((out2 == -777.0).all()), 'a refused call wrote its output'
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.gconv3x3(torch.zeros(1, 4, 4, 128), torch.zeros(8, 9, 1, 64, 4), 32)


def test_small_launch_after_a_large_one_touches_only_its_output():
    """The kernel keeps no workspace: a small launch into the front of a buffer that a large launch filled changes nothing behind
    its own output."""
    G, Cg = 32, 8
    C = G * Cg
    gen = _gen(11)
    x, w, _, _ = _operands(G, Cg, (2, 19, 37), gen, False)
    wp = _prep.gconv(w, G)
    buf = torch.empty(2 * 19 * 37 * C, device='cuda')
    big = ops.gconv3x3(x, wp, G, out=buf.view(2, 19, 37, C))
    _check(big, x, w, G, 1, None, None, False, False, 'large')
    before = buf.clone()
    xs = x[:1, :3, :5].contiguous()
    n = 3 * 5 * C
    small = ops.gconv3x3(xs, wp, G, out=buf[:n].view(1, 3, 5, C))
    _check(small, xs, w, G, 1, None, None, False, False, 'small')
    assert torch.equal(buf[n:], before[n:]), 'the small launch wrote outside its output'
