"""CPU: the float64 convolution reference of tests/conv_ref.py against torch.nn.functional.conv2d and its autograd, at small odd
shapes covering every tap / stride / pad / group combination of the B = 128 launch table (tests/test_gpu_train_geometry.py)."""
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R

# (kh, kw, stride, pad, groups): 1x1 s1 / s2, 3x3 s1 / s2 pad 1, 7x7 s2 pad 3 (the stem), the 5 x 1 composite planes, grouped GEMMs
CASES = [(1, 1, 1, 0, 1), (1, 1, 2, 0, 1), (3, 3, 1, 1, 1), (3, 3, 2, 1, 1), (7, 7, 2, 3, 1), (5, 1, 1, 0, 5), (1, 1, 1, 0, 3),
         (3, 3, 2, 1, 2)]


def _torch_ref(x, w, kh, kw, stride, pad):
    """x [G, B, H, W, C], w [G, N, kh * kw * C] (KRSC) -> [G, B, Ho, Wo, N] through F.conv2d (NCHW / OIHW)."""
    G, B, H, W, C = x.shape
    N = w.shape[1]
    out = [F.conv2d(x[g].permute(0, 3, 1, 2), w[g].view(N, kh, kw, C).permute(0, 3, 1, 2), stride=stride, padding=pad)
           for g in range(G)]
    return torch.stack([o.permute(0, 2, 3, 1) for o in out])


def _data(kh, kw, stride, pad, G, seed=0):
    g = torch.Generator().manual_seed(seed)
    B, H, W, C, N = 2, 9, 11, 5, 7
    x = torch.randn((G, B, H, W, C), generator=g, dtype=torch.float64)
    w = torch.randn((G, N, kh * kw * C), generator=g, dtype=torch.float64)
    return x, w, g


@pytest.mark.parametrize('kh,kw,stride,pad,G', CASES)
def test_forward_matches_conv2d(kh, kw, stride, pad, G):
    x, w, gen = _data(kh, kw, stride, pad, G)
    N = w.shape[1]
    scale, shift = torch.randn(N, generator=gen, dtype=torch.float64), torch.randn(N, generator=gen, dtype=torch.float64)
    ref = _torch_ref(x, w, kh, kw, stride, pad)
    res = torch.randn(ref.shape, generator=gen, dtype=torch.float64)
    mask = torch.randint(-1, 2, ref.shape, generator=gen).double()
    got = R.conv(x, w, kh=kh, kw=kw, stride=stride, pad=pad, scale=scale, shift=shift, alpha=0.5, residual=res, relu=True, mask=mask)
    want = torch.where(mask > 0, (0.5 * ref * scale + shift + res).clamp_min(0), torch.zeros(()))
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    # the gradient wrt x and w of <ref, gy> through autograd is the data / weight gradient
    xg, wg = x.clone().requires_grad_(), w.clone().requires_grad_()
    y = _torch_ref(xg, wg, kh, kw, stride, pad)
    gy = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    dx, dw = torch.autograd.grad((y * gy).sum(), (xg, wg))
    H, W = x.shape[2:4]
    torch.testing.assert_close(R.dgrad(gy, w, H=H, W=W, kh=kh, kw=kw, stride=stride, pad=pad), dx, rtol=1e-12, atol=1e-12)
    got_w, _ = R.wgrad(gy, x, kh=kh, kw=kw, stride=stride, pad=pad)
    torch.testing.assert_close(got_w, dw, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('kh,kw,stride,pad,G', CASES)
def test_dgrad_epilogue(kh, kw, stride, pad, G):
    """a_scale scales g per output channel, alpha the sum; residual is added everywhere, residual2 at the even / even pixels, then
    the mask zeroes where mask <= 0 (zeros included)."""
    x, w, gen = _data(kh, kw, stride, pad, G, seed=1)
    B, H, W, C = x.shape[1:]
    N = w.shape[1]
    gy = torch.randn(_torch_ref(x, w, kh, kw, stride, pad).shape, generator=gen, dtype=torch.float64)
    a = torch.randn(N, generator=gen, dtype=torch.float64)
    res = torch.randn((G, B, H, W, C), generator=gen, dtype=torch.float64)
    res2 = torch.randn((G, B, (H + 1) // 2, (W + 1) // 2, C), generator=gen, dtype=torch.float64)
    mask = torch.randint(-1, 2, (G, B, H, W, C), generator=gen).double()
    base = R.dgrad(gy * a, w, H=H, W=W, kh=kh, kw=kw, stride=stride, pad=pad)
    want = 2.0 * base + res
    want[..., 0::2, 0::2, :] += res2
    want = torch.where(mask > 0, want, torch.zeros(()))
    got = R.dgrad(gy, w, H=H, W=W, kh=kh, kw=kw, stride=stride, pad=pad, a_scale=a, alpha=2.0, residual=res, residual2=res2, mask=mask)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    assert bool((got[mask <= 0] == 0).all())


@pytest.mark.parametrize('kh,kw,stride,pad,G', CASES)
def test_wgrad_epilogue(kh, kw, stride, pad, G):
    """row_scale and alpha scale the sum, `out` is accumulated into, bias_grad += column sums of g."""
    x, w, gen = _data(kh, kw, stride, pad, G, seed=2)
    N = w.shape[1]
    gy = torch.randn(_torch_ref(x, w, kh, kw, stride, pad).shape, generator=gen, dtype=torch.float64)
    rs = torch.randn(N, generator=gen, dtype=torch.float64)
    pre = torch.randn(w.shape, generator=gen, dtype=torch.float64)
    gb0 = torch.randn((G, N), generator=gen, dtype=torch.float64)
    base, _ = R.wgrad(gy, x, kh=kh, kw=kw, stride=stride, pad=pad)
    got, gb = R.wgrad(gy, x, kh=kh, kw=kw, stride=stride, pad=pad, row_scale=rs, alpha=0.5, out=pre, bias_grad=gb0)
    torch.testing.assert_close(got, pre + 0.5 * base * rs[:, None], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(gb, gb0 + gy.sum((1, 2, 3)), rtol=1e-12, atol=1e-12)


def test_explicit_output_size_and_shared_group_operand():
    """Ho / Wo given explicitly (the kh x 1 composite planes: Ho = 1) and a group stride of 0 (one operand shared by all groups)."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn((1, 1, 5, 13, 4), generator=g, dtype=torch.float64).expand(3, 1, 5, 13, 4)
    w = torch.randn((3, 6, 5 * 4), generator=g, dtype=torch.float64)
    got = R.conv(x, w, kh=5, kw=1, Ho=1, Wo=13)
    want = torch.einsum('gbhwc,gnhc->gbwn', x, w.view(3, 6, 5, 4))[:, :, None]
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)


def test_abs_ref_is_the_magnitude_sum():
    g = torch.Generator().manual_seed(4)
    x = torch.randn((1, 2, 6, 7, 3), generator=g, dtype=torch.float64)
    w = torch.randn((1, 5, 27), generator=g, dtype=torch.float64)
    a = R.abs_ref(R.conv, x, w, kh=3, kw=3, pad=1, alpha=-2.0)
    torch.testing.assert_close(a, R.conv(x.abs(), w.abs(), kh=3, kw=3, pad=1, alpha=2.0))
    assert bool((a >= R.conv(x, w, kh=3, kw=3, pad=1, alpha=-2.0).abs() - 1e-12).all())
