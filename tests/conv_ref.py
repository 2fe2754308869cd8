"""Float64 reference of the convolution family the HIP GEMM kernels implement (include/nbm_hip.h: nbm_gemm_conv,
nbm_conv_dgrad, nbm_conv_wgrad).  Plain torch only -- nothing here calls the HIP library -- so it runs on any device; the
big cases run it in float64 on the GPU.  One float64 matmul per filter tap over a shifted / strided view of the padded map.

Layouts follow the kernels: activations NHWC [..., B, H, W, C], weights KRSC [..., N, kh * kw * C] (column (r * kw + s) * C + c).
Leading dimensions before B (and before N of the weights) are groups: they broadcast through torch.matmul.

`abs_ref(fn, ...)` runs the same operation on |operands|: the per-element scale of the rounding-error bounds."""
import torch


def _f64(t):
    return None if t is None else t.to(torch.float64)


def out_size(H, W, kh, kw, stride, pad):
    return (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1


def _tap_view(xp, r, s, Ho, Wo, stride):
    """Rows r, r + stride, ... and columns s, s + stride, ... of the padded map: the input pixels under tap (r, s)."""
    return xp[..., r:r + stride * (Ho - 1) + 1:stride, s:s + stride * (Wo - 1) + 1:stride, :]


def _pad(x, pad, extra_h=0, extra_w=0):
    """Zero padding of an NHWC map (pad rows / columns in front, pad + extra behind)."""
    *lead, B, H, W, C = x.shape
    xp = x.new_zeros((*lead, B, H + 2 * pad + extra_h, W + 2 * pad + extra_w, C))
    xp[..., pad:pad + H, pad:pad + W, :] = x
    return xp


def conv(x, w, *, kh=1, kw=1, stride=1, pad=0, Ho=None, Wo=None, scale=None, shift=None, alpha=1.0, residual=None,
         relu=False, mask=None):
    """y = relu?(alpha * conv(x, w) * scale[n] + shift[n] + residual), then 0 where mask <= 0 (nbm_gemm_conv's epilogue order).
    x [..., B, H, W, C], w [..., N, kh * kw * C] -> [..., B, Ho, Wo, N]."""
    x, w = _f64(x), _f64(w)
    *_, B, H, W, C = x.shape
    N = w.shape[-2]
    assert w.shape[-1] == kh * kw * C, (w.shape, kh, kw, C)
    ho, wo = out_size(H, W, kh, kw, stride, pad)
    Ho, Wo = ho if Ho is None else Ho, wo if Wo is None else Wo
    xp = _pad(x, pad, max(0, stride * (Ho - 1) + kh - H - 2 * pad), max(0, stride * (Wo - 1) + kw - W - 2 * pad))
    y = None
    for r in range(kh):
        for s in range(kw):
            t = r * kw + s
            p = torch.matmul(_tap_view(xp, r, s, Ho, Wo, stride).reshape(*x.shape[:-4], -1, C),
                             w[..., t * C:(t + 1) * C].transpose(-1, -2))
            y = p if y is None else y.add_(p)
    y = y.reshape(*x.shape[:-4], B, Ho, Wo, N) * alpha
    if scale is not None:
        y = y * _f64(scale)
    if shift is not None:
        y = y + _f64(shift)
    if residual is not None:
        y = y + _f64(residual)
    if relu:
        y = y.clamp_min(0)
    if mask is not None:
        y = torch.where(mask > 0, y, y.new_zeros(()))
    return y


def dgrad(g, w, *, H, W, kh=1, kw=1, stride=1, pad=0, a_scale=None, alpha=1.0, residual=None, residual2=None, mask=None):
    """dX[b, iy, ix, c] = alpha * sum_{r, s, n} g[b, oy, ox, n] a_scale[n] w[n, (r, s, c)] over iy = oy * stride - pad + r (and the same
    for x), + residual, + residual2 at the even / even pixels, then 0 where mask <= 0 (nbm_conv_dgrad's epilogue order).
    g [..., B, Ho, Wo, N], w [..., N, kh * kw * C] -> [..., B, H, W, C]."""
    g, w = _f64(g), _f64(w)
    *lead, B, Ho, Wo, N = g.shape
    C = w.shape[-1] // (kh * kw)
    assert w.shape[-2] == N and w.shape[-1] == kh * kw * C
    if a_scale is not None:
        g = g * _f64(a_scale)
    outp = _pad(g.new_zeros((*lead, B, H, W, C)), pad, max(0, stride * (Ho - 1) + kh - H - 2 * pad),
                max(0, stride * (Wo - 1) + kw - W - 2 * pad))
    g2 = g.reshape(*lead, -1, N)
    for r in range(kh):
        for s in range(kw):
            t = r * kw + s
            p = torch.matmul(g2, w[..., t * C:(t + 1) * C]).reshape(*lead, B, Ho, Wo, C)
            _tap_view(outp, r, s, Ho, Wo, stride).add_(p)
    dx = outp[..., pad:pad + H, pad:pad + W, :] * alpha
    if residual is not None:
        dx = dx + _f64(residual)
    if residual2 is not None:
        dx[..., 0::2, 0::2, :] += _f64(residual2)
    if mask is not None:
        dx = torch.where(mask > 0, dx, dx.new_zeros(()))
    return dx


def wgrad(g, x, *, kh=1, kw=1, stride=1, pad=0, row_scale=None, alpha=1.0, out=None, bias_grad=None):
    """dW[n, (r, s, c)] = out[n, (r, s, c)] + alpha * row_scale[n] * sum_m g[m, n] x[pix(m) + (r, s), c]; with `bias_grad` also returns
    bias_grad + sum_m g[m, n].  g [..., B, Ho, Wo, N], x [..., B, H, W, C] -> ([..., N, kh * kw * C], [..., N] or None)."""
    g, x = _f64(g), _f64(x)
    *lead, B, Ho, Wo, N = g.shape
    C = x.shape[-1]
    H, W = x.shape[-3:-1]
    xp = _pad(x, pad, max(0, stride * (Ho - 1) + kh - H - 2 * pad), max(0, stride * (Wo - 1) + kw - W - 2 * pad))
    gT = g.reshape(*lead, -1, N).transpose(-1, -2)
    cols = [torch.matmul(gT, _tap_view(xp, r, s, Ho, Wo, stride).reshape(*lead, -1, C)) for r in range(kh) for s in range(kw)]
    dw = torch.cat(cols, -1) * alpha
    if row_scale is not None:
        dw = dw * _f64(row_scale)[..., None]
    if out is not None:
        dw = dw + _f64(out)
    gb = None
    if bias_grad is not None:
        gb = _f64(bias_grad) + g.reshape(*lead, -1, N).sum(-2)
    return dw, gb


def abs_ref(fn, *args, **kw):
    """The same operation on |every tensor operand| (masks keep their sign: they select, they do not scale): the sum of the
    magnitudes of the terms of each output element, the scale of a rounding-error bound."""
    a = [t.abs() if torch.is_tensor(t) else t for t in args]
    k = {n: (v.abs() if torch.is_tensor(v) and n != 'mask' else v) for n, v in kw.items()}
    if 'alpha' in k:
        k['alpha'] = abs(k['alpha'])
    return fn(*a, **k)


def sq_ref(fn, *args, **kw):
    """The same operation on the squares of every tensor operand (and alpha^2; masks keep their sign): sum_k (a_k b_k)^2 per output
    element, the square of the l2 norm of its terms -- the scale of an rms rounding-error bound."""
    a = [t.to(torch.float64).square() if torch.is_tensor(t) else t for t in args]
    k = {n: (v.to(torch.float64).square() if torch.is_tensor(v) and n != 'mask' else v) for n, v in kw.items()}
    if 'alpha' in k:
        k['alpha'] = k['alpha'] ** 2
    return fn(*a, **k)
