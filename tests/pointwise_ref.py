"""Float64 references of the point-wise kernels (csrc/pointwise.hip, csrc/pointwise_bwd.hip), for tests/test_gpu_pointwise_edges.py.

Every function takes the fp32 operands the kernel takes (NHWC maps, row-major matrices; torch tensors or numpy arrays on the host),
computes in float64 and returns `(value, absref)` pairs: `absref` is the same computation carried out on the absolute values of every
operand and product, so that a bound `k * 2^-24 * absref` follows cancellation (a sum of large terms of both signs has a small value and
a large absref).  Where torch has the operation the value IS torch in float64; the hand-written formulas (everything a kernel defines
on operands torch never sees: saved statistics, a recorded softmax, a clip coefficient) are checked against torch float64 autograd or
an independent formulation in tests/test_pointwise_ref_cpu.py.  No GPU is needed anywhere in this module."""
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24          # unit round-off of fp32 (round to nearest)
U64 = 2.0 ** -53


def t64(x):
    """Any operand -> a float64 torch tensor on the host (fp32 values are carried over exactly)."""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    return x.detach().cpu().double()


def to_nchw(x):
    return t64(x).permute(0, 3, 1, 2).contiguous()


def to_nhwc(x):
    return x.detach().permute(0, 2, 3, 1).contiguous()


# --------------------------------------------------------------------------- bilinear (align_corners=True)
def bilinear_fwd(src, Ho, Wo, add=None):
    """src [B,Hi,Wi,C] -> [B,Ho,Wo,C] (+ add).  The weights are non-negative: absref = the same interpolation of |src| (+ |add|)."""
    s = to_nchw(src)
    v = F.interpolate(s, size=(Ho, Wo), mode='bilinear', align_corners=True)
    a = F.interpolate(s.abs(), size=(Ho, Wo), mode='bilinear', align_corners=True)
    if add is not None:
        v, a = v + to_nchw(add), a + to_nchw(add).abs()
    return to_nhwc(v), to_nhwc(a)


def bilinear_bwd(gy, Hi, Wi):
    """gy [B,Ho,Wo,C] -> d/d(src) [B,Hi,Wi,C] through float64 autograd."""
    g = to_nchw(gy)
    B, C, Ho, Wo = g.shape
    out = []
    for gg in (g, g.abs()):
        s = torch.zeros(B, C, Hi, Wi, dtype=torch.float64, requires_grad=True)
        F.interpolate(s, size=(Ho, Wo), mode='bilinear', align_corners=True).backward(gg)
        out.append(to_nhwc(s.grad))
    return out[0], out[1]


def bilinear_matrix(n_in, n_out):
    """[n_out, n_in] float64 interpolation matrix of one axis (align_corners=True): an independent formulation of the operator, and
    the contributor count per coarse index (its column-wise non-zeros)."""
    m = np.zeros((n_out, n_in))
    for o in range(n_out):
        f = o * (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
        p0 = min(int(math.floor(f)), n_in - 1)
        p1 = min(p0 + 1, n_in - 1)
        l = f - p0
        m[o, p0] += 1.0 - l
        m[o, p1] += l
    return m


def bilinear_axis_f32(n_coarse, n_fine):
    """One axis in the kernels' own arithmetic: the host's fp32 scale s = (n_coarse - 1) / (n_fine - 1) and, per coarse index, how many
    fine indices o give it a non-zero weight at the fp32 position fl(s * o) -> (s, [count])."""
    f32 = np.float32
    s = f32(n_coarse - 1) / f32(n_fine - 1) if n_fine > 1 else f32(0)
    cnt = [0] * n_coarse
    for o in range(n_fine):
        f = f32(s * f32(o))
        p0 = int(f)
        p1 = p0 + (1 if p0 < n_coarse - 1 else 0)
        l = min(max(f32(f - f32(p0)), f32(0)), f32(1))
        if float(f32(1) - l) != 0.0 or p1 == p0:
            cnt[p0] += 1
        if float(l) != 0.0 and p1 != p0:
            cnt[p1] += 1
    return s, cnt


def bilinear_position_absref(t, Hi, Wi, Ho, Wo, backward):
    """What an error of the fp32 POSITION s * o can reach.  The product is rounded at its own magnitude (up to n_coarse - 1) and s carries
    its own rounding, so a position is off by d <= 2 * 2^-24 * max(Hi, Wi); a weight w = wy * wx then is off by <= 2 d, and that on
    every coarse neighbour the position can be moved onto -- including one whose exact weight is 0: scaling 32 -> 8 columns, fl(s * 7)
    = 30.999998 gives column 30 the weight 2e-6 where exact arithmetic (and float64 torch) gives it none.  -> the operator with weight 1
    on the support of the exact operator widened by one coarse index, on |t|: [B,Ho,Wo,C] (forward) or [B,Hi,Wi,C] (backward); the
    caller multiplies by 4 * 2^-24 * max(Hi, Wi).  Only needed when down-sampling: up-sampling positions are rounded below the
    magnitude of o, and every coarse index has neighbours of full weight in `absref` already (the 3 * max(Ho, Wo) term)."""
    def wide(n_in, n_out):
        m = bilinear_matrix(n_in, n_out) != 0
        d = m.copy()
        d[:, 1:] |= m[:, :-1]
        d[:, :-1] |= m[:, 1:]
        return torch.from_numpy(d.astype(np.float64))
    Ny, Nx = wide(Hi, Ho), wide(Wi, Wo)
    return torch.einsum('oy,px,bopc->byxc' if backward else 'oy,px,byxc->bopc', Ny, Nx, t64(t).abs())


# --------------------------------------------------------------------------- softmax rows
def softmax_rows(x):
    """x [rows, cols] -> softmax over the last axis; every term is positive: absref = value."""
    v = torch.softmax(t64(x), -1)
    return v, v.clone()


def softmax_rows_bwd(p, gp, alpha=1.0):
    """dS = P * (dP - sum(P * dP)) * alpha on the recorded fp32 P."""
    p, g = t64(p), t64(gp)
    v = p * (g - (p * g).sum(-1, keepdim=True)) * alpha
    a = p.abs() * (g.abs() + (p.abs() * g.abs()).sum(-1, keepdim=True)) * abs(alpha)
    return v, a


def pair_softmax(x, n_anchor):
    """x [n_pix, ld >= 2 * n_anchor] -> softmax over each (bg, fg) pair of the first 2 * n_anchor columns."""
    x = t64(x)
    v = x[:, :2 * n_anchor].reshape(x.shape[0], n_anchor, 2).softmax(-1).reshape(x.shape[0], 2 * n_anchor)
    return v, v.clone()


def pair_softmax_bwd(y, gy):
    y, g = t64(y), t64(gy)
    n = y.shape[-1] // 2
    v, a = softmax_rows_bwd(y.reshape(-1, n, 2), g.reshape(-1, n, 2))
    return v.reshape(y.shape), a.reshape(y.shape)


# --------------------------------------------------------------------------- LayerNorm
def _ln_parts(x, eps):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh_abs = (x.abs() + x.abs().mean(-1, keepdim=True)) * rstd        # |x| + |mean| <= |x| + mean|x|
    return mean, rstd, xh_abs


def layernorm(x, w, b, eps=1e-5):
    x, w, b = t64(x), t64(w), t64(b)
    _, _, xh_abs = _ln_parts(x, eps)
    return F.layer_norm(x, (x.shape[-1],), w, b, eps), xh_abs * w.abs() + b.abs()


def layernorm_bwd(x, w, g, eps=1e-5):
    """-> (gx, gw, gb), each a (value, absref) pair: gx = rstd * (g w - mean(g w) - xhat mean(g w xhat)), gw = sum g xhat, gb = sum g."""
    x, w, g = t64(x), t64(w), t64(g)
    mean, rstd, xh_abs = _ln_parts(x, eps)
    xh = (x - mean) * rstd
    gw_ = g * w
    gx = rstd * (gw_ - gw_.mean(-1, keepdim=True) - xh * (gw_ * xh).mean(-1, keepdim=True))
    gx_a = rstd * (gw_.abs() + gw_.abs().mean(-1, keepdim=True) + xh_abs * (gw_.abs() * xh_abs).mean(-1, keepdim=True))
    return (gx, gx_a), ((g * xh).sum(0), (g.abs() * xh_abs).sum(0)), (g.sum(0), g.abs().sum(0))


# --------------------------------------------------------------------------- element-wise
def silu(x):
    x = t64(x)
    v = x * torch.sigmoid(x)
    return v, v.abs()


def silu_bwd(gy, x):
    g, x = t64(gy), t64(x)
    s = torch.sigmoid(x)
    return g * (s * (1 + x * (1 - s))), g.abs() * (s * (1 + x.abs() * (1 - s)))


def relu_bwd(gy, y):
    g, y = t64(gy), t64(y)
    v = torch.where(y > 0, g, torch.zeros_like(g))
    return v, v.abs()


def leaky_relu_bwd(gy, y, slope):
    g, y = t64(gy), t64(y)
    v = torch.where(y > 0, g, g * float(np.float32(slope)))
    return v, v.abs()


def axpby(a, b=None, alpha=1.0, beta=1.0):
    """alpha * a + beta * b, a smaller b repeated along the leading axes (flat period b.numel())."""
    a = t64(a)
    alpha, beta = float(np.float32(alpha)), float(np.float32(beta))
    v, ab = alpha * a, abs(alpha) * a.abs()
    if b is not None:
        bb = t64(b).reshape(-1).repeat(a.numel() // b.numel()).reshape(a.shape)
        v, ab = v + beta * bb, ab + abs(beta) * bb.abs()
    return v, ab


def film_fwd(z, film):
    """z [n_pix, C], film [n_pix, 2C] = (gamma | beta) -> z * gamma + beta."""
    z, f = t64(z), t64(film)
    C = z.shape[-1]
    return z * f[:, :C] + f[:, C:], z.abs() * f[:, :C].abs() + f[:, C:].abs()


def film_bwd(gy, z, film):
    """-> (gz, gfilm) pairs."""
    g, z, f = t64(gy), t64(z), t64(film)
    C = z.shape[-1]
    gz = g * f[:, :C]
    gf = torch.cat([g * z, g], -1)
    return (gz, gz.abs()), (gf, gf.abs())


def init_conv(x, w, b):
    """x [B,H,W,1], w [C], b [C] -> x * w + b, [B,H,W,C]."""
    x, w, b = t64(x), t64(w).reshape(-1), t64(b).reshape(-1)
    return x * w + b, x.abs() * w.abs() + b.abs()


# --------------------------------------------------------------------------- BiFPN weighted sum
WS_EPS = float(np.float32(1e-4))


def weighted_sum(xs, wraw):
    """(sum_i relu(w_i) x_i) / (sum_i relu(w_i) + 1e-4)."""
    xs, w = [t64(x) for x in xs], t64(wraw).clamp(min=0)
    den = float(w[:len(xs)].sum()) + WS_EPS
    return sum(wi * x for wi, x in zip(w, xs)) / den, sum(wi * x.abs() for wi, x in zip(w, xs)) / den


def weighted_sum_bwd(xs, wraw, g):
    """-> ([gx_i pairs], gw pair): gx_i = g relu(w_i) / den, gw_i = [w_i > 0] sum g (x_i - out) / den."""
    g, raw = t64(g), t64(wraw)
    w = raw.clamp(min=0)
    xs = [t64(x) for x in xs]
    den = float(w[:len(xs)].sum()) + WS_EPS
    out, out_a = weighted_sum(xs, wraw)
    gxs = [(g * (float(wi) / den), g.abs() * (float(wi) / den)) for wi, _ in zip(w, xs)]
    gw = torch.stack([(g * (x - out)).sum() / den if float(r) > 0 else torch.zeros((), dtype=torch.float64) for r, x in zip(raw, xs)])
    gw_a = torch.stack([(g.abs() * (x.abs() + out_a)).sum() / den if float(r) > 0 else torch.zeros((), dtype=torch.float64)
                        for r, x in zip(raw, xs)])
    return gxs, (gw, gw_a)


# --------------------------------------------------------------------------- column reductions, train-mode BatchNorm
def colsum(g, n=None):
    g = t64(g)
    n = g.shape[1] if n is None else n
    return g[:, :n].sum(0), g[:, :n].abs().sum(0)


def bn_train_fwd(x, w, b, eps, momentum, run_mean, run_var):
    """bn_finalize_kernel's semantics written out (torch refuses M = 1): mean, biased variance clamped at 0, invstd = 1 / sqrt(var + eps),
    running statistics with the unbiased variance var * M / (M - 1) (var itself when M == 1) and (1 - momentum) * old + momentum * new.
    -> dict of (value, absref) pairs: y, mean, invstd, run_mean, run_var; plus 'var_cancel' = E[x^2] + mean^2 per channel, the magnitude
    the device's float64 `E[x^2] - mean^2` cancels from."""
    x, w, b = t64(x), t64(w), t64(b)
    M = x.shape[0]
    mom = float(np.float32(momentum))
    eps = float(np.float32(eps))
    mu = x.mean(0)
    var = ((x - mu) ** 2).mean(0)
    invstd = 1.0 / torch.sqrt(var + eps)
    unb = var * M / (M - 1) if M > 1 else var
    rm, rv = t64(run_mean), t64(run_var)
    amu = x.abs().mean(0)
    return {
        'y': ((x - mu) * invstd * w + b, (x.abs() + amu) * invstd * w.abs() + b.abs()),
        'mean': (mu, amu),
        'invstd': (invstd, invstd.clone()),
        'run_mean': ((1 - mom) * rm + mom * mu, (1 - mom) * rm.abs() + mom * amu),
        'run_var': ((1 - mom) * rv + mom * unb, (1 - mom) * rv.abs() + mom * unb),
        'var': (var, var.clone()),
        'var_cancel': (x * x).mean(0) + mu * mu,
    }


def bn_train_bwd(g, x, mean, invstd, w):
    """On the SAVED fp32 mean / invstd (operands like any other): xhat = (x - mean) invstd, gx = w invstd (g - mean(g) - xhat mean(g xhat)),
    gw = sum g xhat, gb = sum g.  -> (gx, gw, gb) pairs."""
    g, x, mean, invstd, w = (t64(t) for t in (g, x, mean, invstd, w))
    xh = (x - mean) * invstd
    xh_a = (x.abs() + mean.abs()) * invstd
    sg, sgx = g.mean(0), (g * xh).mean(0)
    sg_a, sgx_a = g.abs().mean(0), (g.abs() * xh_a).mean(0)
    gx = w * invstd * (g - sg - xh * sgx)
    gx_a = w.abs() * invstd * (g.abs() + sg_a + xh_a * sgx_a)
    return (gx, gx_a), ((g * xh).sum(0), (g.abs() * xh_a).sum(0)), (g.sum(0), g.abs().sum(0))


# --------------------------------------------------------------------------- max pooling 3x3 / stride 2 / pad 1
def maxpool(x):
    """x [B,H,W,C] -> (y [B,Ho,Wo,C], idx [B,Ho,Wo,C] = r * 3 + s of the first maximum of the window in (r, s) scan order: torch's rule)."""
    xc = to_nchw(x)
    B, C, H, W = xc.shape
    y, flat = F.max_pool2d(xc, 3, 2, 1, return_indices=True)
    Ho, Wo = y.shape[2:]
    iy, ix = flat // W, flat % W
    oy = torch.arange(Ho).view(1, 1, Ho, 1)
    ox = torch.arange(Wo).view(1, 1, 1, Wo)
    idx = (iy - (2 * oy - 1)) * 3 + (ix - (2 * ox - 1))
    return to_nhwc(y), to_nhwc(idx).to(torch.uint8)


def maxpool_bwd(x, gy, residual=None, mask=None):
    """(torch float64 autograd of max_pool2d + residual) * (mask > 0)."""
    xc = to_nchw(x).requires_grad_(True)
    F.max_pool2d(xc, 3, 2, 1).backward(to_nchw(gy))
    g = to_nhwc(xc.grad)
    if residual is not None:
        g = g + t64(residual)
    if mask is not None:
        g = torch.where(t64(mask) > 0, g, torch.zeros_like(g))
    return g


# --------------------------------------------------------------------------- depthwise 3x3 / pad 1
def dwconv(x, w, bias, mult, stride):
    """x [B,H,W,Cin], w [Cin*mult,1,3,3], bias [Cin*mult] or None -> [B,Ho,Wo,Cin*mult]."""
    xc, w = to_nchw(x), t64(w)
    b = t64(bias) if bias is not None else None
    v = F.conv2d(xc, w, b, stride=stride, padding=1, groups=xc.shape[1])
    a = F.conv2d(xc.abs(), w.abs(), b.abs() if b is not None else None, stride=stride, padding=1, groups=xc.shape[1])
    return to_nhwc(v), to_nhwc(a)


def dwconv_bwd(x, g, w, mult, stride):
    """-> (gx [B,H,W,Cin], gw [Cin*mult,1,3,3], gb [Cin*mult]) by float64 autograd."""
    xc, w = to_nchw(x).requires_grad_(True), t64(w).requires_grad_(True)
    b = torch.zeros(w.shape[0], dtype=torch.float64, requires_grad=True)
    F.conv2d(xc, w, b, stride=stride, padding=1, groups=xc.shape[1]).backward(to_nchw(g))
    return to_nhwc(xc.grad), w.grad, b.grad


# --------------------------------------------------------------------------- 2x2 average pooling, space to batch
def avgpool2x2_f32(x):
    """fp32, in the order the kernel states as torch's CPU order: (((a + b) + c) + d) * 0.25 over the block row by row."""
    x = x.detach().cpu().float()
    return (((x[:, 0::2, 0::2] + x[:, 0::2, 1::2]) + x[:, 1::2, 0::2]) + x[:, 1::2, 1::2]) * 0.25


def avgpool2x2_bwd_f32(gy):
    g = gy.detach().cpu().float() * 0.25
    return g.repeat_interleave(2, 1).repeat_interleave(2, 2)


def space_to_batch2(x):
    """[B,H,W,C] -> [4B,H/2,W/2,C], class 2a + b major."""
    x = x.detach().cpu()
    return torch.cat([x[:, a::2, b::2] for a in range(2) for b in range(2)], 0).contiguous()


# --------------------------------------------------------------------------- optimiser
def sqnorm(g):
    """Exact sum of squares of the fp32 values (math.fsum of exact float64 squares)."""
    v = t64(g).reshape(-1).numpy()
    return math.fsum((v * v).tolist())


def clip_coef(sqn, max_norm):
    """torch.nn.utils.clip_grad_norm_'s coefficient: min(max_norm / (norm + 1e-6), 1)."""
    return min(float(max_norm) / (math.sqrt(sqn) + 1e-6), 1.0)


def adamw_step(p, g, m, v, lr, beta1, beta2, eps, wd, step, coef=1.0):
    """One torch.optim.AdamW step (decoupled decay, bias corrections) on g * coef -> (p, m, v) pairs."""
    p, g, m, v = (t64(t) for t in (p, g, m, v))
    lr, beta1, beta2, eps, wd = (float(np.float32(t)) for t in (lr, beta1, beta2, eps, wd))
    g = g * coef
    m2 = beta1 * m + (1 - beta1) * g
    v2 = beta2 * v + (1 - beta2) * g * g
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    upd = (lr / bc1) * (m2 / (v2.sqrt() / math.sqrt(bc2) + eps))
    p2 = p * (1 - lr * wd) - upd
    m_a = beta1 * m.abs() + (1 - beta1) * g.abs()
    return (p2, p.abs() * (1 + lr * wd) + upd.abs()), (m2, m_a), (v2, v2.clone())


# --------------------------------------------------------------------------- bounds
def ratio(got, ref, absref, k, extra=0.0):
    """max over the elements of |got - ref| / (k * 2^-24 * absref + extra); an element whose bound is 0 must be exact (its ratio is 0
    when it is, inf when it is not).  NaN anywhere in `got` -> inf."""
    got = t64(got)
    ref, absref = t64(ref), t64(absref)
    assert got.shape == ref.shape == absref.shape, (got.shape, ref.shape, absref.shape)
    if not bool(torch.isfinite(got).all()):
        return float('inf')
    err = (got - ref).abs()
    bound = k * U * absref + extra
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max()) if r.numel() else 0.0
