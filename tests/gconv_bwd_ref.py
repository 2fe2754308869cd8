"""Float64 references of the ResNeXt training path, plain torch only (nothing here calls the HIP library): torch.autograd through
the float64 restatements of tests/gconv_ref.py, on the CPU.

`gconv_grads`  both gradients of y = relu(scale * gconv(x, W) + shift) for a cotangent g: autograd through F.conv2d(groups=...) with
               dz = scale * g * (y > 0) as the cotangent of the convolution (what nbm_gconv3x3_dgrad / _wgrad compute);
`block_grads`  d/dx and every weight gradient of a chain of bottlenecks (gconv_ref.bottleneck);
`body_grads`   every parameter gradient of the body (gconv_ref.resnet_taps) for one cotangent per tap."""
import torch
import torch.nn.functional as F

import gconv_ref


def gconv_grads(x, w, groups, g, stride=1, scale=None, y_mask=None):
    """x [B,H,W,C] NHWC, w [C,Cg,3,3], g [B,Ho,Wo,C], scale [C] or None, y_mask [B,Ho,Wo,C] or None (counts where > 0)
    -> (gx [B,H,W,C], gw [C,Cg,3,3]), float64 on the CPU."""
    xd = x.detach().double().cpu().permute(0, 3, 1, 2).requires_grad_(True)
    wd = w.detach().double().cpu().requires_grad_(True)
    dz = g.detach().double().cpu()
    if scale is not None:
        dz = dz * scale.detach().double().cpu()
    if y_mask is not None:
        dz = dz * (y_mask.detach().cpu() > 0).double()
    z = F.conv2d(xd, wd, stride=stride, padding=1, groups=groups)
    gx, gw = torch.autograd.grad(z, (xd, wd), dz.permute(0, 3, 1, 2))
    return gx.permute(0, 2, 3, 1).contiguous(), gw


def gconv_grads_abs(x, w, groups, g, stride=1, scale=None, y_mask=None):
    """The same gradients of the absolute values of every operand (the mask keeps its sign: it selects): the scale of the
    rounding-error bound."""
    return gconv_grads(x.abs(), w.abs(), groups, g.abs(), stride, None if scale is None else scale.abs(), y_mask)


def _leaves(sd):
    """float64 leaves: conv weights (and init_conv's bias) ask for a gradient, FrozenBN buffers do not."""
    out = {}
    for k, v in sd.items():
        t = v.detach().double().cpu().clone()
        is_bn = any(k.endswith(s) for s in ('running_mean', 'running_var', 'num_batches_tracked')) or '.bn' in k or 'downsample.1.' in k
        out[k] = t.requires_grad_(not is_bn)
    return out


def block_grads(x, sd, blocks, groups, cotangent):
    """x [B,C,H,W] NCHW, blocks = [(key prefix, stride), ...] run one after the other, cotangent of the last output (NCHW)
    -> (output, d/dx, {key: gradient} of every conv weight), float64."""
    ld = _leaves(sd)
    xd = x.detach().double().cpu().requires_grad_(True)
    r = xd
    for p, s in blocks:
        r = gconv_ref.bottleneck(r, ld, p, s, groups)
    keys = [k for k, v in ld.items() if v.requires_grad]
    grads = torch.autograd.grad(r, [xd] + [ld[k] for k in keys], cotangent.detach().double().cpu())
    return r.detach(), grads[0], dict(zip(keys, grads[1:]))


def body_grads(sd, img, layers, cotangents, groups=1, dilation=False):
    """sd: the `backbone.0.` part of a state_dict; cotangents: five NCHW tensors, one per tap; loss = sum <tap_i, cotangent_i>
    -> (taps, {key: gradient} of every parameter), float64."""
    ld = _leaves(sd)
    taps = gconv_ref.resnet_taps(ld, img, layers, groups=groups, dilation=dilation)
    keys = [k for k, v in ld.items() if v.requires_grad]
    loss = sum((t * c.detach().double().cpu()).sum() for t, c in zip(taps, cotangents))
    grads = torch.autograd.grad(loss, [ld[k] for k in keys])
    return [t.detach() for t in taps], dict(zip(keys, grads))
