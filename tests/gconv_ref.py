"""Float64 references of the ResNeXt additions, plain torch only (nothing here calls the HIP library):

`gconv`       the grouped 3x3 convolution `nbm_gconv3x3` implements, on top of conv_ref.conv -- whose leading dimensions ARE groups;
`resnet_taps` the ResNet / ResNeXt body written from the published architecture (He et al. 2016 v1.5, Xie et al. 2017: stem 7x7 / 2,
              max-pool 3x3 / 2, bottlenecks with the stride on the (grouped) 3x3, frozen BatchNorm with eps 1e-5, optional dilated
              layer4), returning the five taps the detector reads.  groups = 1 is ResNet: the same code measures the parent's kernels."""
import torch
import torch.nn.functional as F

import conv_ref


def gconv(x, w, groups, *, stride=1, scale=None, shift=None, relu=False):
    """x [B,H,W,C] NHWC, w [C,Cg,3,3] (checkpoint layout), scale / shift [C] -> float64 [B,Ho,Wo,C]; pad 1."""
    B, H, W, C = x.shape
    Cg = C // groups
    assert w.shape == (C, Cg, 3, 3)
    xg = x.reshape(B, H, W, groups, Cg).permute(3, 0, 1, 2, 4)                                  # [G,B,H,W,Cg]
    wg = w.reshape(groups, Cg, Cg, 3, 3).permute(0, 1, 3, 4, 2).reshape(groups, Cg, 9 * Cg)     # KRSC rows per group
    per_group = lambda v: None if v is None else v.reshape(groups, 1, 1, 1, Cg)
    y = conv_ref.conv(xg, wg, kh=3, kw=3, stride=stride, pad=1, scale=per_group(scale), shift=per_group(shift), relu=relu)
    return y.permute(1, 2, 3, 0, 4).reshape(B, y.shape[2], y.shape[3], C)


def gconv_abs(x, w, groups, *, stride=1, scale=None, shift=None, relu=False):
    """The same convolution on the absolute values of every operand: the scale of the rounding-error bound."""
    a = lambda v: None if v is None else v.abs()
    return gconv(x.abs(), w.abs(), groups, stride=stride, scale=a(scale), shift=a(shift), relu=relu)


def _bn(x, sd, p):
    s = sd[p + '.weight'].double() / torch.sqrt(sd[p + '.running_var'].double() + 1e-5)
    return x * s.view(1, -1, 1, 1) + (sd[p + '.bias'].double() - sd[p + '.running_mean'].double() * s).view(1, -1, 1, 1)


def bottleneck(x, sd, p, stride, groups, dilation=1):
    """One bottleneck, NCHW float64; `p` = key prefix ('body.layer1.0')."""
    c = lambda name: sd[f'{p}.{name}.weight'].double()
    o = F.relu(_bn(F.conv2d(x, c('conv1')), sd, p + '.bn1'))
    o = F.relu(_bn(F.conv2d(o, c('conv2'), stride=stride, padding=dilation, dilation=dilation, groups=groups), sd, p + '.bn2'))
    o = _bn(F.conv2d(o, c('conv3')), sd, p + '.bn3')
    if f'{p}.downsample.0.weight' in sd:
        x = _bn(F.conv2d(x, c('downsample.0'), stride=stride), sd, p + '.downsample.1')
    return F.relu(o + x)


def resnet_taps(sd, img, layers, groups=1, dilation=False):
    """sd: the `backbone.0.` part of a model state_dict (keys 'init_conv.*', 'body.*'); img [B,1,H,W] -> five NCHW float64 taps
    (stem ReLU, layer1 .. layer4)."""
    x = F.conv2d(img.double(), sd['init_conv.weight'].double(), sd['init_conv.bias'].double())
    x = F.relu(_bn(F.conv2d(x, sd['body.conv1.weight'].double(), stride=2, padding=3), sd, 'body.bn1'))
    taps = [x]
    x = F.max_pool2d(x, 3, 2, 1)
    for li, n in enumerate(layers, start=1):
        for bi in range(n):
            stride = 2 if (bi == 0 and li > 1 and not (dilation and li == 4)) else 1
            x = bottleneck(x, sd, f'body.layer{li}.{bi}', stride, groups, dilation=2 if (dilation and li == 4 and bi > 0) else 1)
        taps.append(x)
    return taps
