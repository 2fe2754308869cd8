"""Backbone modules (reference nets/backbone.py), HIP forward.

Same classes / constructor arguments / state_dict keys as the reference: `backbone.0.init_conv.*`,
`backbone.0.body.<torchvision ResNet-50 names>`.  torchvision is not a dependency: the ResNet-50 v1.5
definition (public architecture, reference backbone.py:131 `getattr(torchvision.models, name)`) is
stated here as parameter containers, and the forward is a chain of fp32-MFMA implicit-GEMM launches with
FrozenBatchNorm affine + ReLU + residual fused into the epilogues.  Activations are NHWC.
The ResNeXt names (resnext50_32x4d, resnext101_32x8d, resnext101_64x4d) are the same body with grouped bottlenecks, whose 3x3 runs
on `ops.gconv3x3` (csrc/gconv.hip) and trains through `Fn.GConv3x3` (csrc/gconv_bwd.hip) in training mode.
The EfficientNet names (efficientnet_b0 .. efficientnet_b4; Tan & Le 2019, torchvision's module / state_dict names) are a body of MBConv
blocks: 1x1 GEMMs, the depthwise kernel and the squeeze-and-excitation kernel of csrc/mbconv.hip, frozen and evaluation only.
`--norm_layer_backbone batchnorm` (ResNet / ResNeXt names) puts the live `BatchNorm2d` in place of FrozenBatchNorm2d: the same launches in
eval mode, a chain of convolutions and `Fn.BatchNormAct` nodes (csrc/bnorm.hip) in training mode.
"""
import math

import torch
from torch import nn

from .. import ops
from . import _prep, functional as Fn
from .position_encoding import build_position_encoding

bcbk_channels = {'resnet': {'2': 64, '3': 256, '4': 512, '5': 1024, '6': 2048}}
_RESNET_LAYERS = {'resnet50': [3, 4, 6, 3], 'resnet101': [3, 4, 23, 3], 'resnet152': [3, 8, 36, 3]}
# ResNeXt (Xie et al. 2017; torchvision's names): name -> (layers, groups, base width); the taps keep the ResNet channel counts
_RESNEXT = {'resnext50_32x4d': ([3, 4, 6, 3], 32, 4), 'resnext101_32x8d': ([3, 4, 23, 3], 32, 8),
            'resnext101_64x4d': ([3, 4, 23, 3], 64, 4)}
# EfficientNet-B0 (Tan & Le 2019, table 1): (expand ratio, kernel, stride, in, out, repeats) per stage; name -> (width, depth) multiplier
_EFFNET_BASE = ((1, 3, 1, 32, 16, 1), (6, 3, 2, 16, 24, 2), (6, 5, 2, 24, 40, 2), (6, 3, 2, 40, 80, 3), (6, 5, 1, 80, 112, 3),
                (6, 5, 2, 112, 192, 4), (6, 3, 1, 192, 320, 1))
_EFFICIENTNET = {'efficientnet_b0': (1.0, 1.0), 'efficientnet_b1': (1.0, 1.1), 'efficientnet_b2': (1.1, 1.2),
                 'efficientnet_b3': (1.2, 1.4), 'efficientnet_b4': (1.4, 1.8)}
_EFFNET_TAPS = (1, 2, 3, 5, 7)         # the reference's IntermediateLayerGetter return layers of `features`


def _make_divisible(v, divisor=8):
    """Nearest multiple of `divisor`, never below it, and one step up if rounding lost more than 10 %."""
    new_v = max(divisor, int(v + divisor / 2) // divisor * divisor)
    return new_v + divisor if new_v < 0.9 * v else new_v


def efficientnet_stages(name):
    """[(expand ratio, kernel, stride, in, out, repeats)] of the seven MBConv stages with the width / depth multipliers applied."""
    width, depth = _EFFICIENTNET[name]
    return [(t, k, s, _make_divisible(i * width), _make_divisible(o * width), int(math.ceil(n * depth))) for t, k, s, i, o, n in _EFFNET_BASE]


class FrozenBatchNorm2d(nn.Module):
    """Fixed statistics + affine (reference backbone.py:26-62, eps = 1e-5); never run on its own: its
    (scale, shift) are folded into the producing convolution's epilogue."""

    def __init__(self, n):
        super().__init__()
        self.register_buffer('weight', torch.ones(n))
        self.register_buffer('bias', torch.zeros(n))
        self.register_buffer('running_mean', torch.zeros(n))
        self.register_buffer('running_var', torch.ones(n))

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        state_dict.pop(prefix + 'num_batches_tracked', None)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                                      error_msgs)

    def affine(self):
        return _prep.bn_affine(self.weight, self.bias, self.running_mean, self.running_var, 1e-5, frozen=True)


class BatchNorm2d(nn.BatchNorm2d):
    """Live BatchNorm (reference backbone.py:125-126, `--norm_layer_backbone batchnorm`): torch's module and state_dict (weight, bias,
    running_mean, running_var, num_batches_tracked), never run through torch.  In eval mode its running statistics fold into the
    producing convolution's epilogue like FrozenBatchNorm2d's (`affine`); in training mode `act` normalises with the batch statistics
    and updates the running ones (`Fn.BatchNormAct`, csrc/bnorm.hip) -- whatever `requires_grad` says and also under no_grad, as
    nn.BatchNorm2d does."""

    def __init__(self, n):
        super().__init__(n)                 # affine = True, track_running_stats = True, eps = 1e-5, momentum = 0.1
        del self.__dict__['affine']         # torch's flag (always True here) would hide the method every norm layer of the body has

    def extra_repr(self):
        return f'{self.num_features}, eps={self.eps}, momentum={self.momentum}'

    def affine(self):
        return _prep.bn_affine(self.weight, self.bias, self.running_mean, self.running_var, self.eps, frozen=False)

    def act(self, z, residual=None, relu=False):
        """Training mode: act(BatchNorm(z) (+ residual)) on the batch statistics; one more batch tracked."""
        self.num_batches_tracked += 1
        return Fn.BatchNormAct.apply(z, self.weight, self.bias, self.running_mean, self.running_var, self.eps, self.momentum, residual,
                                     relu)


def _live(norm):
    return isinstance(norm, BatchNorm2d)


def _grad_asked(mod, x):
    return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in mod.parameters()))


def _refuse_eval_grad(what):
    raise NotImplementedError(f'{what} with live BatchNorm in eval mode has no backward pass (the fused eval kernels have no gradient for '
                              'the weight and bias of the norm): call .train() on the model to train through it, or run it under '
                              'torch.no_grad()')


class _Bottleneck(nn.Module):
    """ResNet v1.5 bottleneck (stride on the 3x3).  With live BatchNorm in training mode the block is a chain of tape nodes: the three
    convolutions without epilogue (`Fn.conv`), each followed by `Fn.BatchNormAct` (the last one with the shortcut and the ReLU)."""

    def __init__(self, inplanes, planes, stride, downsample, norm_layer):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = norm_layer(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = norm_layer(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = norm_layer(planes * 4)
        self.downsample = downsample
        self.stride = stride
        # set by _ResNetBody: is the input a ReLU output / does the output feed anything besides the next block
        self.mask_input, self.mask_gy = False, True

    def forward_live(self, x):
        o = self.bn1.act(Fn.conv(x, self.conv1.weight), relu=True)
        o = self.bn2.act(Fn.conv(o, self.conv2.weight, kh=3, kw=3, stride=self.stride, pad=1), relu=True)
        return _live_tail(self, x, o)

    def forward(self, x):
        if _live(self.bn1):
            if self.training:
                return self.forward_live(x)
            if _grad_asked(self, x):
                _refuse_eval_grad('a ResNet block')
        if torch.is_grad_enabled() and x.dim() == 4 and self.conv1.weight.shape[0] % 32 == 0:
            ds = self.downsample
            sd, bd = ds[1].affine() if ds is not None else (None, None)
            return Fn.Bottleneck.apply(x, self.conv1.weight, self.conv2.weight, self.conv3.weight,
                                       ds[0].weight if ds is not None else None, *self.bn1.affine(), *self.bn2.affine(),
                                       *self.bn3.affine(), sd, bd, self.stride, self.mask_input, self.mask_gy)
        s, b = self.bn1.affine()
        o = Fn.conv(x, self.conv1.weight, scale=s, shift=b, act=ops.ACT_RELU)
        s, b = self.bn2.affine()
        if self.stride == 1 and Fn._winograd_ok(o, self.conv2.weight, 3, 3, 1, 1):
            # >= 128 channels: Winograd F(2x2,3x3) with FrozenBN + ReLU in the output transform (same as Fn.Bottleneck)
            o = ops.conv3x3_winograd(o, _prep.wino23(self.conv2.weight), b, scale=s, relu=True)
        else:
            o = Fn.conv(o, self.conv2.weight, scale=s, shift=b, kh=3, kw=3, stride=self.stride, pad=1, act=ops.ACT_RELU)
        if self.downsample is not None:
            s, b = self.downsample[1].affine()
            idt = Fn.conv(x, self.downsample[0].weight, scale=s, shift=b, stride=self.stride)
        else:
            idt = x
        s, b = self.bn3.affine()
        return Fn.conv(o, self.conv3.weight, scale=s, shift=b, residual=idt, act=ops.ACT_RELU)


def _live_tail(blk, x, o):
    """conv3 -> bn3 (+ shortcut, ReLU) of a live-BatchNorm block; the projection shortcut is a convolution and a norm without ReLU."""
    if blk.downsample is not None:
        idt = blk.downsample[1].act(Fn.conv(x, blk.downsample[0].weight, stride=blk.stride))
    else:
        idt = x
    return blk.bn3.act(Fn.conv(o, blk.conv3.weight), residual=idt, relu=True)


class _GroupedBottleneck(nn.Module):
    """ResNeXt bottleneck (torchvision's `Bottleneck` with groups > 1; same module / state_dict names): 1x1 to `width` =
    int(planes * base_width / 64) * groups channels, GROUPED 3x3 (stride on it) through `ops.gconv3x3` with bn2 + ReLU in its epilogue,
    1x1 to 4 * planes with the shortcut in its epilogue.  In training mode with a gradient asked for the grouped convolution is the
    tape node `Fn.GConv3x3` (same forward launch; backward: `ops.gconv3x3_dgrad` / `ops.gconv3x3_wgrad`) between the `Fn.conv` nodes of
    the 1x1 convolutions; a gradient asked of a block in eval mode is refused."""

    def __init__(self, inplanes, planes, stride, downsample, norm_layer, groups, base_width):
        super().__init__()
        width = int(planes * base_width / 64) * groups
        self.conv1 = nn.Conv2d(inplanes, width, 1, bias=False)
        self.bn1 = norm_layer(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride=stride, padding=1, groups=groups, bias=False)
        self.bn2 = norm_layer(width)
        self.conv3 = nn.Conv2d(width, planes * 4, 1, bias=False)
        self.bn3 = norm_layer(planes * 4)
        self.downsample = downsample
        self.stride, self.groups = stride, groups
        self.mask_input, self.mask_gy = False, True           # (set by _ResNetBody; only Fn.Bottleneck reads them)

    def forward(self, x):
        grad = _grad_asked(self, x)
        if _live(self.bn1):
            if self.training:         # the bare grouped convolution (no affine, no ReLU, no mask) between the norms
                o = self.bn1.act(Fn.conv(x, self.conv1.weight), relu=True)
                o = self.bn2.act(Fn.GConv3x3.apply(o, self.conv2.weight, None, None, self.groups, self.stride, False), relu=True)
                return _live_tail(self, x, o)
            if grad:
                _refuse_eval_grad('a ResNeXt block')
        if grad and not self.training:
            raise NotImplementedError('a ResNeXt block in eval mode has no backward pass: call .train() on the model to train through it '
                                      '(FrozenBN makes the two modes compute the same), or train with --lr_backbone 0 (a frozen '
                                      'backbone), or run it under torch.no_grad()')
        s, b = self.bn1.affine()
        o = Fn.conv(x, self.conv1.weight, scale=s, shift=b, act=ops.ACT_RELU)
        s, b = self.bn2.affine()
        if grad:          # the training chain: the same launch as a tape node (Fn.conv is a tape node already)
            o = Fn.GConv3x3.apply(o, self.conv2.weight, s, b, self.groups, self.stride)
        else:
            o = ops.gconv3x3(o, _prep.gconv(self.conv2.weight, self.groups), self.groups, stride=self.stride, scale=s, shift=b, relu=True)
        if self.downsample is not None:
            s, b = self.downsample[1].affine()
            idt = Fn.conv(x, self.downsample[0].weight, scale=s, shift=b, stride=self.stride)
        else:
            idt = x
        s, b = self.bn3.affine()
        return Fn.conv(o, self.conv3.weight, scale=s, shift=b, residual=idt, act=ops.ACT_RELU)


class _ResNetBody(nn.Module):
    """conv1/bn1/relu/maxpool/layer1..4 with torchvision's names; returns the 5 taps the reference takes
    with IntermediateLayerGetter (backbone.py:82-85): relu, layer1..layer4."""

    def __init__(self, layers, norm_layer, dilation=False, groups=1, base_width=64):
        """`groups` > 1: ResNeXt blocks (`_GroupedBottleneck`) of `base_width` channels per group at layer1.
        `dilation` (reference backbone.py:129-131: torchvision's `replace_stride_with_dilation=[False, False, True]`): layer4 keeps
        layer3's resolution -- its first block runs with stride 1 (3x3 dilation 1, like torchvision: the first block uses the
        PREVIOUS dilation), the following blocks with 3x3 / dilation 2 / padding 2.  Same parameters, same state_dict."""
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = norm_layer(64)
        self.dilation = bool(dilation)
        inplanes = 64
        for li, (planes, n, stride) in enumerate(zip((64, 128, 256, 512), layers, (1, 2, 2, 1 if dilation else 2)), start=1):
            blocks = []
            for bi in range(n):
                st = stride if bi == 0 else 1
                ds = None
                if bi == 0 and (st != 1 or inplanes != planes * 4):
                    ds = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride=st, bias=False), norm_layer(planes * 4))
                blocks.append(_Bottleneck(inplanes, planes, st, ds, norm_layer) if groups == 1 else
                              _GroupedBottleneck(inplanes, planes, st, ds, norm_layer, groups, base_width))
                if dilation and li == 4 and bi > 0:                   # state_dict / repr parity with torchvision's module
                    blocks[-1].conv2.dilation, blocks[-1].conv2.padding = (2, 2), (2, 2)
                blocks[-1].mask_input = not (li == 1 and bi == 0)      # layer1.0 reads the max-pool output
                blocks[-1].mask_gy = bi == n - 1                       # the layer output is a tap (several consumers)
                inplanes = planes * 4
            setattr(self, f'layer{li}', nn.Sequential(*blocks))

    def forward(self, x, init_conv=None):
        """x: NHWC image; with `init_conv` (1 -> 3 channels) the stem is ONE differentiable op (Fn.Stem)."""
        if _live(self.bn1) and self.training:
            # live BatchNorm: the bare stem (Fn.StemRaw: the stem kernel has the ReLU built in), then the norm + ReLU
            z = Fn.StemRaw.apply(x, init_conv.weight, init_conv.bias, self.conv1.weight) if init_conv is not None else \
                Fn.conv(x, self.conv1.weight, kh=7, kw=7, stride=2, pad=3)
            x = self.bn1.act(z, relu=True)
        else:
            if _live(self.bn1) and torch.is_grad_enabled() and (x.requires_grad or self.conv1.weight.requires_grad or
                                                                self.bn1.weight.requires_grad):
                _refuse_eval_grad('the stem')
            s, b = self.bn1.affine()
            if init_conv is not None:
                x = Fn.Stem.apply(x, init_conv.weight, init_conv.bias, self.conv1.weight, s, b)
            else:
                x = Fn.conv(x, self.conv1.weight, scale=s, shift=b, kh=7, kw=7, stride=2, pad=3, act=ops.ACT_RELU)
        taps = [x]
        x = Fn.MaxPool.apply(x, True)              # the stem output is a ReLU output
        for li in range(1, 5):
            for bi, blk in enumerate(getattr(self, f'layer{li}')):
                if self.dilation and li == 4 and bi == 1:
                    # the dilated blocks: a 3x3 / dilation-2 / pad-2 convolution is the ordinary 3x3 on the four parity classes of the
                    # pixels, and the rest of a bottleneck is point-wise -> run the ordinary blocks on the space-to-batch form
                    x = Fn.SpaceToBatch2.apply(x, False)
                x = blk(x)
            if self.dilation and li == 4 and len(self.layer4) > 1:
                x = Fn.SpaceToBatch2.apply(x, True)
            taps.append(x)
        return taps


class _SqueezeExcitation(nn.Module):
    """Parameter holder of torchvision's SqueezeExcitation: fc1 (C -> Csq) and fc2 (Csq -> C), 1x1 convolutions with bias."""

    def __init__(self, channels, squeeze):
        super().__init__()
        self.fc1 = nn.Conv2d(channels, squeeze, 1)
        self.fc2 = nn.Conv2d(squeeze, channels, 1)


def _conv_norm(cin, cout, k, stride, groups, norm_layer):
    return nn.Sequential(nn.Conv2d(cin, cout, k, stride=stride, padding=(k - 1) // 2, groups=groups, bias=False), norm_layer(cout))


class _MBConv(nn.Module):
    """One MBConv block, torchvision's names (`block.{i}`: [expand,] depthwise, SE, project).  Forward (no tape: the body is frozen):
    expand 1x1 GEMM with norm + SiLU in the epilogue -> `ops.dwconv_bn_act` (norm + SiLU, and the pool partials) -> `ops.se_gate` (the gate,
    folded into one copy of the project weights per image) -> the project 1x1 as a GEMM with groups = B, norm and the block input in its
    epilogue.  The gated map is never written."""

    def __init__(self, ratio, k, stride, cin, cout, norm_layer):
        super().__init__()
        cexp = _make_divisible(cin * ratio)
        layers = [] if cexp == cin else [_conv_norm(cin, cexp, 1, 1, 1, norm_layer)]
        layers += [_conv_norm(cexp, cexp, k, stride, cexp, norm_layer), _SqueezeExcitation(cexp, max(1, cin // 4)),
                   _conv_norm(cexp, cout, 1, 1, 1, norm_layer)]
        self.block = nn.Sequential(*layers)
        self.k, self.stride, self.use_res = k, stride, stride == 1 and cin == cout

    def forward(self, x):
        *expand, dw, se, proj = self.block
        o = x
        for e in expand:
            s, b = e[1].affine()
            o = ops.conv2d(o, _prep.krsc(e[0].weight), scale=s, shift=b, act=ops.ACT_SILU)
        s, b = dw[1].affine()
        o, part = ops.dwconv_bn_act(o, _prep.dw_taps(dw[0].weight), self.k, self.stride, scale=s, shift=b, act=ops.ACT_SILU, pool=True)
        _, wb = ops.se_gate(part, o.shape[1] * o.shape[2], se.fc1.weight.detach(), se.fc1.bias.detach(), se.fc2.weight.detach(),
                            se.fc2.bias.detach(), wproj=_prep.krsc(proj[0].weight))
        s, b = proj[1].affine()
        return ops.conv1x1_per_image(o, wb, proj[0].weight.shape[0], scale=s, shift=b, residual=x if self.use_res else None)


class _EfficientNetBody(nn.Sequential):
    """torchvision's `efficientnet_bN().features` up to stage 7 under the reference's IntermediateLayerGetter (children '0' .. '7': the
    stem and the seven MBConv stages; the 1x1 head convolution, index 8, and the classifier are not part of the detector); returns the
    outputs of stages 1, 2, 3, 5, 7."""

    def __init__(self, name, norm_layer):
        stages = efficientnet_stages(name)
        mods = [_conv_norm(3, stages[0][3], 3, 2, 1, norm_layer)]
        for t, k, s, cin, cout, n in stages:
            mods.append(nn.Sequential(*[_MBConv(t, k, s if i == 0 else 1, cin if i == 0 else cout, cout, norm_layer) for i in range(n)]))
        super().__init__(*mods)
        self.num_channels = [stages[i - 1][4] for i in _EFFNET_TAPS]

    def stem(self, x, init_conv=None):
        """x: NHWC image -> the stage-0 output.  The stem's zero padding surrounds the OUTPUT of init_conv (1 -> 3 channels, with a bias):
        the bias is inside the image and not in the padding, so the two are not composed into one convolution -- `ops.init_conv` writes
        the 3-channel image (three times the input, the smallest map of the network) and the stem reads it with its own padding."""
        if init_conv is not None:
            x = ops.init_conv(x, init_conv.weight.detach(), init_conv.bias.detach())
        s, b = self[0][1].affine()
        return ops.conv2d(x, _prep.krsc(self[0][0].weight), 3, 3, 2, 1, scale=s, shift=b, act=ops.ACT_SILU)

    def forward(self, x, init_conv=None):
        x = self.stem(x, init_conv)
        taps = []
        for i in range(1, 8):
            for blk in self[i]:
                x = blk(x)
            if i in _EFFNET_TAPS:
                taps.append(x)
        return taps


class BackboneBase(nn.Module):

    def __init__(self, backbone, name, in_channels, train_backbone):
        super().__init__()
        for _, parameter in backbone.named_parameters():
            if not train_backbone:
                parameter.requires_grad_(False)
        self.body = backbone
        self.num_channels = list(getattr(backbone, 'num_channels', bcbk_channels['resnet'].values()))
        if in_channels != 3:
            self.init_conv = nn.Conv2d(in_channels, 3, 1)
        self.in_channels = in_channels
        self.strides = [2 ** (i + 1) for i in range(len(self.num_channels))]

    def forward(self, x):
        """x: NHWC [B,H,W,in_channels] -> list of 5 NHWC maps (reference backbone.py:110-113)."""
        if hasattr(self, 'init_conv'):
            if self.in_channels != 1:
                raise NotImplementedError('init_conv is implemented for 1 input channel (reference default)')
            return self.body(x, self.init_conv)
        return self.body(x)


class Backbone(BackboneBase):
    """ResNet / ResNeXt / EfficientNet backbone (reference backbone.py:116-132); `norm_layer_name`: frozen_batchnorm, or batchnorm
    (live `BatchNorm2d`) for the ResNet and ResNeXt names."""

    def __init__(self, name, in_channels, train_backbone, dilation, norm_layer_name):
        if name not in _RESNET_LAYERS and name not in _RESNEXT and name not in _EFFICIENTNET:
            raise ValueError(f'not supported {name}: the accelerated path implements '
                             f'{sorted(_RESNET_LAYERS) + sorted(_RESNEXT) + sorted(_EFFICIENTNET)} (efficientnet_v2_* and vgg16_bn are not)')
        if norm_layer_name not in ('frozen_batchnorm', 'batchnorm') or (name in _EFFICIENTNET and norm_layer_name != 'frozen_batchnorm'):
            raise NotImplementedError('only --norm_layer_backbone frozen_batchnorm (reference default) is implemented' if name in _EFFICIENTNET
                                      else f'--norm_layer_backbone {norm_layer_name}: frozen_batchnorm (reference default) and batchnorm are '
                                      'implemented')
        if name in _EFFICIENTNET:
            if train_backbone:
                raise NotImplementedError(f'fine-tuning the {name} body is not implemented (the depthwise and squeeze-and-excitation kernels '
                                          'have no backward pass yet): train behind the frozen body with --lr_backbone 0')
            if in_channels != 1:
                raise NotImplementedError(f'{name}: only --inpt_channels 1 (reference default) is implemented')
            # `dilation` has no effect: the reference passes replace_stride_with_dilation to the resn* names only (backbone.py:129-131)
            super().__init__(_EfficientNetBody(name, FrozenBatchNorm2d), name, in_channels, False)
            # the frozen body runs without a tape, so no gradient reaches init_conv; its learning rate is --lr_backbone = 0 anyway
            self.init_conv.requires_grad_(False)
            return
        layers, groups, base_width = _RESNEXT[name] if name in _RESNEXT else (_RESNET_LAYERS[name], 1, 64)
        norm_layer = BatchNorm2d if norm_layer_name == 'batchnorm' else FrozenBatchNorm2d
        super().__init__(_ResNetBody(layers, norm_layer, dilation=dilation, groups=groups, base_width=base_width), name,
                         in_channels, train_backbone)
        if groups > 1 and not train_backbone and hasattr(self, 'init_conv'):
            # a frozen ResNeXt body asks for no gradient, so none reaches init_conv; its learning rate is --lr_backbone = 0 anyway
            self.init_conv.requires_grad_(False)


class Joiner(nn.Sequential):
    def __init__(self, backbone, position_embedding):
        super().__init__(backbone, position_embedding)

    def forward(self, x):
        """-> (list of 5 NHWC feature maps, None).  The per-level sine encodings of the reference
        (backbone.py:139-148) are unused by the default config and not evaluated."""
        return self[0](x), None


def build_backbone(args, inference=False):
    """`inference` (run_detection.load_model): the model will only be evaluated -- an EfficientNet checkpoint whose training arguments
    hold an lr_backbone > 0 loads with its body frozen instead of being refused."""
    position_embedding = build_position_encoding(args)
    train_backbone = args.lr_backbone > 0 and not (inference and args.backbone in _EFFICIENTNET)
    backbone = Backbone(args.backbone, args.inpt_channels, train_backbone, args.dilation, args.norm_layer_backbone)
    model = Joiner(backbone, position_embedding)
    model.num_channels = backbone.num_channels
    model.strides = backbone.strides
    setattr(args, 'n_layers', len(backbone.num_channels))
    return model
