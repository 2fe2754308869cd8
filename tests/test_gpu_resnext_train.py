"""GPU: training through the ResNeXt backbones -- the grouped blocks in `.train()` mode (`Fn.GConv3x3` between `Fn.conv` nodes), the
whole body, and one optimisation step of the public route with `--lr_backbone` > 0.  The reference is float64 autograd through the
restatement of the published architecture (tests/gconv_ref.py, tests/gconv_bwd_ref.py); the yardstick for the error is what the
ResNet kernels -- code this feature does not touch -- reach under the SAME harness (groups = 1).  Errors are relative L2 norms per
tensor, e = ||got - ref|| / ||ref||, so that a single ReLU sign disagreement between fp32 and float64 cannot decide a test."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gconv_bwd_ref                                                          # noqa: E402
from birdsoundclassif_amd import synth                                        # noqa: E402
from birdsoundclassif_amd.nets import backbone as BB, functional as Fn        # noqa: E402
from helpers import filler_state_dict                                         # noqa: E402

RX = 'resnext50_32x4d'
PREFIX = 'backbone.0.'
MARGIN = 4.0      # the margin of tests/test_gpu_resnext.py: another weight draw and 1x1 convolutions with up to twice the K (sqrt 2 on the
#                   rms error); an indexing or group-mapping error is of order 1, a bf16-level loss about 2^-9


def _rel(got, ref):
    return float((got.double().cpu() - ref).norm() / ref.norm())


def _normal(tag, shape):
    return torch.from_numpy(synth.normal(tag, int(np.prod(shape))).astype(np.float32)).reshape(shape)


# ------------------------------------------------------------------------------------------------------ blocks
def _block_sd(mod, prefix):
    sd = synth.fill_state_dict({prefix + k: tuple(v.shape) for k, v in mod.state_dict().items()})
    mod.load_state_dict({k[len(prefix):]: v for k, v in sd.items()})
    return sd


def _ds(i, o, s):
    return torch.nn.Sequential(torch.nn.Conv2d(i, o, 1, stride=s, bias=False), BB.FrozenBatchNorm2d(o))


def _block_errors(blocks, specs, groups, x, tag):
    """blocks: modules run one after the other on x (NCHW, CPU); specs: [(key prefix, stride)] -> {tensor name: e}."""
    sd = {}
    for b, (p, _) in zip(blocks, specs):
        sd.update(_block_sd(b, p + '.'))
    g = x.permute(0, 2, 3, 1).contiguous().cuda().requires_grad_(True)
    Fn.stash_reset()                                   # a new forward pass, as NbmModel starts one
    o = g
    for b in blocks:
        o = b.cuda().train()(o)
    cot = _normal(tag + '-cot', tuple(o.permute(0, 3, 1, 2).shape))
    o.backward(cot.permute(0, 2, 3, 1).contiguous().cuda())
    ref_out, ref_gx, ref_gw = gconv_bwd_ref.block_grads(x, sd, specs, groups, cot)
    assert 0.05 < float((o != 0).float().mean())
    errs = {'out': _rel(o.detach().permute(0, 3, 1, 2), ref_out), 'd/dx': _rel(g.grad.permute(0, 3, 1, 2), ref_gx)}
    params = {p + '.' + k: v for b, (p, _) in zip(blocks, specs) for k, v in b.named_parameters()}
    assert sorted(params) == sorted(ref_gw), (sorted(params), sorted(ref_gw))
    for k, v in params.items():
        assert v.grad is not None and tuple(v.grad.shape) == tuple(ref_gw[k].shape), k
        errs[k] = _rel(v.grad, ref_gw[k])
    return errs


def _pair(groups, base_width):
    """layer1.0 -> layer2.0 on the 2 x 13 x 21 map of the forward block-pair test."""
    N = BB.FrozenBatchNorm2d
    mk = (lambda i, p, s: BB._GroupedBottleneck(i, p, s, _ds(i, 4 * p, s), N, groups, base_width)) if groups > 1 else \
        (lambda i, p, s: BB._Bottleneck(i, p, s, _ds(i, 4 * p, s), N))
    x = _normal('resnext-block-x', (2, 64, 13, 21)).clamp_min(0)
    return _block_errors([mk(64, 64, 1), mk(256, 128, 2)], [('body.layer1.0', 1), ('body.layer2.0', 2)], groups, x, 'pair')


_YARD = {}


def _resnet_pair():
    if 'pair' not in _YARD:
        _YARD['pair'] = _pair(1, 64)
    return _YARD['pair']


@pytest.mark.parametrize('groups,base_width', [(32, 4), (64, 4)])
def test_block_pair_gradients_against_float64_autograd(groups, base_width):
    e_rx, e_rn = _pair(groups, base_width), _resnet_pair()
    assert sorted(e_rx) == sorted(e_rn)
    for k in e_rx:
        print(f'{groups}x{base_width}d block pair {k}: e_resnext = {e_rx[k]:.3e}  e_resnet = {e_rn[k]:.3e}')
    for k in e_rx:
        assert e_rx[k] <= MARGIN * e_rn[k], (k, e_rx[k], e_rn[k])


def test_block_with_64_channels_per_group_at_stride_2():
    """`_GroupedBottleneck(1024, 512, 2, ds, ..., 32, 8)`: conv2 has 1024 channels in 32 groups of 64, stride 2 (resnext101_32x8d
    layer4.0) on a 2 x 5 x 7 map; the yardstick is the ResNet block of the same position (1024 -> 512 -> 2048, stride 2)."""
    N = BB.FrozenBatchNorm2d
    x = _normal('resnext-cg64-x', (2, 1024, 5, 7)).clamp_min(0)
    spec = [('body.layer4.0', 2)]
    e_rx = _block_errors([BB._GroupedBottleneck(1024, 512, 2, _ds(1024, 2048, 2), N, 32, 8)], spec, 32, x, 'cg64')
    e_rn = _block_errors([BB._Bottleneck(1024, 512, 2, _ds(1024, 2048, 2), N)], spec, 1, x, 'cg64')
    for k in e_rx:
        print(f'32x8d layer4.0 {k}: e_resnext = {e_rx[k]:.3e}  e_resnet = {e_rn[k]:.3e}')
    for k in e_rx:
        assert e_rx[k] <= MARGIN * e_rn[k], (k, e_rx[k], e_rn[k])


def test_a_frozen_grouped_weight_inside_a_trainable_chain_gets_no_gradient():
    N = BB.FrozenBatchNorm2d
    blk = BB._GroupedBottleneck(64, 64, 1, _ds(64, 256, 1), N, 32, 4)
    _block_sd(blk, 'b.')
    blk = blk.cuda().train()
    blk.conv2.weight.requires_grad_(False)
    x = _normal('resnext-frozen-x', (1, 6, 9, 64)).cuda().requires_grad_(True)
    Fn.stash_reset()
    blk(x).sum().backward()
    assert blk.conv2.weight.grad is None and blk.conv1.weight.grad is not None and x.grad is not None
    # eval mode keeps refusing, and says what to do
    with pytest.raises(NotImplementedError, match=r'\.train\(\)'):
        blk.eval()(x)
    with pytest.raises(NotImplementedError, match='--lr_backbone 0'):
        blk.eval()(x)


# ------------------------------------------------------------------------------------------------------ whole body
def _image(B=2, H=64, W=96):
    return torch.from_numpy(synth.uniform(('resnext-img', B, H, W), B * H * W).astype(np.float32)).reshape(B, 1, H, W)


_SD = {}


def _backbone_sd(name):
    if name not in _SD:
        _SD[name] = {k[len(PREFIX):]: v for k, v in filler_state_dict(backbone=name).items() if k.startswith(PREFIX)}
    return _SD[name]


def _stage(key):
    return key.split('.')[1] if key.startswith('body.layer') else 'stem'


def _body_errors(name, dilation):
    """-> ({stage: worst e over its parameter gradients}, number of gradients, taps of the training pass, the backbone)."""
    layers, groups = (BB._RESNEXT[name][0], BB._RESNEXT[name][1]) if name in BB._RESNEXT else (BB._RESNET_LAYERS[name], 1)
    bb = BB.Backbone(name, 1, True, dilation, 'frozen_batchnorm')
    bb.load_state_dict(_backbone_sd(name))
    bb = bb.cuda().train()
    img = _image()
    Fn.stash_reset()
    taps = bb(img.permute(0, 2, 3, 1).contiguous().cuda())
    cots = [_normal(f'resnext-body-cot{i}', tuple(t.permute(0, 3, 1, 2).shape)) for i, t in enumerate(taps)]
    sum((t * c.permute(0, 2, 3, 1).contiguous().cuda()).sum() for t, c in zip(taps, cots)).backward()
    _, ref = gconv_bwd_ref.body_grads(_backbone_sd(name), img, layers, cots, groups=groups, dilation=dilation)
    params = dict(bb.named_parameters())
    assert sorted(params) == sorted(ref)
    worst = {}
    for k, v in params.items():
        assert v.grad is not None and torch.isfinite(v.grad).all(), k
        worst[_stage(k)] = max(worst.get(_stage(k), 0.0), _rel(v.grad.reshape(ref[k].shape), ref[k]))
    return worst, len(params), [t.detach() for t in taps], bb


@pytest.mark.parametrize('dilation', [False, True])
def test_resnext50_parameter_gradients_against_float64_autograd(dilation):
    e_rx, n_rx, taps, bb = _body_errors(RX, dilation)
    e_rn, n_rn, _, _ = _body_errors('resnet50', dilation)
    # of the architecture's 161 tensors with a gradient the 106 BatchNorm affines are FrozenBN buffers here: 53 convolution weights and
    # init_conv's weight and bias remain, and every one of them is compared
    assert n_rx == n_rn == 55, (n_rx, n_rn)
    for st in ('stem', 'layer1', 'layer2', 'layer3', 'layer4'):
        print(f'dilation={dilation} {st}: worst e_resnext = {e_rx[st]:.3e}  worst e_resnet50 = {e_rn[st]:.3e}')
    # how much each stage's yardstick weighs: ResNet-50's stem, layer1 and layer2 gradients carry the error of its F(4x4,3x3) backward
    # convolutions (4e-4, 1.5e-3, 3e-6), so only layer3 and layer4 (1.3e-6, 1.5e-6) bound the ResNeXt figures tightly here; the early
    # stages' grouped gradients are held to fp32 level by the block-pair test above (layer1.0 -> layer2.0, yardstick 4e-7) and to the
    # bit by tests/test_gpu_gconv_bwd.py
    for st in e_rx:
        assert e_rx[st] <= MARGIN * e_rn[st], (st, e_rx, e_rn)
    # the training chain runs the launches of the inference chain: the same bits
    with torch.no_grad():
        ev = bb.eval()(_image().permute(0, 2, 3, 1).contiguous().cuda())
    assert all(torch.equal(a, b) for a, b in zip(taps, ev))


# ------------------------------------------------------------------------------------------------------ the public route
def test_training_steps_update_the_resnext_backbone():
    from birdsoundclassif_amd.nets import build_model
    from birdsoundclassif_amd.train import build_optimizer, default_args, train_one_step
    args = default_args(device='cuda', backbone=RX, lr_backbone=1e-5)
    model, crit = build_model(args)
    model.load_state_dict(filler_state_dict(backbone=RX))
    model = model.cuda().train()
    crit.train()
    opt, _ = build_optimizer(model, args)
    before = {k: v.detach().clone() for k, v in model.state_dict().items() if k.startswith('backbone.0.')}
    fpn_before = model.fpn.out_convs['0'].weight.detach().clone()
    head_before = model.head.fast_rcnn.rcnn.bbox_reg_layer.weight.detach().clone()
    img = torch.from_numpy(synth.image_batch(0, 2))
    bb, ids, lengths = synth.label_batch(0, 2)
    np.random.seed(7)
    loss = train_one_step(model, crit, opt, [img, img, bb, ids, lengths], args.clip_max_norm, 'cuda', negative_sample=False)
    torch.cuda.synchronize()
    vals = {k: float(v.detach() if torch.is_tensor(v) else v) for k, v in loss.items()}
    print(vals)
    assert vals and all(np.isfinite(v) for v in vals.values())
    after = {k: v.detach().clone() for k, v in model.state_dict().items() if k.startswith('backbone.0.')}
    convs = [k for k in before if k.startswith('backbone.0.body.') and k.endswith('.weight') and
             ('conv' in k.rsplit('.', 2)[-2] or k.endswith('downsample.0.weight'))]
    assert len(convs) == 53, len(convs)
    for k in convs + ['backbone.0.init_conv.weight', 'backbone.0.init_conv.bias']:
        assert not torch.equal(before[k], after[k]), f'{k} did not change'
    frozen = [k for k in before if k not in convs and not k.startswith('backbone.0.init_conv.')]
    assert len(frozen) == 53 * 4, len(frozen)
    for k in frozen:
        assert torch.equal(before[k], after[k]), f'FrozenBN buffer {k} changed'
    assert not torch.equal(fpn_before, model.fpn.out_convs['0'].weight) and \
        not torch.equal(head_before, model.head.fast_rcnn.rcnn.bbox_reg_layer.weight)
    # a second step: the prepared copies of the grouped weights (_prep.gconv / _prep.gconv_dgrad) must follow the optimiser's update
    from birdsoundclassif_amd.nets import _prep
    w2 = model.backbone[0].body.layer1[0].conv2.weight
    img2 = torch.from_numpy(synth.image_batch(1, 2))
    bb2, ids2, lengths2 = synth.label_batch(1, 2)
    loss2 = train_one_step(model, crit, opt, [img2, img2, bb2, ids2, lengths2], args.clip_max_norm, 'cuda', negative_sample=False)
    torch.cuda.synchronize()
    vals2 = {k: float(v.detach() if torch.is_tensor(v) else v) for k, v in loss2.items()}
    print(vals2)
    assert all(np.isfinite(v) for v in vals2.values())
    assert not torch.equal(after['backbone.0.body.layer1.0.conv2.weight'], w2.detach())
    with torch.no_grad():
        assert torch.equal(_prep.gconv(w2, 32), _prep._gconv_fragments(w2.detach().clone(), 32)), 'stale prepared weights'
