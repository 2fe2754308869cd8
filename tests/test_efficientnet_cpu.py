"""CPU: the EfficientNet backbones (`--backbone efficientnet_b0 .. efficientnet_b4`) pinned to PUBLIC facts about torchvision's
definitions (torchvision is absent here): the tap channels, the state_dict key names under the reference's wrapper, the block counts per
stage and the documented parameter counts of the whole networks -- which a wrong width, depth, squeeze width or rounding rule cannot
reproduce for all five.  Construction only, no compute."""
import numpy as np
import pytest

import effnet_ref
from helpers import filler_state_dict, state_dict_shapes

BODY = 'backbone.0.body.'
NAMES = ['efficientnet_b0', 'efficientnet_b1', 'efficientnet_b2', 'efficientnet_b3', 'efficientnet_b4']
TAP_CHANNELS = {'efficientnet_b0': [16, 24, 40, 112, 320], 'efficientnet_b1': [16, 24, 40, 112, 320],
                'efficientnet_b2': [16, 24, 48, 120, 352], 'efficientnet_b3': [24, 32, 48, 136, 384],
                'efficientnet_b4': [24, 32, 56, 160, 448]}
PARAMETERS = {'efficientnet_b0': 5_288_548, 'efficientnet_b1': 7_794_184, 'efficientnet_b2': 9_109_994,
              'efficientnet_b3': 12_233_232, 'efficientnet_b4': 19_341_616}       # torchvision's documented counts
BLOCKS = {'efficientnet_b0': [1, 2, 2, 3, 3, 4, 1], 'efficientnet_b1': [2, 3, 3, 4, 4, 5, 2], 'efficientnet_b2': [2, 3, 3, 4, 4, 5, 2],
          'efficientnet_b3': [2, 3, 3, 5, 5, 6, 2], 'efficientnet_b4': [2, 4, 4, 6, 6, 8, 2]}       # ceil(repeats * depth)
NORM = ('weight', 'bias', 'running_mean', 'running_var')


def _shapes(name):
    return state_dict_shapes(backbone=name, lr_backbone=0.0)


def _body(name):
    return {k[len(BODY):]: v for k, v in _shapes(name).items() if k.startswith(BODY)}


@pytest.mark.parametrize('name', NAMES)
def test_taps_blocks_and_published_parameter_counts(name):
    from birdsoundclassif_amd.nets import build_model
    from birdsoundclassif_amd.train import default_args
    args = default_args(device='cpu', backbone=name, lr_backbone=0.0)
    model, _ = build_model(args)
    bb = model.backbone[0]
    assert bb.num_channels == TAP_CHANNELS[name] == list(model.backbone.num_channels)
    assert bb.strides == [2, 4, 8, 16, 32] and args.n_layers == 5
    s = _shapes(name)
    for i, c in enumerate(TAP_CHANNELS[name]):
        assert s[f'fpn.pt_wise.{i}.weight'] == (384, c, 1, 1)
    body = _body(name)
    # stage index 8 (the 1x1 head convolution) and the classifier are not there
    assert sorted({int(k.split('.')[0]) for k in body}) == list(range(8))
    assert [1 + max(int(k.split('.')[1]) for k in body if k.startswith(f'{st}.')) for st in range(1, 8)] == BLOCKS[name]
    assert [n for *_, n in effnet_ref.stages(name)] == BLOCKS[name]
    # the whole published network = what the body holds (norm buffers aside) + the dropped head convolution, its norm and the classifier
    last = TAP_CHANNELS[name][-1]
    dropped = last * 4 * last + 2 * 4 * last + 4 * last * 1000 + 1000
    held = sum(int(np.prod(v)) for k, v in body.items() if 'running_' not in k)
    assert held + dropped == PARAMETERS[name]
    assert effnet_ref.parameter_count(name) == PARAMETERS[name]
    assert not any(p.requires_grad for p in bb.parameters())          # init_conv included


def test_b0_key_set():
    body = _body('efficientnet_b0')
    assert not any('num_batches_tracked' in k for k in body)
    s = _shapes('efficientnet_b0')
    assert s['backbone.0.init_conv.weight'] == (3, 1, 1, 1) and s['backbone.0.init_conv.bias'] == (3,)
    conv_norm = lambda p, shape: {p + '.0.weight': shape, **{f'{p}.1.{leaf}': (shape[0],) for leaf in NORM}}
    se = lambda p, c, q: {p + '.fc1.weight': (q, c, 1, 1), p + '.fc1.bias': (q,), p + '.fc2.weight': (c, q, 1, 1), p + '.fc2.bias': (c,)}
    want = conv_norm('0', (32, 3, 3, 3))                                                   # the stem
    # stage 1: no expand convolution -- depthwise 0, SE 1, project 2; squeeze width 32 // 4
    want.update({**conv_norm('1.0.block.0', (32, 1, 3, 3)), **se('1.0.block.1', 32, 8), **conv_norm('1.0.block.2', (16, 32, 1, 1))})
    # stage 3, first block: 24 -> 40, 5 x 5 / stride 2, expanded to 144, squeezed to 24 // 4
    want.update({**conv_norm('3.0.block.0', (144, 24, 1, 1)), **conv_norm('3.0.block.1', (144, 1, 5, 5)), **se('3.0.block.2', 144, 6),
                 **conv_norm('3.0.block.3', (40, 144, 1, 1))})
    # the last block: 192 -> 320, 3 x 3
    want.update({**conv_norm('7.0.block.0', (1152, 192, 1, 1)), **conv_norm('7.0.block.1', (1152, 1, 3, 3)), **se('7.0.block.2', 1152, 48),
                 **conv_norm('7.0.block.3', (320, 1152, 1, 1))})
    for k, v in want.items():
        assert body.get(k) == v, (k, body.get(k), v)
    for p in ('0.', '1.0.', '3.0.', '7.0.'):
        assert sorted(k for k in body if k.startswith(p)) == sorted(k for k in want if k.startswith(p))
    assert '1.0.block.3.0.weight' not in body and '8.0.weight' not in body
    # 16 blocks: 1 without an expand convolution (14 leaves), 15 with (19 leaves), + the stem's 5
    assert len(body) == 5 + 14 + 15 * 19


def test_refusals_name_the_limit():
    from birdsoundclassif_amd.nets import backbone as BB
    with pytest.raises(NotImplementedError, match='--lr_backbone 0'):
        state_dict_shapes(backbone='efficientnet_b0')                                 # train.py's default lr_backbone is 1e-5
    with pytest.raises(ValueError, match='efficientnet_b4.*efficientnet_v2'):
        state_dict_shapes(backbone='efficientnet_v2_s', lr_backbone=0.0)
    with pytest.raises(ValueError, match='not supported'):
        BB.Backbone('vgg16_bn', 1, False, False, 'frozen_batchnorm')
    with pytest.raises(NotImplementedError, match='frozen_batchnorm'):
        BB.Backbone('efficientnet_b0', 1, False, False, 'batchnorm')
    with pytest.raises(NotImplementedError, match='inpt_channels'):
        BB.Backbone('efficientnet_b0', 3, False, False, 'frozen_batchnorm')
    BB.Backbone('efficientnet_b0', 1, False, True, 'frozen_batchnorm')               # --dilation is accepted (and has no effect)


def test_a_training_checkpoint_loads_for_inference():
    """`load_model` builds for evaluation: an lr_backbone > 0 in the checkpoint's arguments does not refuse an EfficientNet body there."""
    from birdsoundclassif_amd.nets.backbone import build_backbone
    from birdsoundclassif_amd.train import default_args
    args = default_args(device='cpu', backbone='efficientnet_b2')
    assert args.lr_backbone > 0
    m = build_backbone(args, inference=True)
    assert m.num_channels == TAP_CHANNELS['efficientnet_b2'] and not any(p.requires_grad for p in m.parameters())
    with pytest.raises(NotImplementedError, match='--lr_backbone 0'):
        build_backbone(args)


def test_filler_is_usable_and_leaves_the_other_names_alone():
    """The fillers of the new leaves are positive where a variance must be; every name of the default model keeps its value whether or
    not EfficientNet names are in the same mapping."""
    sd = filler_state_dict(backbone='efficientnet_b0', lr_backbone=0.0)
    for k, v in sd.items():
        if k.startswith(BODY) and k.endswith('running_var'):
            assert float(v.min()) >= 0.9
    assert abs(float(sd[BODY + '3.0.block.1.0.weight'].std()) - (2.0 / 25) ** 0.5) < 0.03        # depthwise fan-in: k * k
    assert 0.5 < float(sd[BODY + '3.0.block.2.fc2.bias'].mean()) < 1.5
    ref = filler_state_dict()
    shared = [k for k in ref if k in sd and ref[k].shape == sd[k].shape]
    assert len(shared) > 50 and all((ref[k] == sd[k]).all() for k in shared)
