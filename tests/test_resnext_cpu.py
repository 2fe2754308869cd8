"""CPU: the ResNeXt backbones (`--backbone resnext50_32x4d | resnext101_32x8d | resnext101_64x4d`) pinned to PUBLIC facts about
torchvision's ResNeXt definitions (torchvision is absent here, as for ResNet-50: test_resnet50_public_facts.py): the grouped `conv2`
shapes, the published parameter counts and the state_dict key names, which are ResNet's.  Construction only, no compute."""
import numpy as np
import pytest

from helpers import state_dict_shapes

BODY = 'backbone.0.body.'
# (layer1.0.conv2, layer4.2.conv2, published parameter count of the torchvision model - the 2 049 000 of its unused `fc`)
FACTS = {'resnext50_32x4d': ((128, 4, 3, 3), (1024, 32, 3, 3), 25_028_904 - 2_049_000),
         'resnext101_32x8d': ((256, 8, 3, 3), (2048, 64, 3, 3), 88_791_336 - 2_049_000),
         'resnext101_64x4d': ((256, 4, 3, 3), (2048, 32, 3, 3), 83_455_272 - 2_049_000)}


def _body(shapes):
    return {k[len(BODY):]: v for k, v in shapes.items() if k.startswith(BODY)}


@pytest.mark.parametrize('name', sorted(FACTS))
def test_grouped_shapes_and_published_parameter_counts(name):
    first, last, count = FACTS[name]
    s = state_dict_shapes(backbone=name)
    assert s[BODY + 'layer1.0.conv2.weight'] == first
    assert s[BODY + 'layer4.2.conv2.weight'] == last
    assert count == {'resnext50_32x4d': 22_979_904, 'resnext101_32x8d': 86_742_336, 'resnext101_64x4d': 81_406_272}[name]
    body = _body(s)
    got = sum(int(np.prod(v)) for k, v in body.items() if 'running_' not in k and 'num_batches_tracked' not in k)
    assert got == count
    # the rest of the detector does not see the backbone's inside: the five taps keep the ResNet channel counts
    assert s[BODY + 'layer1.2.conv3.weight'][0] == 256 and s[BODY + 'layer4.2.conv3.weight'][0] == 2048
    assert s['fpn.pt_wise.4.weight'] == (384, 2048, 1, 1)


def test_resnext50_has_the_resnet50_key_set():
    a, b = _body(state_dict_shapes(backbone='resnext50_32x4d')), _body(state_dict_shapes(backbone='resnet50'))
    assert list(a) == list(b)
    diff = sorted(k for k in a if a[k] != b[k])
    # only the inner width differs: conv1 / bn1 / conv2 / bn2 and the input side of conv3 of every block
    assert diff and all(k.split('.')[2] in ('conv1', 'bn1', 'conv2', 'bn2', 'conv3') for k in diff)
    assert a['layer3.0.downsample.0.weight'] == b['layer3.0.downsample.0.weight'] == (1024, 512, 1, 1)


def test_resnet50_is_unchanged():
    s = state_dict_shapes(backbone='resnet50')
    assert len(s) == 407 and sum(int(np.prod(v)) if len(v) else 1 for v in s.values()) == 43930779
    assert s == state_dict_shapes()
    assert s[BODY + 'layer1.0.conv2.weight'] == (64, 64, 3, 3)


def test_unknown_backbone_lists_the_new_names():
    with pytest.raises(ValueError, match='resnext101_64x4d'):
        state_dict_shapes(backbone='wide_resnet50_2')


def test_checkpoint_of_a_training_run_still_constructs():
    """`lr_backbone > 0` in a checkpoint's args must not stop construction: the missing backward pass is reported when a gradient is
    asked for, not before."""
    from birdsoundclassif_amd.nets import build_model
    from birdsoundclassif_amd.train import default_args
    model, _ = build_model(default_args(device='cpu', backbone='resnext50_32x4d', lr_backbone=1e-5))
    assert model.backbone[0].body.layer1[0].conv2.weight.requires_grad
    frozen, _ = build_model(default_args(device='cpu', backbone='resnext50_32x4d', lr_backbone=0.0))
    assert not any(p.requires_grad for p in frozen.backbone[0].parameters())
