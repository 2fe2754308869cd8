"""CPU: `--norm_layer_backbone batchnorm` -- construction, state_dict, parameter counts, refusals and the host-only plan of the
BatchNorm kernels (no compute on a device)."""
import pytest
import torch

from birdsoundclassif_amd import ops
from birdsoundclassif_amd.nets import backbone as BB
from helpers import state_dict_shapes


def _model(**kw):
    from birdsoundclassif_amd.nets import build_model
    from birdsoundclassif_amd.train import default_args
    return build_model(default_args(device='cpu', **kw))[0]


def test_state_dict_is_the_frozen_one_plus_53_batch_counters():
    live = _model(norm_layer_backbone='batchnorm').state_dict()
    frozen = state_dict_shapes()
    extra = sorted(set(live) - set(frozen))
    assert set(frozen) <= set(live) and len(extra) == 53
    assert all(k.startswith('backbone.0.body.') and k.endswith('.num_batches_tracked') for k in extra)
    assert all(live[k].dtype == torch.int64 and live[k].dim() == 0 for k in extra)
    assert all(tuple(live[k].shape) == frozen[k] for k in frozen)


def test_body_parameter_count_is_torchvisions_resnet50_without_fc():
    body = BB.Backbone('resnet50', 1, True, False, 'batchnorm').body
    n_live = sum(p.numel() for p in body.parameters())
    assert n_live == 25_557_032 - 2_049_000 == 23_508_032
    frozen = BB.Backbone('resnet50', 1, True, False, 'frozen_batchnorm').body
    n_frozen = sum(p.numel() for p in frozen.parameters())
    assert n_live - n_frozen == 26_560 * 2 == 53_120
    norms = [m for m in body.modules() if isinstance(m, BB.BatchNorm2d)]
    assert len(norms) == 53 and sum(m.num_features for m in norms) == 26_560
    assert isinstance(norms[0], torch.nn.BatchNorm2d) and norms[0].eps == 1e-5 and norms[0].momentum == 0.1


@pytest.mark.parametrize('name', ['resnet50', 'resnext50_32x4d'])
@pytest.mark.parametrize('train', [False, True])
def test_requires_grad_follows_train_backbone(name, train):
    bb = BB.Backbone(name, 1, train, False, 'batchnorm')
    assert all(p.requires_grad == train for p in bb.body.parameters())
    assert len([k for k, _ in bb.body.named_parameters() if '.bn' in k or 'downsample.1' in k or k.startswith('bn1')]) == 106


def test_refusals():
    with pytest.raises(NotImplementedError, match='frozen_batchnorm'):
        BB.Backbone('efficientnet_b0', 1, False, False, 'batchnorm')
    for name in ('resnet50', 'resnext50_32x4d'):
        with pytest.raises(NotImplementedError, match='groupnorm'):
            BB.Backbone(name, 1, False, False, 'groupnorm')
    with pytest.raises(NotImplementedError):
        BB.Backbone('efficientnet_b0', 1, False, False, 'groupnorm')


def test_build_backbone_on_a_batchnorm_checkpoints_args():
    from birdsoundclassif_amd.train import default_args
    for inference in (False, True):
        for name in ('resnet50', 'resnext101_32x8d'):
            args = default_args(device='cpu', backbone=name, norm_layer_backbone='batchnorm', lr_backbone=1e-5)
            j = BB.build_backbone(args, inference=inference)
            assert isinstance(j[0].body.bn1, BB.BatchNorm2d) and j.num_channels == [64, 256, 512, 1024, 2048]


def test_eval_affine_of_a_live_norm_is_the_frozen_affine():
    live, frozen = BB.BatchNorm2d(8), BB.FrozenBatchNorm2d(8)
    g = torch.Generator().manual_seed(3)
    sd = {'weight': torch.rand(8, generator=g) + 0.5, 'bias': torch.randn(8, generator=g), 'running_mean': torch.randn(8, generator=g),
          'running_var': torch.rand(8, generator=g) + 0.5}
    frozen.load_state_dict(sd)
    live.load_state_dict(dict(sd, num_batches_tracked=torch.tensor(7)))
    assert all(torch.equal(a, b) for a, b in zip(live.affine(), frozen.affine()))
    assert sorted(live.state_dict()) == ['bias', 'num_batches_tracked', 'running_mean', 'running_var', 'weight']


@pytest.mark.parametrize('M,C', [(1, 64), (2, 64), (12_320_768, 64), (1536, 2048), (5000, 68), (257, 4)])
def test_bn_act_plan_is_a_function_of_the_shape(M, C):
    a, b = ops.bn_act_plan(M, C), ops.bn_act_plan(M, C)
    assert a == b and a[0] >= 1 and a[1] >= a[0] * 2 * C * 8 and a[1] % 16 == 0
    if M <= 2:
        assert a[0] == 1            # toy sizes: one workgroup per channel block
    if M == 12_320_768:
        assert a[0] >= 256          # the backbone's largest map: enough workgroups for 256 CUs


def test_bn_act_plan_refuses_what_the_kernels_refuse():
    from birdsoundclassif_amd._lib import NbmHipError
    with pytest.raises(NbmHipError, match='NBM_EUNSUPPORTED'):
        ops.bn_act_plan(16, 6)
    with pytest.raises(NbmHipError, match='NBM_EINVAL'):
        ops.bn_act_plan(0, 64)
