"""GPU: `--norm_layer_backbone batchnorm` on the public routes -- optimiser steps with a trainable and with a frozen backbone (live
statistics either way, as nn.BatchNorm2d in `.train()`), the refusal of a gradient in eval mode, and a checkpoint folder whose args
say `batchnorm` through `load_model` / `detect`, the captured bulk route and the command line."""
import ast
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from birdsoundclassif_amd import synth                                        # noqa: E402
from birdsoundclassif_amd.nets import backbone as BB, functional as Fn        # noqa: E402
from helpers import filler_state_dict                                         # noqa: E402

BODY = 'backbone.0.body.'


def _step(lr_backbone):
    from birdsoundclassif_amd.nets import build_model
    from birdsoundclassif_amd.train import build_optimizer, default_args, train_one_step
    args = default_args(device='cuda', norm_layer_backbone='batchnorm', lr_backbone=lr_backbone)
    model, crit = build_model(args)
    model.load_state_dict(filler_state_dict(norm_layer_backbone='batchnorm'))
    model = model.cuda().train()
    crit.train()
    opt, _ = build_optimizer(model, args)
    before = {k: v.detach().clone() for k, v in model.state_dict().items() if k.startswith('backbone.0.')}
    head_before = model.head.fast_rcnn.rcnn.bbox_reg_layer.weight.detach().clone()
    img = torch.from_numpy(synth.image_batch(0, 2))
    bb, ids, lengths = synth.label_batch(0, 2)
    np.random.seed(7)
    loss = train_one_step(model, crit, opt, [img, img, bb, ids, lengths], args.clip_max_norm, 'cuda', negative_sample=False)
    torch.cuda.synchronize()
    vals = {k: float(v.detach() if torch.is_tensor(v) else v) for k, v in loss.items()}
    print(vals)
    assert vals and all(np.isfinite(v) for v in vals.values())
    assert not torch.equal(head_before, model.head.fast_rcnn.rcnn.bbox_reg_layer.weight)
    after = {k: v.detach().clone() for k, v in model.state_dict().items() if k.startswith('backbone.0.')}
    convs = [k for k in before if k.startswith(BODY) and k.endswith('.weight') and
             ('conv' in k.rsplit('.', 2)[-2] or k.endswith('downsample.0.weight'))]
    stats = [k for k in before if k.endswith(('running_mean', 'running_var'))]
    counters = [k for k in before if k.endswith('num_batches_tracked')]
    affines = [k for k in before if k.startswith(BODY) and k not in convs and k not in stats and k not in counters]
    assert (len(convs), len(affines), len(stats), len(counters)) == (53, 106, 106, 53)
    return model, opt, before, after, convs, affines, stats, counters


def test_a_training_step_updates_weights_affines_and_statistics():
    model, opt, before, after, convs, affines, stats, counters = _step(1e-5)
    for k in convs + affines + ['backbone.0.init_conv.weight', 'backbone.0.init_conv.bias'] + stats:
        assert not torch.equal(before[k], after[k]), f'{k} did not change'
        assert torch.isfinite(after[k]).all(), k
    assert all(int(after[k]) == 1 and int(before[k]) == 0 for k in counters)
    # every trainable backbone parameter sits in the --lr_backbone group, and data-parallel training would reduce every one of them
    ids = {id(p) for p in opt.param_groups[1]['params']} if hasattr(opt, 'param_groups') else None
    named = {n: p for n, p in model.named_parameters() if n.startswith('backbone.0.')}
    assert len(named) == 53 + 106 + 2 and all(p.requires_grad for p in named.values())
    if ids is not None:
        assert all(id(p) in ids for p in named.values())


def test_a_frozen_backbone_keeps_its_parameters_and_still_tracks_statistics():
    """The reference's quirk: --lr_backbone 0 freezes the parameters, but nn.BatchNorm2d in .train() normalises with batch statistics
    and updates the running ones."""
    _, _, before, after, convs, affines, stats, counters = _step(0.0)
    for k in convs + affines:
        assert torch.equal(before[k], after[k]), f'{k} changed'
    for k in stats:
        assert not torch.equal(before[k], after[k]), f'{k} did not change'
    assert all(int(after[k]) == 1 for k in counters)


def test_a_gradient_in_eval_mode_is_refused():
    N = BB.BatchNorm2d
    ds = torch.nn.Sequential(torch.nn.Conv2d(64, 256, 1, bias=False), N(256))
    x = torch.rand(1, 6, 9, 64, device='cuda')
    for blk in (BB._Bottleneck(64, 64, 1, ds, N), BB._GroupedBottleneck(64, 64, 1, ds, N, 32, 4)):
        blk = blk.cuda().eval()
        with pytest.raises(NotImplementedError, match=r'\.train\(\)'):
            blk(x)
        with torch.no_grad():
            y = blk(x)                                   # inference is unaffected
        Fn.stash_reset()
        z = blk.train()(x)
        assert z.requires_grad and y.shape == z.shape
    bb = BB.Backbone('resnet50', 1, True, False, 'batchnorm').cuda().eval()
    with pytest.raises(NotImplementedError, match=r'\.train\(\)'):
        bb(torch.rand(1, 64, 96, 1, device='cuda'))


# ------------------------------------------------------------------------------------------------------ public routes
def _write_ckpt(root, norm, sd):
    from birdsoundclassif_amd.train import default_args
    ck = root / 'model_weights'
    ck.mkdir(parents=True)
    args = default_args(device='cuda', norm_layer_backbone=norm)
    assert args.lr_backbone > 0
    cfg = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in vars(args).items() if k not in ('scales',)}
    (ck / 'args').write_text(json.dumps(cfg))
    torch.save({'checkpoints': sd, 'steps': 0, 'epoch': 0, 'best_val_cls_loss': 99}, str(ck / 'model_chkpt.pt'))
    (root / 'bird_dict.json').write_text(json.dumps({f'Species {i}': i for i in range(1, 151)}))
    return root


@pytest.fixture(scope='module')
def checkpoints(tmp_path_factory):
    """Two checkpoint folders in the reference layout holding the same tensors: args `batchnorm` / `frozen_batchnorm`."""
    sd = filler_state_dict(norm_layer_backbone='batchnorm')
    root = tmp_path_factory.mktemp('bn')
    frozen_sd = {k: v for k, v in sd.items() if not (k.startswith(BODY) and k.endswith('num_batches_tracked'))}
    return _write_ckpt(root / 'live', 'batchnorm', sd), _write_ckpt(root / 'frozen', 'frozen_batchnorm', frozen_sd)


def test_loaded_model_detects_like_the_frozen_one_and_the_captured_route_gives_the_same_bits(checkpoints):
    from birdsoundclassif_amd import bulk
    from birdsoundclassif_amd.run_detection import load_model
    live, frozen = checkpoints
    model, args = load_model(str(live / 'model_weights'))
    assert args.norm_layer_backbone == 'batchnorm' and isinstance(model.backbone[0].body.bn1, BB.BatchNorm2d) and not model.training
    fmodel, fargs = load_model(str(frozen / 'model_weights'))
    assert fargs.norm_layer_backbone == 'frozen_batchnorm' and isinstance(fmodel.backbone[0].body.bn1, BB.FrozenBatchNorm2d)
    pcm = torch.from_numpy(synth.clip_batch_pcm16(500, 2)).cuda()
    det = bulk.GraphedDetector(model, 2, 66150, 22050, min_score=0.05)
    try:
        c = det.census
        assert c['memset'] == c['memcpy'] == c['host'] == c['other'] == 0 and c['kernel'] > 100, c
        with torch.no_grad():
            imgs, _ = det.fe(pcm, 22050)
            imgs = imgs[:, 0][:, None].contiguous()
            d, n = model.detect(imgs, 0.3, 0.05)
            fd, fn = fmodel.detect(imgs, 0.3, 0.05)
        d, n = d.clone(), n.clone()
        det.pcm.copy_(pcm)
        det.replay()
        torch.cuda.synchronize()
        assert int(n.sum()) > 0
        assert torch.equal(d, fd) and torch.equal(n, fn)
        assert torch.equal(det.n_det, n) and torch.equal(det.det, d)
    finally:
        det.close()
    assert all(int(m.num_batches_tracked) == 0 for m in model.modules() if isinstance(m, BB.BatchNorm2d))


def test_cli_writes_the_same_files_on_both_routes(checkpoints):
    import shutil
    from birdsoundclassif_amd import nbm_detect
    live, _ = checkpoints
    a, b = live / 'bulk', live / 'perfile'
    a.mkdir()
    for i in range(3):
        synth.write_wav(str(a / f'clip{i}.wav'), synth.clip_pcm16(600 + i), 22050)
    shutil.copytree(str(a), str(b))
    common = ['--ckpt', str(live / 'model_weights'), '--min_score', '0.05', '--batch', '4', '--bird_dict', str(live / 'bird_dict.json')]
    nbm_detect.main(common + ['--audio_dir', str(a), '--bulk_batch', '4'])
    nbm_detect.main(common + ['--audio_dir', str(b), '--no_bulk'])
    names = sorted(p.name for p in a.glob('*.txt'))
    assert len(names) == 3 and names == sorted(p.name for p in b.glob('*.txt'))
    n = 0
    for name in names:
        ta, tb = (a / name).read_text(), (b / name).read_text()
        assert ta == tb, name
        n += sum(len(v['scores']) for v in ast.literal_eval(ta).values())
    assert n > 0
