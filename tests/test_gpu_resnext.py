"""GPU: the ResNeXt backbones (`--backbone resnext50_32x4d | resnext101_32x8d | resnext101_64x4d`) from the taps up to the public
routes.  There is no ResNeXt golden fixture (the oracle's torchvision stand-in knows ResNet-50 only): the reference is the float64
restatement of the published architecture in tests/gconv_ref.py, and the yardstick for the error is what the ResNet-50 kernels -- code
this feature does not touch -- reach against the SAME restatement (groups = 1) on the same image."""
import ast
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gconv_ref                                                              # noqa: E402
from birdsoundclassif_amd import synth                                        # noqa: E402
from birdsoundclassif_amd.nets import backbone as BB                          # noqa: E402
from helpers import filler_state_dict                                         # noqa: E402

RX = 'resnext50_32x4d'
PREFIX = 'backbone.0.'


def _image(B=2, H=64, W=96):
    """[B,1,H,W] in [0,1]: layer3 of a 64 x 96 image is 4 x 6, even, as the dilated layer4 (SpaceToBatch2) needs."""
    return torch.from_numpy(synth.uniform(('resnext-img', B, H, W), B * H * W).astype(np.float32)).reshape(B, 1, H, W)


_SD = {}


def _backbone_sd(name):
    if name not in _SD:
        _SD[name] = {k[len(PREFIX):]: v for k, v in filler_state_dict(backbone=name).items() if k.startswith(PREFIX)}
    return _SD[name]


def _backbone(name, dilation, train_backbone=False):
    bb = BB.Backbone(name, 1, train_backbone, dilation, 'frozen_batchnorm')
    bb.load_state_dict(_backbone_sd(name))
    return bb.cuda().eval()


def _taps(bb, img):
    return [t.permute(0, 3, 1, 2) for t in bb(img.permute(0, 2, 3, 1).contiguous().cuda())]


_REF = {}


def _ref_taps(name, dilation):
    """float64 taps of the restatement, computed once per (backbone, dilation) and never modified."""
    key = (name, bool(dilation))
    if key not in _REF:
        layers, groups = (BB._RESNEXT[name][0], BB._RESNEXT[name][1]) if name in BB._RESNEXT else (BB._RESNET_LAYERS[name], 1)
        with torch.no_grad():
            _REF[key] = gconv_ref.resnet_taps(_backbone_sd(name), _image(), layers, groups=groups, dilation=dilation)
    return _REF[key]


def _rel_errors(name, dilation):
    with torch.no_grad():
        got = _taps(_backbone(name, dilation), _image())
    ref = _ref_taps(name, dilation)
    assert [tuple(g.shape) for g in got] == [tuple(r.shape) for r in ref]
    return [float((g.double().cpu() - r).abs().max() / r.abs().max()) for g, r in zip(got, ref)], got


@pytest.mark.parametrize('dilation', [False, True])
def test_resnext50_taps_against_the_float64_restatement(dilation):
    e_rx, got = _rel_errors(RX, dilation)
    e_rn, _ = _rel_errors('resnet50', dilation)
    assert [g.shape[1] for g in got] == [64, 256, 512, 1024, 2048]
    assert tuple(got[4].shape[2:]) == ((4, 6) if dilation else (2, 3))
    for i, g in enumerate(got):
        nz = float((g != 0).float().mean())
        print(f'dilation={dilation} tap {i} {tuple(g.shape)}: e_resnext = {e_rx[i]:.3e}  e_resnet50 = {e_rn[i]:.3e}  '
              f'non-zero {nz:.2f}  max {float(g.max()):.3g}')
        # the filler weights (He-scaled on the grouped fan-in) neither kill nor saturate the ResNeXt activations: no taming needed
        assert torch.isfinite(g).all() and 0.05 < nz and 0.01 < float(g.max()) < 1e3
    for i in range(5):
        # 4 x: another weight draw and 1x1 convolutions with up to twice the K (sqrt 2 on the rms error); an indexing or group-mapping
        # error is of order 1, a bf16-level loss about 2^-9
        assert e_rx[i] <= 4 * e_rn[i], (i, e_rx, e_rn)


def _block_sd(mod, prefix):
    sd = synth.fill_state_dict({prefix + k: tuple(v.shape) for k, v in mod.state_dict().items()})
    mod.load_state_dict({k[len(prefix):]: v for k, v in sd.items()})
    return sd


def _block_pair(groups, base_width):
    """layer1.0 -> layer2.0 of a (ResNeXt | ResNet) body in isolation -> relative errors of the two outputs."""
    N = BB.FrozenBatchNorm2d
    ds = lambda i, o, s: torch.nn.Sequential(torch.nn.Conv2d(i, o, 1, stride=s, bias=False), N(o))
    mk = (lambda i, p, s: BB._GroupedBottleneck(i, p, s, ds(i, 4 * p, s), N, groups, base_width)) if groups > 1 else \
        (lambda i, p, s: BB._Bottleneck(i, p, s, ds(i, 4 * p, s), N))
    blocks = [mk(64, 64, 1), mk(256, 128, 2)]
    sd = {}
    for b, p in zip(blocks, ('body.layer1.0.', 'body.layer2.0.')):
        sd.update(_block_sd(b, p))
    x = torch.from_numpy(synth.normal('resnext-block-x', 2 * 64 * 13 * 21).astype(np.float32)).reshape(2, 64, 13, 21).clamp_min(0)
    errs = []
    with torch.no_grad():
        g, r = x.permute(0, 2, 3, 1).contiguous().cuda(), x.double()
        for b, p, s in zip(blocks, ('body.layer1.0', 'body.layer2.0'), (1, 2)):
            g = b.cuda().eval()(g)
            r = gconv_ref.bottleneck(r, sd, p, s, groups)
            assert 0.05 < float((g != 0).float().mean())
            errs.append(float((g.permute(0, 3, 1, 2).double().cpu() - r).abs().max() / r.abs().max()))
    return errs


def test_resnext101_64x4d_block_pair():
    """G = 64: layer1.0 (256 channels in 64 groups of 4) and layer2.0 (512 in 64 groups of 8, stride 2) on a 13 x 21 map."""
    e_rx, e_rn = _block_pair(64, 4), _block_pair(1, 64)
    print(f'64x4d block pair: e_resnext = {e_rx}  e_resnet = {e_rn}')
    for a, b in zip(e_rx, e_rn):
        assert a <= 4 * b, (e_rx, e_rn)


# ------------------------------------------------------------------------------------------------------ gradient rules
def test_frozen_backbone_runs_under_enable_grad_bit_identically():
    bb = _backbone(RX, False)
    assert not any(p.requires_grad for p in bb.parameters())
    with torch.no_grad():
        a = _taps(bb, _image())
    with torch.enable_grad():
        b = _taps(bb, _image())
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and not any(t.requires_grad for t in b)


def test_a_trainable_grouped_weight_raises_when_a_gradient_is_asked_for():
    bb = _backbone(RX, False)
    bb.body.layer2[1].conv2.weight.requires_grad_(True)
    with torch.no_grad():
        _taps(bb, _image())                                         # inference is unaffected
    with torch.enable_grad(), pytest.raises(NotImplementedError, match='--lr_backbone 0'):
        _taps(bb, _image())
    # a backbone built for training (checkpoint args with lr_backbone > 0) constructs and infers, and raises only here
    tb = _backbone(RX, False, train_backbone=True)
    with torch.no_grad():
        _taps(tb, _image())
    with torch.enable_grad(), pytest.raises(NotImplementedError, match='--lr_backbone 0'):
        _taps(tb, _image())


def test_one_training_step_behind_a_frozen_resnext():
    from birdsoundclassif_amd.nets import build_model
    from birdsoundclassif_amd.train import build_optimizer, default_args, train_one_step
    args = default_args(device='cuda', backbone=RX, lr_backbone=0.0)
    model, crit = build_model(args)
    model.load_state_dict(filler_state_dict(backbone=RX))
    model = model.cuda().train()
    crit.train()
    opt, _ = build_optimizer(model, args)
    body = {k: v.detach().clone() for k, v in model.state_dict().items() if k.startswith('backbone.0.body.')}
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
    after = model.state_dict()
    assert len(body) == 53 * 5 and all(torch.equal(v, after[k]) for k, v in body.items())
    assert not torch.equal(fpn_before, model.fpn.out_convs['0'].weight) and \
        not torch.equal(head_before, model.head.fast_rcnn.rcnn.bbox_reg_layer.weight)


# ------------------------------------------------------------------------------------------------------ public routes
@pytest.fixture(scope='module')
def checkpoint(tmp_path_factory):
    """A checkpoint folder in the reference layout whose args name the ResNeXt backbone -- with the lr_backbone > 0 a training run
    leaves there."""
    from birdsoundclassif_amd.train import default_args
    root = tmp_path_factory.mktemp('resnext')
    ck = root / 'model_weights'
    ck.mkdir()
    args = default_args(device='cuda', backbone=RX)
    assert args.lr_backbone > 0
    cfg = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in vars(args).items() if k not in ('scales',)}
    (ck / 'args').write_text(json.dumps(cfg))
    torch.save({'checkpoints': filler_state_dict(backbone=RX), 'steps': 0, 'epoch': 0, 'best_val_cls_loss': 99}, str(ck / 'model_chkpt.pt'))
    (root / 'bird_dict.json').write_text(json.dumps({f'Species {i}': i for i in range(1, 151)}))
    return root


def test_loaded_model_detects_and_the_captured_route_gives_the_same_bits(checkpoint):
    from birdsoundclassif_amd import bulk
    from birdsoundclassif_amd.run_detection import load_model
    model, args = load_model(str(checkpoint / 'model_weights'))
    assert args.backbone == RX and args.lr_backbone > 0
    assert isinstance(model.backbone[0].body.layer1[0], BB._GroupedBottleneck) and not model.training
    pcm = torch.from_numpy(synth.clip_batch_pcm16(500, 2)).cuda()
    det = bulk.GraphedDetector(model, 2, 66150, 22050, min_score=0.05)
    try:
        c = det.census
        assert c['memset'] == c['memcpy'] == c['host'] == c['other'] == 0 and c['kernel'] > 100, c
        with torch.no_grad():
            imgs, _ = det.fe(pcm, 22050)
            imgs = imgs[:, 0][:, None].contiguous()
            d, n = model.detect(imgs, 0.3, 0.05)
            dc, nc = model.detect_calls(imgs, None, 0.3, 0.05)
            dicts = model(imgs, 0.3, 0.05)
        d, n = d.clone(), n.clone()
        det.pcm.copy_(pcm)
        det.replay()
        torch.cuda.synchronize()
        assert int(n.sum()) > 0 and len(dicts) == 2
        assert torch.equal(d, dc) and torch.equal(n, nc)
        assert torch.equal(det.n_det, n) and torch.equal(det.det, d)
    finally:
        det.close()


def test_cli_writes_the_same_files_on_both_routes(checkpoint):
    import shutil
    from birdsoundclassif_amd import nbm_detect
    a, b = checkpoint / 'bulk', checkpoint / 'perfile'
    a.mkdir()
    for i in range(3):
        synth.write_wav(str(a / f'clip{i}.wav'), synth.clip_pcm16(600 + i), 22050)
    shutil.copytree(str(a), str(b))
    common = ['--ckpt', str(checkpoint / 'model_weights'), '--min_score', '0.05', '--batch', '4',
              '--bird_dict', str(checkpoint / 'bird_dict.json')]
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
