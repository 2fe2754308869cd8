"""GPU: the EfficientNet backbones (`--backbone efficientnet_b0 .. efficientnet_b4`) from the taps up to the public routes.  There is no
EfficientNet golden fixture (torchvision is absent): the reference is the float64 restatement of the published architecture in
tests/effnet_ref.py, and the yardstick for the error is what the ResNet-50 kernels -- code this feature does not touch -- reach against
THEIR restatement (tests/gconv_ref.py) on the same image in the same run."""
import ast
import json
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import effnet_ref                                                             # noqa: E402
import gconv_ref                                                              # noqa: E402
from birdsoundclassif_amd import synth                                        # noqa: E402
from birdsoundclassif_amd.nets import backbone as BB                          # noqa: E402
from helpers import filler_state_dict                                         # noqa: E402

B0 = 'efficientnet_b0'
PREFIX = 'backbone.0.'
# Worst measured ratio (EfficientNet tap error / ResNet-50 tap error, both relative to the tap's largest reference value) rounded up to
# the next power of two; profiles/efficientnet.txt holds the per-tap figures.  Never more than 16: an indexing, stride or gate-mapping
# error is of order 1 -- a million times the fp32 level -- and a bf16-level loss thousands of times it.
MAX_RATIO = 4          # measured: 2.22 (b0, tap 1), 1.77 (b4, tap 1)


def _image(B=2, H=64, W=96):
    """The image of test_gpu_resnext.py: the coarsest tap is 2 x 3."""
    return torch.from_numpy(synth.uniform(('resnext-img', B, H, W), B * H * W).astype(np.float32)).reshape(B, 1, H, W)


_SD, _REF, _GOT = {}, {}, {}


def _backbone_sd(name):
    if name not in _SD:
        kw = {'lr_backbone': 0.0} if name in BB._EFFICIENTNET else {}
        _SD[name] = {k[len(PREFIX):]: v for k, v in filler_state_dict(backbone=name, **kw).items() if k.startswith(PREFIX)}
    return _SD[name]


def _backbone(name, dilation=False):
    bb = BB.Backbone(name, 1, False, dilation, 'frozen_batchnorm')
    bb.load_state_dict(_backbone_sd(name))
    return bb.cuda().eval()


def _nhwc(img):
    return img.permute(0, 2, 3, 1).contiguous().cuda()


def _taps(bb, img):
    with torch.no_grad():
        return [t.permute(0, 3, 1, 2).cpu() for t in bb(_nhwc(img))]


def _ref(name):
    """float64 (stage-0 output or None, taps) of the restatements, computed once per backbone and never modified."""
    if name not in _REF:
        with torch.no_grad():
            if name in BB._EFFICIENTNET:
                _REF[name] = effnet_ref.taps(_backbone_sd(name), _image(), name)
            else:
                _REF[name] = (None, gconv_ref.resnet_taps(_backbone_sd(name), _image(), BB._RESNET_LAYERS[name]))
    return _REF[name]


def _got(name):
    if name not in _GOT:
        _GOT[name] = _taps(_backbone(name), _image())
    return _GOT[name]


def _rel_errors(name):
    got, ref = _got(name), _ref(name)[1]
    assert [tuple(g.shape) for g in got] == [tuple(r.shape) for r in ref]
    return [float((g.double() - r).abs().max() / r.abs().max()) for g, r in zip(got, ref)]


@pytest.mark.parametrize('name', [B0, 'efficientnet_b4'])
def test_taps_against_the_float64_restatement(name):
    e_en, e_rn, got = _rel_errors(name), _rel_errors('resnet50'), _got(name)
    assert [g.shape[1] for g in got] == {B0: [16, 24, 40, 112, 320], 'efficientnet_b4': [24, 32, 56, 160, 448]}[name]
    assert [tuple(g.shape[2:]) for g in got] == [(32, 48), (16, 24), (8, 12), (4, 6), (2, 3)]
    ratios = [a / b for a, b in zip(e_en, e_rn)]
    for i, g in enumerate(got):
        alive = float((g.abs() > 1e-3).float().mean())
        print(f'{name} tap {i} {tuple(g.shape)}: e_efficientnet = {e_en[i]:.3e}  e_resnet50 = {e_rn[i]:.3e}  ratio {ratios[i]:.2f}  '
              f'|x| > 1e-3: {alive:.2f}  std {float(g.std()):.3g}  max {float(g.abs().max()):.3g}')
        # the filler weights neither kill nor saturate the activations (SiLU outputs and linear taps: "non-zero" is "away from zero")
        assert torch.isfinite(g).all() and alive > 0.5 and float(g.std()) > 0.02 and float(g.abs().max()) < 1e3
    print(f'{name}: worst ratio {max(ratios):.2f}')
    assert max(ratios) <= MAX_RATIO, (ratios, e_en, e_rn)


def test_stem_border_rows_and_columns():
    """init_conv's bias is inside the image and not in the stem's zero padding: the first and last two rows and columns of the stage-0
    output against the restatement, at the taps' bound (yardstick: the ResNet-50 stem tap)."""
    bb = _backbone(B0)
    with torch.no_grad():
        got = bb.body.stem(_nhwc(_image()), bb.init_conv).permute(0, 3, 1, 2).cpu().double()
    ref = _ref(B0)[0]
    assert got.shape == ref.shape == (2, 32, 32, 48)
    border = torch.zeros(32, 48, dtype=torch.bool)
    border[:2] = border[-2:] = True
    border[:, :2] = border[:, -2:] = True
    e = float((got - ref).abs()[:, :, border].max() / ref.abs().max())
    e_rn = _rel_errors('resnet50')[0]
    print(f'stem border: e = {e:.3e}, ResNet-50 stem tap e = {e_rn:.3e}, ratio {e / e_rn:.2f}')
    assert e <= MAX_RATIO * e_rn
    # a bias that leaked into the padding would show here: the restatement with init_conv composed into the stem differs on the border
    sd = _backbone_sd(B0)
    w = (sd['body.0.0.weight'].double() * sd['init_conv.weight'].double().view(1, 3, 1, 1)).sum(1, keepdim=True)
    wb = (sd['body.0.0.weight'].double() * sd['init_conv.bias'].double().view(1, 3, 1, 1)).sum((1, 2, 3))
    naive = torch.nn.functional.conv2d(_image().double(), w, wb, stride=2, padding=1)
    naive = effnet_ref.silu(effnet_ref._bn(naive, sd, 'body.0.1'))
    assert float((naive - ref).abs()[:, :, border].max() / ref.abs().max()) > 100 * MAX_RATIO * e_rn


def test_image_0_does_not_depend_on_its_batch():
    bb = _backbone(B0)
    img = torch.cat([_image(), _image()[:1].flip(3)])
    one, three = _taps(bb, img[:1]), _taps(bb, img)
    assert all(torch.equal(a[0], b[0]) for a, b in zip(one, three))
    assert all(torch.equal(a[0], b[0]) for a, b in zip(one, _got(B0)))


def test_dilation_changes_nothing():
    assert all(torch.equal(a, b) for a, b in zip(_taps(_backbone(B0, dilation=True), _image()), _got(B0)))


def test_frozen_body_runs_under_enable_grad_without_a_tape():
    bb = _backbone(B0)
    assert not any(p.requires_grad for p in bb.parameters())
    with torch.enable_grad():
        taps = bb(_nhwc(_image()))
    assert not any(t.requires_grad for t in taps)
    assert all(torch.equal(t.permute(0, 3, 1, 2).cpu(), g) for t, g in zip(taps, _got(B0)))


def test_refusals():
    with pytest.raises(NotImplementedError, match='--lr_backbone 0'):
        BB.Backbone(B0, 1, True, False, 'frozen_batchnorm')                    # --lr_backbone 1e-5
    with pytest.raises(ValueError, match='not supported efficientnet_v2_s'):
        BB.Backbone('efficientnet_v2_s', 1, False, False, 'frozen_batchnorm')


# ------------------------------------------------------------------------------------------------------ public routes
@pytest.fixture(scope='module')
def checkpoint(tmp_path_factory):
    """A checkpoint folder in the reference layout whose args name the EfficientNet backbone -- with the lr_backbone > 0 an upstream
    training run leaves there."""
    from birdsoundclassif_amd.train import default_args
    root = tmp_path_factory.mktemp('efficientnet')
    ck = root / 'model_weights'
    ck.mkdir()
    args = default_args(device='cuda', backbone=B0, lr_backbone=0.0)
    cfg = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in vars(args).items() if k not in ('scales',)}
    cfg['lr_backbone'] = 1e-5
    (ck / 'args').write_text(json.dumps(cfg))
    torch.save({'checkpoints': filler_state_dict(backbone=B0, lr_backbone=0.0), 'steps': 0, 'epoch': 0, 'best_val_cls_loss': 99},
               str(ck / 'model_chkpt.pt'))
    (root / 'bird_dict.json').write_text(json.dumps({f'Species {i}': i for i in range(1, 151)}))
    return root


def test_loaded_model_detects_and_the_captured_route_gives_the_same_bits(checkpoint):
    from birdsoundclassif_amd import bulk
    from birdsoundclassif_amd.run_detection import load_model
    model, args = load_model(str(checkpoint / 'model_weights'))
    assert args.backbone == B0 and args.lr_backbone > 0
    assert isinstance(model.backbone[0].body, BB._EfficientNetBody) and not model.training
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
        assert int(n.sum()) > 0 and len(dicts) == 2 and bool(torch.isfinite(d).all())
        assert torch.equal(d, dc) and torch.equal(n, nc)
        assert torch.equal(det.n_det, n) and torch.equal(det.det, d)
    finally:
        det.close()


def test_cli_writes_the_same_files_on_every_route(checkpoint, monkeypatch):
    """Eight equal clips take `bulk.detect_files`, one short multi-window recording takes `bulk.detect_recordings` (captured graphs of
    kernel nodes only: both detectors refuse anything else), `--no_bulk` takes the per-file driver: the txt files are the same bytes."""
    from birdsoundclassif_amd import bulk, nbm_detect
    a, b = checkpoint / 'bulk', checkpoint / 'perfile'
    a.mkdir()
    for i in range(nbm_detect.BULK_MIN_FILES):
        synth.write_wav(str(a / f'clip{i}.wav'), synth.clip_pcm16(600 + i), 22050)
    synth.write_wav(str(a / 'rec.wav'), synth.clip_pcm16(640, int(22050 * 11.3)), 22050)
    shutil.copytree(str(a), str(b))
    n_windows = bulk.recording_windows(22050, int(22050 * 11.3))
    assert n_windows > 1
    monkeypatch.setattr(nbm_detect, 'RECORDINGS_MIN_WINDOWS', n_windows)
    seen = {'clips': [], 'recordings': []}
    real_files, real_rec = bulk.detect_files, bulk.detect_recordings

    def spy_files(model, files, **kw):
        out = real_files(model, files, **kw)
        seen['clips'].append(len(files))
        return out

    def spy_rec(model, files, **kw):
        out = real_rec(model, files, **kw)
        seen['recordings'].append((sorted(os.path.basename(f) for f in files), list(kw['stats']['rejected'])))
        return out

    monkeypatch.setattr(bulk, 'detect_files', spy_files)
    monkeypatch.setattr(bulk, 'detect_recordings', spy_rec)
    common = ['--ckpt', str(checkpoint / 'model_weights'), '--min_score', '0.05', '--batch', '4',
              '--bird_dict', str(checkpoint / 'bird_dict.json')]
    nbm_detect.main(common + ['--audio_dir', str(a), '--bulk_batch', '8'])
    assert seen == {'clips': [nbm_detect.BULK_MIN_FILES], 'recordings': [(['rec.wav'], [])]}
    nbm_detect.main(common + ['--audio_dir', str(b), '--no_bulk'])
    assert len(seen['clips']) == 1 and len(seen['recordings']) == 1
    names = sorted(p.name for p in a.glob('*.txt'))
    assert len(names) == nbm_detect.BULK_MIN_FILES + 1 and names == sorted(p.name for p in b.glob('*.txt'))
    n = 0
    for name in names:
        ta, tb = (a / name).read_text(), (b / name).read_text()
        assert ta == tb, name
        n += sum(len(v['scores']) for v in ast.literal_eval(ta).values())
    assert n > 0
