"""GPU, model level: a checkpoint with `--roi_pool_h 3 --roi_pool_w 4` through every route -- the second stage (both heads,
forward and gradients) and `detect` against the CPU oracle, one positive and one negative training step, and the CLI with
and without the captured bulk routes.  B = 2, real geometry."""
import ast
import json
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from birdsoundclassif_amd import synth                                        # noqa: E402
from birdsoundclassif_amd.nets import functional as Fn                        # noqa: E402
from helpers import dets_to_rows, filler_state_dict                           # noqa: E402
from oracle import nets_ref as O                                              # noqa: E402

PH, PW = 3, 4
POOL = dict(roi_pool_h=PH, roi_pool_w=PW)
B, R_HEAD = 2, 16
# chosen on the CPU: the oracle returns MIN_ROWS detections or more on image_batch(0, 2) at this score
MIN_SCORE, MIN_ROWS = 0.05, 10


def rnd(key, *shape):
    return torch.from_numpy(synth.normal(key, int(np.prod(shape))).astype(np.float32).reshape(shape))


def close(got, ref, tol, name):
    got, ref = got.detach().cpu().float(), ref.detach().cpu().float()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = float(ref.abs().max()) + 1e-12
    err = float((got - ref).abs().max())
    print(f'{name}: max err {err:.3e} vs scale {scale:.3e}')
    assert err <= tol * scale, f'{name}: max err {err:.3e} vs scale {scale:.3e}'


def build(train=False, **kw):
    from birdsoundclassif_amd.nets import build_model
    from birdsoundclassif_amd.train import default_args
    args = default_args(device='cuda', **POOL, **kw)
    model, crit = build_model(args)
    model.load_state_dict(filler_state_dict(0, **POOL, **kw))
    model = model.cuda()
    return (model.train() if train else model.eval()), crit, args


@pytest.fixture(scope='module')
def first_stage():
    """The oracle's first stage on two images, once: (state dict, cfg, images, its output).  Never modified."""
    sd = filler_state_dict(0, **POOL)
    cfg = O.make_cfg(**POOL)
    x = torch.from_numpy(synth.image_batch(0, B))[:, None]
    with torch.no_grad():
        ref = O.forward_first_stage(sd, cfg, x)
    return sd, cfg, x, ref


@pytest.fixture(scope='module')
def model():
    return build()[0]


def _spread_rois(cfg, ref):
    """R_HEAD of the oracle's proposals per image, taken level by level in turn so that every pyramid level the proposals
    reach has RoIs (the first R_HEAD by score sit on the two finest levels)."""
    prop = ref['rois']
    lvl = O.roi_geometry(cfg, prop, [f.shape[-2] for f in ref['fpn_out']], [f.shape[-1] for f in ref['fpn_out']])[0]
    out = []
    for b in range(prop.shape[0]):
        by_level = [[i for i in range(prop.shape[1]) if int(lvl[b, i]) == l] for l in range(len(ref['fpn_out']))]
        order = [q[k] for k in range(prop.shape[1]) for q in by_level if k < len(q)]
        out.append(prop[b, order[:R_HEAD]])
    return torch.stack(out).contiguous()


def _second_stage_pair(run_device, sd_head, cfg, ref, names, tag):
    """Oracle second stage (training form) + autograd on the oracle's FPN maps and R_HEAD of its RoIs per image, then the
    device through `run_device(fpn NCHW-shaped list, rois)`; compares outputs, the gradients of `names` and of the maps
    (a level without a RoI: no gradient in the oracle, an all-zero map on the device)."""
    rois = _spread_rois(cfg, ref)
    fm =[f.detach().clone().requires_grad_(True) for f in ref['fpn_out']]
    sdg = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and '.running_' not in k else v)
           for k, v in sd_head.items() if k.startswith('head.fast_rcnn.')}
    o = O.forward_second_stage(sdg, cfg, fm, rois, training=True, new_buffers={})
    r1, r2 = rnd(('e2e_r1', tag), *o['bbox_reg'].shape), rnd(('e2e_r2', tag), *o['bbox_classes'].shape)
    ((o['bbox_reg'] * r1).sum() + (o['bbox_classes'] * r2).sum() * 50).backward()
    fd = [f.detach().permute(0, 2, 3, 1).contiguous().cuda().requires_grad_(True) for f in fm]
    try:
        got, params = run_device([f.permute(0, 3, 1, 2) for f in fd], rois.cuda())
        err_r = float((got['bbox_reg'].detach().cpu() - o['bbox_reg'].detach()).abs().max())
        err_c = float((got['bbox_classes'].detach().cpu() - o['bbox_classes'].detach()).abs().max())
        print(f'{tag}: bbox_reg max err {err_r:.3e}, bbox_classes max err {err_c:.3e}')
        assert err_r <= 1e-4 and err_c <= 1e-4, (tag, err_r, err_c)
        ((got['bbox_reg'] * r1.cuda()).sum() + (got['bbox_classes'] * r2.cuda()).sum() * 50).backward()
    finally:
        Fn._GRAD_ACC.clear()
    for name in names:
        close(params[name].grad, sdg['head.fast_rcnn.' + name].grad, 3e-4, f'{tag} d{name}')
    for i, f in enumerate(fd):
        ref_g = fm[i].grad if fm[i].grad is not None else torch.zeros_like(fm[i])
        close(f.grad.permute(0, 3, 1, 2), ref_g, 2e-4, f'{tag} dfpn{i}')


def test_second_stage_conv_head_and_gradients_vs_oracle(first_stage):
    """`model.forward_second_stage(training=True)` against the oracle: outputs within 1e-4 (the 2 x 2 head test's bound),
    gradients at the tolerances of test_transformer_rcnn_head_gradients_vs_oracle (3e-4 parameters, 2e-4 inputs)."""
    sd, cfg, _, ref = first_stage
    m = build(train=True)[0]

    def run(fpn, rois):
        out = m.forward_second_stage(fpn, rois, training=True)
        return out, {k[len('head.fast_rcnn.'):]: p for k, p in m.named_parameters() if k.startswith('head.fast_rcnn.')}

    _second_stage_pair(run, sd, cfg, ref, ['rcnn.bbox_reg_layer.weight', 'rcnn.rcnn.0.depth_wise.weight', 'rcnn.pe_proj.weight'], 'conv')


@pytest.mark.parametrize('pe_qk', [False, True], ids=['std', 'peqk'])
def test_second_stage_transformer_head_and_gradients_vs_oracle(first_stage, pe_qk):
    """The same for `--tf_rcnn`, both encoder flavours (two encoder layers, as the 2 x 2 gradient test): the head module
    `FastRCNN` -- what `forward_second_stage` calls -- on the same maps and RoIs."""
    from birdsoundclassif_amd.nets.layers import FastRCNN
    from birdsoundclassif_amd.train import default_args
    _, _, _, ref = first_stage
    kw = dict(tf_rcnn=True, tf_pe_qk=pe_qk, tf_num_encoder_layers=2)
    head = FastRCNN(default_args(device='cuda', **POOL, **kw))
    pre = 'head.fast_rcnn.'
    sd = synth.fill_state_dict({pre + k: tuple(v.shape) for k, v in head.state_dict().items()})
    head.load_state_dict({k[len(pre):]: v for k, v in sd.items()})
    head = head.cuda().train()
    assert sd[pre + 'rcnn.rois_embedding.0.weight'].shape == (512, 256 * PH * PW)

    def run(fpn, rois):
        reg, cls = head(fpn, rois, training=True)
        return {'bbox_reg': reg, 'bbox_classes': cls}, dict(head.named_parameters())

    _second_stage_pair(run, sd, O.make_cfg(**POOL, **kw), ref,
                       ['rcnn.bbox_reg_layer.weight', 'rcnn.rois_embedding.0.weight', 'rcnn.pos_embedding.0.weight'], f'tf{int(pe_qk)}')


def test_detect_vs_oracle(first_stage, model):
    sd, cfg, x, ref = first_stage
    with torch.no_grad():
        ref_d = O.forward_second_stage(sd, cfg, ref['fpn_out'], ref['rois'], 0.3, MIN_SCORE)
        got1 = model.forward_first_stage(x.cuda())
        got_d = model(x.cuda(), min_score=MIN_SCORE)
    assert torch.equal(got1['rois'].cpu(), ref['rois'])
    r, q = dets_to_rows(ref_d), dets_to_rows(got_d)
    assert len(r) >= MIN_ROWS, len(r)
    assert r.shape == q.shape and np.array_equal(r[:, :6], q[:, :6])
    assert np.abs(r[:, 6] - q[:, 6]).max() <= 1e-4


def test_one_positive_and_one_negative_training_step():
    from birdsoundclassif_amd.train import build_optimizer, train_one_step
    m, crit, args = build(train=True)
    crit.train()
    opt, _ = build_optimizer(m, args)
    img = torch.from_numpy(synth.image_batch(0, B))
    neg_img = torch.from_numpy(synth.image_batch(100, B))
    bb, ids, lengths = synth.label_batch(0, B)
    np.random.seed(1234)
    for neg in (False, True):
        loss = train_one_step(m, crit, opt, [img, neg_img, bb, ids, lengths], args.clip_max_norm, 'cuda', negative_sample=neg)
        assert loss and all(np.isfinite(float(v)) for v in loss.values()), loss
        assert any(k.startswith('sec_') for k in loss), sorted(loss)          # the second stage ran
        missing = [n for n, p in m.named_parameters() if p.requires_grad and (p.grad is None or not bool(torch.isfinite(p.grad).all()))]
        assert not missing, (neg, missing[:5])
    assert not Fn._PARKED


def test_cli_routes_write_identical_files_and_the_captured_step_is_kernel_only(tmp_path, model):
    """The recipe of test_gpu_detect_cli.py with a (3, 4) checkpoint directory: 8 one-window clips (captured clip route) and a
    three-window file (captured recordings route) with --bulk_batch 8, against --no_bulk (per-file driver)."""
    from birdsoundclassif_amd import bulk, nbm_detect
    ck = tmp_path / 'model_weights'
    ck.mkdir()
    cfg = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in vars(model.args).items() if k not in ('scales',)}
    assert cfg['roi_pool_h'] == PH and cfg['roi_pool_w'] == PW
    (ck / 'args').write_text(json.dumps(cfg))
    torch.save({'checkpoints': filler_state_dict(0, **POOL), 'steps': 0, 'epoch': 0, 'best_val_cls_loss': 99}, str(ck / 'model_chkpt.pt'))
    (tmp_path / 'bird_dict.json').write_text(json.dumps({f'Species {i}': i for i in range(1, 151)}))
    a, b = tmp_path / 'bulk', tmp_path / 'perfile'
    a.mkdir()
    for i in range(8):
        synth.write_wav(str(a / f'clip{i}.wav'), synth.clip_pcm16(400 + i), 22050)
    synth.write_wav(str(a / 'long.wav'), np.concatenate([synth.clip_pcm16(430), synth.clip_pcm16(431), synth.clip_pcm16(432)]), 22050)
    shutil.copytree(str(a), str(b))
    common = ['--ckpt', str(ck), '--min_score', '0.05', '--batch', '4', '--bird_dict', str(tmp_path / 'bird_dict.json')]
    nbm_detect.main(common + ['--audio_dir', str(a), '--bulk_batch', '8'])
    nbm_detect.main(common + ['--audio_dir', str(b), '--no_bulk'])
    names = sorted(p.name for p in a.glob('*.txt'))
    assert len(names) == 9 and names == sorted(p.name for p in b.glob('*.txt'))
    n = 0
    for name in names:
        ta, tb = (a / name).read_text(), (b / name).read_text()
        assert ta == tb, name
        n += sum(len(v['scores']) for v in ast.literal_eval(ta).values())
    assert n > 0
    det = bulk.GraphedDetector(model, 2, 66150, 22050, min_score=0.05)
    try:
        c = det.census
        assert c['memset'] == c['memcpy'] == c['host'] == c['other'] == 0 and c['kernel'] > 100, c
    finally:
        det.close()
