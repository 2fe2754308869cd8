"""GPU: the transformer head (`--tf_rcnn`) at head counts whose head dim exceeds 64 -- `--tf_nhead` 4, 2, 1 in the default flavour,
`--tf_pe_qk --tf_model_dim 1024 --tf_nhead 8` -- through every route: training forward and gradients against float64 autograd
(tests/tf_dropout_ref.py) with and without dropout, detection against the oracle, load_model / detect / detect_calls, both captured
bulk routes, the CLI against `--no_bulk`, and one training step."""
import json
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tf_dropout_ref as R                                                     # noqa: E402
from birdsoundclassif_amd import bulk, ops, synth                              # noqa: E402
from birdsoundclassif_amd.nets.layers import Transformer_RCNN                  # noqa: E402
from birdsoundclassif_amd.train import build_optimizer, default_args, train_one_step   # noqa: E402
from helpers import dets_to_rows, filler_state_dict                            # noqa: E402
from oracle import nets_ref as O                                               # noqa: E402
from test_gpu_tf_dropout_head import B, CH, NR, PRE, SEED, _checkpoint, close, inputs, nhwc_tokens, run_head   # noqa: E402
from test_gpu_tf_segments import RAGGED, SCORE_TOL, _assert_same_rows, _kernel_only, _order_score_ties  # noqa: E402

# the three configurations that used to be refused: head dims 128, 512 and 128
FLAVOURS = [dict(tf_pe_qk=False, tf_nhead=4), dict(tf_pe_qk=False, tf_nhead=1), dict(tf_pe_qk=True, tf_model_dim=1024, tf_nhead=8)]
_ids = lambda kw: '-'.join(f'{k}{v}' for k, v in kw.items())
_SD = {}
LAYOUT = [4, 1, 2]                              # the model calls of the detection test: 7 images keep the oracle's CPU first stage short


def head_weights(kw):
    key = (kw['tf_pe_qk'], kw.get('tf_model_dim', 512))         # nn.MultiheadAttention's parameters do not depend on the head count
    if key not in _SD:
        head = Transformer_RCNN(default_args(device='cpu', tf_rcnn=True, tf_num_encoder_layers=2, **kw))
        _SD[key] = synth.fill_state_dict({PRE + k: tuple(v.shape) for k, v in head.state_dict().items()})
    return _SD[key]


def make_head(kw, dropout):
    head = Transformer_RCNN(default_args(device='cuda', tf_rcnn=True, tf_num_encoder_layers=2, dropout=dropout, **kw))
    head.load_state_dict({k[len(PRE):]: v for k, v in head_weights(kw).items()})
    return head.cuda()


@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('kw', FLAVOURS, ids=_ids)
def test_head_training_forward_and_gradients_vs_float64(kw, p):
    """Geometry and bounds of tests/test_gpu_tf_dropout_head.py (B = 5, 16 RoIs, 2 encoder layers): 2e-5 outputs, 2e-4 input gradient,
    3e-4 parameter gradients, relative to the largest reference value; at p = 0 the evaluation-mode rows are the training-mode
    rows within 2e-5."""
    pool, pe, r1, r2 = inputs(kw['tf_pe_qk'])
    E = kw.get('tf_model_dim', 512)
    cfg = O.make_cfg(tf_rcnn=True, tf_num_encoder_layers=2, **kw)
    masks = R.reference_masks(cfg, B, NR, E, p, SEED, 0) if p else R.ones_masks(cfg, B, NR, E)
    sdg = {k: v.double().requires_grad_(True) for k, v in head_weights(kw).items()}
    pool64 = pool.double().requires_grad_(True)
    reg, cls = R.head_forward(sdg, cfg, pool64, pe.double(), masks, p)
    ((reg * r1.double()).sum() + (cls * r2.double()).sum() * 50).backward()

    head = make_head(kw, p).train()
    head.set_dropout_stream(SEED, 0)
    greg, gcls, gpool, grads = run_head(head, pool, pe, r1, r2)
    assert head.dropout_call == (1 if p else 0)
    close(greg, reg, 2e-5, 'reg'); close(gcls, cls, 2e-5, 'cls')
    close(gpool.view(B, NR, 2, 2, CH).permute(0, 1, 4, 2, 3), pool64.grad, 2e-4, 'dpool')
    for name, g in grads.items():
        close(g, sdg[PRE + name].grad, 3e-4, 'd' + name)
    if not p:
        with torch.no_grad():
            ereg, ecls, _, _ = run_head(head.eval(), pool, pe, r1, r2, grad=False)
        close(ereg, greg, 2e-5, 'eval reg vs training reg'); close(ecls, gcls, 2e-5, 'eval cls vs training cls')


# ----------------------------------------------------------------------------------------------- detection
def _model(**kw):
    from birdsoundclassif_amd.nets import build_model
    kw = dict(tf_rcnn=True, tf_num_encoder_layers=2, **kw)
    m, _ = build_model(default_args(device='cuda', **kw))
    m.load_state_dict(filler_state_dict(**kw))
    return m.cuda().eval()


_FIRST = {}


def _oracle_first_stage(sd, cfg, x):
    """The oracle's first stage per segment of LAYOUT, computed once: it does not read the head's weights."""
    shared = {k: v for k, v in sd.items() if not k.startswith(PRE)}
    if not _FIRST:
        s, out = 0, []
        for k in LAYOUT:
            with torch.no_grad():
                out.append(O.forward_first_stage(sd, cfg, x[s:s + k]))
            s += k
        _FIRST.update(weights=shared, out=out)
    assert shared.keys() == _FIRST['weights'].keys() and all(torch.equal(v, _FIRST['weights'][k]) for k, v in shared.items())
    return _FIRST['out']


@pytest.mark.parametrize('kw', [dict(tf_pe_qk=False, tf_nhead=4), dict(tf_pe_qk=True, tf_nhead=2)], ids=_ids)
def test_detect_calls_vs_oracle_one_call_per_segment(kw):
    """test_detect_calls_vs_oracle_one_call_per_segment of tests/test_gpu_tf_segments.py at head dims 128 and 256: classes and boxes
    equal, scores within 1e-4, the order inside runs of oracle scores closer than that left open."""
    from birdsoundclassif_amd.nets.layers import FastRCNN
    ms = 0.2
    kw = dict(tf_rcnn=True, tf_num_encoder_layers=2, **kw)
    m = _model(**{k: v for k, v in kw.items() if k not in ('tf_rcnn', 'tf_num_encoder_layers')}, **RAGGED)
    sd = filler_state_dict(**kw)
    cfg = O.make_cfg(**kw, **RAGGED)
    x = torch.from_numpy(synth.image_batch(0, sum(LAYOUT)))[:, None]
    det, n_det = m.detect_calls(x.cuda(), ops.segment_table(LAYOUT), 0.3, ms)
    got = FastRCNN.dets_to_dicts(det, n_det, 150)
    s, roi_counts, with_dets = 0, [], 0
    for k, f in zip(LAYOUT, _oracle_first_stage(sd, cfg, x)):
        with torch.no_grad():
            ref = dets_to_rows(O.forward_second_stage(sd, cfg, f['fpn_out'], f['rois'], 0.3, ms))
        roi_counts.append(f['rois'].shape[1])
        with_dets += len(set(ref[:, 0].tolist()))
        rows = dets_to_rows(got[s:s + k])
        assert rows.shape == ref.shape, (s, rows.shape, ref.shape)
        assert np.array_equal(rows[:, :2], ref[:, :2]), s
        rows, ref = _order_score_ties(rows, ref)
        assert np.array_equal(rows[:, :6], ref[:, :6]), s
        assert np.abs(rows[:, 6] - ref[:, 6]).max() < SCORE_TOL, s
        s += k
    print('oracle RoI counts per segment', roi_counts, 'images with detections', with_dets)
    assert len(set(roi_counts)) >= 2 and with_dets >= 3            # an all-empty or all-full batch would show nothing


# ----------------------------------------------------------------------------------------------- routes
def test_load_model_takes_a_checkpoint_with_4_heads(tmp_path):
    """`args` with tf_nhead = 4: load_model builds the head with it; detect_calls as one call per image is detect on each image."""
    from birdsoundclassif_amd.run_detection import load_model
    m, args = load_model(_checkpoint(tmp_path / 'nh4', tf_rcnn=True, tf_nhead=4, tf_num_encoder_layers=2))
    assert args.tf_nhead == 4 and m.head.fast_rcnn.rcnn.nhead == 4 and not m.training
    x = torch.from_numpy(synth.image_batch(0, 2))[:, None].cuda()
    det, n = (t.clone() for t in m.detect(x, 0.3, 0.05))
    assert int(n.sum()) > 0
    det, n = (t.clone() for t in m.detect_calls(x, ops.segment_table([1, 1]), 0.3, 0.05))
    for b in range(2):
        d1, n1 = m.detect(x[b:b + 1].contiguous(), 0.3, 0.05)
        _assert_same_rows(det, n, d1, n1, b, 'one call per image')


def test_both_captured_routes_replay_a_wide_head():
    """test_both_captured_routes_replay_this_head of tests/test_gpu_tf_segments.py on `--tf_pe_qk --tf_nhead 2` (hd = 256): kernel-only
    graphs, replays that repeat themselves bit for bit and equal the eager detect_calls."""
    m = _model(tf_pe_qk=True, tf_nhead=2)
    NB = 8
    clip = bulk.GraphedDetector(m, NB, 66150, 22050, min_score=0.05, independent=True, lanes=2)
    rec = bulk.RecordingDetector(m, 12, min_score=0.05)
    try:
        assert _kernel_only(clip.census) and _kernel_only(rec.census), (clip.census, rec.census)
        pcm = [torch.from_numpy(synth.clip_batch_pcm16(300 + NB * k, NB)).cuda() for k in range(2)]
        eager = []
        with ops.lane(9):
            for p_ in pcm:
                imgs, _ = clip.fe(p_, 22050)
                d, n = m.detect_calls(imgs[:, 0][:, None].contiguous(), ops.batch_segments(NB, 1), 0.3, 0.05)
                eager.append((d.clone(), n.clone()))
        torch.cuda.synchronize()
        runs = []
        for _ in range(2):
            with torch.cuda.stream(clip.stream):
                for k in range(2):
                    clip.pcms[k].copy_(pcm[k])
                clip.replay()
                runs.append([(clip.dets[k].clone(), clip.n_dets[k].clone()) for k in range(2)])
            clip.stream.synchronize()
        for k in range(2):
            assert torch.equal(runs[0][k][1], runs[1][k][1]) and torch.equal(runs[0][k][0], runs[1][k][0])
            _assert_same_rows(runs[0][k][0], runs[0][k][1], eager[k][0], eager[k][1], 0, f'clip lane {k}')
        assert sum(int(e[1].sum()) for e in eager) > 0

        fe = rec.fe
        db, mm, Ls = fe.spectrogram_db(torch.from_numpy(synth.clip_pcm16(700, 22050 * 25))[None].cuda(), 22050)
        n_img, cols = fe.last_window_columns(Ls)
        assert n_img == 10
        rows = [ops.window_entry(db[0], mm[0], cols, w, n_img) for w in range(n_img)]
        rows += [np.zeros(ops.WINDOW_ENTRY_WORDS, np.int64)] * 2
        sizes = [4, 4, 2, 1, 1]
        table = torch.from_numpy(np.stack(rows)).cuda()
        with ops.lane(9):
            imgs = ops.spec_windows_table(table, fe.H_PIX, fe.W_PIX, fe.HOP_SPECTRO)
            d, n = m.detect_calls(imgs[:, None], ops.segment_table(sizes), 0.3, 0.05)
            d, n = d.clone(), n.clone()
        torch.cuda.synchronize()
        outs = []
        with torch.cuda.stream(rec.stream):
            rec.table.copy_(table)
            rec.seg.copy_(ops.segment_table(sizes, 'cpu'))
            for _ in range(2):
                rec.replay()
                outs.append((rec.det.clone(), rec.n_det.clone()))
        rec.stream.synchronize()
        assert torch.equal(outs[0][1], outs[1][1]) and int(outs[0][1][:10].sum()) > 0
        _assert_same_rows(outs[0][0], outs[0][1], outs[1][0], outs[1][1], 0, 'recording replays')
        _assert_same_rows(outs[0][0], outs[0][1], d, n, 0, 'recording replay vs eager')
    finally:
        clip.close()
        rec.close()


def test_cli_takes_both_routes_with_4_heads_and_writes_the_per_file_drivers_bytes(tmp_path, monkeypatch):
    """test_cli_takes_both_routes_and_writes_the_per_file_drivers_bytes of tests/test_gpu_tf_segments.py at `--batch 4` on a default-
    flavour checkpoint whose `args` hold tf_nhead = 4: the txt files of the two bulk routes are those of `--no_bulk`, byte for byte."""
    from birdsoundclassif_amd import nbm_detect
    ck = _checkpoint(tmp_path / 'model_weights', tf_rcnn=True, tf_nhead=4, tf_num_encoder_layers=2)
    (tmp_path / 'bird_dict.json').write_text(json.dumps({f'Species {i}': i for i in range(1, 151)}))
    a, b = tmp_path / 'route', tmp_path / 'perfile'
    a.mkdir()
    recordings = {'rec_a.wav': (31.7, 22050), 'rec_b.wav': (9.1, 44100), 'rec_c.wav': (64.2, 22050)}
    for i, (name, (sec, sr)) in enumerate(sorted(recordings.items())):
        synth.write_wav(str(a / name), synth.clip_pcm16(900 + i, int(sr * sec), sr), sr)
    for i in range(nbm_detect.BULK_MIN_FILES + 1):                              # equal 3 s clips: the clip route
        synth.write_wav(str(a / f'clip{i}.wav'), synth.clip_pcm16(930 + i), 22050)
    synth.write_wav(str(a / 'odd.wav'), synth.clip_pcm16(950, int(22050 * 2.1)), 22050)   # alone in its group: recording route
    shutil.copytree(str(a), str(b))
    n_windows = sum(bulk.recording_windows(sr, int(sr * sec)) for sec, sr in recordings.values()) + 1
    monkeypatch.setattr(nbm_detect, 'RECORDINGS_MIN_WINDOWS', n_windows)        # the folder is just large enough for the route
    seen = {'clips': 0, 'recordings': 0}
    real_files, real_rec = bulk.detect_files, bulk.detect_recordings

    def spy_files(model, files, **kw_):
        out = real_files(model, files, **kw_)
        seen['clips'] += 1
        return out

    def spy_rec(model, files, **kw_):
        out = real_rec(model, files, **kw_)
        assert kw_['stats']['rejected'] == [] and kw_['stats']['windows'] == n_windows
        seen['recordings'] += 1
        return out

    monkeypatch.setattr(bulk, 'detect_files', spy_files)
    monkeypatch.setattr(bulk, 'detect_recordings', spy_rec)
    common = ['--ckpt', ck, '--min_score', '0.05', '--batch', '4', '--bird_dict', str(tmp_path / 'bird_dict.json')]
    nbm_detect.main(common + ['--audio_dir', str(a), '--bulk_batch', '16'])
    assert seen == {'clips': 1, 'recordings': 1}
    nbm_detect.main(common + ['--audio_dir', str(b), '--no_bulk'])
    assert seen == {'clips': 1, 'recordings': 1}                                # --no_bulk took neither route
    names = sorted(p.name for p in a.glob('*.txt'))
    assert len(names) == len(recordings) + nbm_detect.BULK_MIN_FILES + 2 and names == sorted(p.name for p in b.glob('*.txt'))
    for name in names:
        assert (a / name).read_text() == (b / name).read_text(), name
    assert sum(len((a / name).read_text()) > 4 for name in names) > 0           # some file holds detections


# ----------------------------------------------------------------------------------------------- training
def _one_step(**kw):
    """One positive training step at B = 2 with the dropout stream (SEED, 0) -> (losses as floats, model, weights before the step)."""
    from birdsoundclassif_amd.nets import build_model
    args = default_args(device='cuda', **kw)
    model, crit = build_model(args)
    before = filler_state_dict(**{k: v for k, v in kw.items() if k != 'dropout'})
    model.load_state_dict(before)
    model = model.cuda().train()
    crit.train()
    model.head.fast_rcnn.rcnn.set_dropout_stream(SEED, 0)
    opt, _ = build_optimizer(model, args)
    bb, ids, lengths = synth.label_batch(0, 2)
    img = torch.from_numpy(synth.image_batch(0, 2))
    np.random.seed(4321)
    torch.manual_seed(77)
    loss = train_one_step(model, crit, opt, [img, img, bb, ids, lengths], args.clip_max_norm, 'cuda', negative_sample=False)
    return {k: float(v.detach() if torch.is_tensor(v) else v) for k, v in loss.items()}, model, before


@pytest.mark.parametrize('kw', [dict(tf_nhead=4), dict(tf_pe_qk=True, tf_nhead=2, dropout=0.1)], ids=_ids)
def test_train_step_with_a_wide_head(kw):
    """`--tf_rcnn --tf_nhead 4` and `--tf_rcnn --tf_pe_qk --tf_nhead 2 --dropout 0.1`: finite losses, every head parameter moves, and
    the dropout step repeats bit for bit under the same dropout stream."""
    kw = dict(tf_rcnn=True, tf_num_encoder_layers=2, **kw)
    loss, model, before = _one_step(**kw)
    print(loss)
    assert 'sec_class_loss' in loss and all(np.isfinite(v) for v in loss.values())
    head = model.head.fast_rcnn.rcnn
    assert head.dropout_call == (1 if kw.get('dropout') else 0)
    for name, p in head.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name
        assert not torch.equal(p.detach().cpu(), before[PRE + name]), name
    if kw.get('dropout'):           # this path sums the LayerNorm parameter gradients in a fixed order: the whole step repeats
        again, model2, _ = _one_step(**kw)
        assert again == loss
        for (name, p), p2 in zip(head.named_parameters(), model2.head.fast_rcnn.rcnn.parameters()):
            assert torch.equal(p, p2), name
