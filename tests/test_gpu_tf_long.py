"""GPU: the transformer head in the DETR flavour (`--tf_rcnn --tf_pe_qk`, 2 encoder layers) with more than 128 RoI slots per image --
the attention's long kernels (csrc/mha.hip) -- through every route: training forward and gradients against float64 autograd
(tests/tf_dropout_ref.py) with and without dropout, detection against the oracle at 153 / 160 RoIs per call, load_model / detect /
detect_calls at `--post_nms_topN_eval 200`, both captured bulk routes, the CLI against `--no_bulk`, and a training step at
`--rcnn_batch_size 160` with dropout, repeated, also under `ops.set_deterministic(True)`."""
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
from test_gpu_tf_dropout_head import CH, PRE, SEED, _checkpoint, head_weights, nhwc_tokens, rnd   # noqa: E402
from test_gpu_tf_segments import SCORE_TOL, _assert_same_rows, _kernel_only, _order_score_ties    # noqa: E402

B, NR, E = 2, 130, 512                          # 130 RoI slots: two key blocks, the second of two keys; the last query block of two rows
TF = dict(tf_rcnn=True, tf_pe_qk=True, tf_num_encoder_layers=2)
BUDGET = 200                                    # --post_nms_topN_eval of the route tests


def _rel(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape
    return float((got - ref).abs().max()) / (float(ref.abs().max()) + 1e-12)


def bounded(got, ref, f32, tol, name):
    """The project's bound, or 3 x the error of the float32 torch restatement of the same reference where that is larger."""
    err, e32 = _rel(got, ref), _rel(f32, ref)
    bound = max(tol, 3 * e32)
    print(f'{name}: relative error {err:.3e}; float32 torch {e32:.3e}; bound {bound:.3e}')
    assert err <= bound, f'{name}: {err:.3e} vs max({tol:.1e}, 3 x {e32:.3e})'


def _reference(dtype, cfg, pool, pe, r1, r2, masks, p):
    sdg = {k: v.clone().to(dtype).requires_grad_(True) for k, v in head_weights(True).items()}     # copies: the shared weights stay plain
    pool_ = pool.clone().to(dtype).requires_grad_(True)
    reg, cls = R.head_forward(sdg, cfg, pool_, pe.to(dtype), masks, p)
    ((reg * r1.to(dtype)).sum() + (cls * r2.to(dtype)).sum() * 50).backward()
    return reg.detach(), cls.detach(), pool_.grad, {k: v.grad for k, v in sdg.items()}


@pytest.mark.parametrize('p', [0.0, 0.1])
def test_head_training_forward_and_gradients_vs_float64_at_130_rois(p):
    """Bounds of tests/test_gpu_tf_dropout_head.py: 2e-5 outputs, 2e-4 input gradient, 3e-4 parameter gradients, relative to the
    largest reference value."""
    assert ops.mha_plan(NR, E // 8).family == 'long'
    pool = rnd('tflpool', B, NR, CH, 2, 2).abs()
    pe = rnd('tflpe', B, NR, CH, 2, 2)
    r1, r2 = rnd('tflr1', B * NR, 604), rnd('tflr2', B * NR, 151)
    cfg = O.make_cfg(**TF)
    masks = R.reference_masks(cfg, B, NR, E, p, SEED, 0) if p else R.ones_masks(cfg, B, NR, E)
    reg, cls, dpool, dsd = _reference(torch.float64, cfg, pool, pe, r1, r2, masks, p)
    reg32, cls32, dpool32, dsd32 = _reference(torch.float32, cfg, pool, pe, r1, r2, masks, p)

    head = Transformer_RCNN(default_args(device='cuda', dropout=p, **TF))
    head.load_state_dict({k[len(PRE):]: v for k, v in head_weights(True).items()})
    head = head.cuda().train()
    head.set_dropout_stream(SEED, 0)
    pd = nhwc_tokens(pool).requires_grad_(True)
    n = torch.full((1,), NR, dtype=torch.int32, device='cuda')
    greg, gcls = head.forward_nhwc(pd, nhwc_tokens(pe), B, NR, n)
    ((greg * r1.cuda()).sum() + (gcls * r2.cuda()).sum() * 50).backward()
    assert head.dropout_call == (1 if p else 0)
    bounded(greg, reg, reg32, 2e-5, 'reg'); bounded(gcls, cls, cls32, 2e-5, 'cls')
    bounded(pd.grad.view(B, NR, 2, 2, CH).permute(0, 1, 4, 2, 3), dpool, dpool32, 2e-4, 'dpool')
    for name, prm in head.named_parameters():
        bounded(prm.grad, dsd[PRE + name], dsd32[PRE + name], 3e-4, 'd' + name)


def test_head_outputs_and_input_gradient_repeat_bit_for_bit_in_the_default_mode():
    """B = 2, 160 RoIs, p = 0.1, the same dropout stream twice, `ops.deterministic()` off: the outputs and the gradient with respect to
    the pooled input -- which passes the attention backward of both layers, the LayerNorm and GEMM data gradients and no sum over token
    rows -- repeat bit for bit.  The parameter gradients are not compared here: in the default mode the weight gradients
    (`nbm_conv_wgrad`) and bias gradients (`nbm_colsum`) add their partial sums with float atomics, DESIGN 4t."""
    assert not ops.deterministic()
    nr = 160
    pool, pe = rnd('tflrpool', B, nr, CH, 2, 2).abs(), rnd('tflrpe', B, nr, CH, 2, 2)
    r1, r2 = rnd('tflrr1', B * nr, 604).cuda(), rnd('tflrr2', B * nr, 151).cuda()
    head = Transformer_RCNN(default_args(device='cuda', dropout=0.1, **TF))
    head.load_state_dict({k[len(PRE):]: v for k, v in head_weights(True).items()})
    head = head.cuda().train()
    n = torch.full((1,), nr, dtype=torch.int32, device='cuda')
    runs = []
    for _ in range(2):
        head.set_dropout_stream(SEED, 0)
        head.zero_grad()
        pd = nhwc_tokens(pool).requires_grad_(True)
        reg, cls = head.forward_nhwc(pd, nhwc_tokens(pe), B, nr, n)
        ((reg * r1).sum() + (cls * r2).sum() * 50).backward()
        runs.append((reg.detach().clone(), cls.detach().clone(), pd.grad.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert float(runs[0][2].abs().max()) > 0 and bool(torch.isfinite(runs[0][2]).all())


# ----------------------------------------------------------------------------------------------- detection
def _model(**kw):
    from birdsoundclassif_amd.nets import build_model
    m, _ = build_model(default_args(device='cuda', **TF, **kw))
    m.load_state_dict(filler_state_dict(**TF))
    return m.cuda().eval()


def test_detect_calls_vs_oracle_with_more_than_128_rois_per_call():
    """test_detect_calls_vs_oracle_one_call_per_segment of tests/test_gpu_tf_segments.py at a budget of 160 RoIs: the oracle keeps 153
    and 160 per call, so every image's attention runs over more than 128 keys.  Classes and boxes equal, scores within 1e-4, the
    order inside runs of oracle scores closer than that left open."""
    from birdsoundclassif_amd.nets.layers import FastRCNN
    budget = dict(pre_nms_topN_eval=400, post_nms_topN_eval=160, nms_thresh=0.5)
    layout, ms = [2, 1], 0.05
    m = _model(**budget)
    sd = filler_state_dict(**TF)
    cfg = O.make_cfg(**TF, **budget)
    x = torch.from_numpy(synth.image_batch(0, sum(layout)))[:, None]
    det, n_det = m.detect_calls(x.cuda(), ops.segment_table(layout), 0.3, ms)
    got = FastRCNN.dets_to_dicts(det, n_det, 150)
    s, roi_counts, with_dets = 0, [], 0
    for k in layout:
        with torch.no_grad():
            f = O.forward_first_stage(sd, cfg, x[s:s + k])
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
    print('oracle RoI counts per call', roi_counts, 'images with detections', with_dets)
    assert min(roi_counts) > ops.MHA_SMAX and with_dets == 3       # the short kernels could not have served either call


# ----------------------------------------------------------------------------------------------- routes
def test_load_model_takes_a_checkpoint_with_a_budget_of_200_rois(tmp_path):
    """`args` with post_nms_topN_eval = 200: detect runs, and detect_calls as one call per image is detect on each image."""
    from birdsoundclassif_amd.run_detection import load_model
    m, args = load_model(_checkpoint(tmp_path / 'r200', post_nms_topN_eval=BUDGET, **TF))
    assert args.post_nms_topN_eval == BUDGET and m.head.fast_rcnn.rcnn.tf_pe_qk and not m.training
    x = torch.from_numpy(synth.image_batch(0, 2))[:, None].cuda()
    det, n = (t.clone() for t in m.detect(x, 0.3, 0.05))
    assert int(n.sum()) > 0
    det, n = (t.clone() for t in m.detect_calls(x, ops.segment_table([1, 1]), 0.3, 0.05))
    for b in range(2):
        d1, n1 = m.detect(x[b:b + 1].contiguous(), 0.3, 0.05)
        _assert_same_rows(det, n, d1, n1, b, 'one call per image')


def test_both_captured_routes_replay_a_budget_of_200_rois():
    """test_both_captured_routes_replay_a_wide_head of tests/test_gpu_tf_head_dims.py at post_nms_topN_eval = 200: kernel-only graphs,
    replays that repeat themselves bit for bit and equal the eager detect_calls."""
    m = _model(post_nms_topN_eval=BUDGET)
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


def test_cli_takes_both_routes_at_200_rois_and_writes_the_per_file_drivers_bytes(tmp_path, monkeypatch):
    """The CLI test of tests/test_gpu_tf_head_dims.py on a small folder (one recording, four clips, one odd file) with a checkpoint whose
    `args` hold post_nms_topN_eval = 200: the txt files of the two bulk routes are those of `--no_bulk`, byte for byte."""
    from birdsoundclassif_amd import nbm_detect
    ck = _checkpoint(tmp_path / 'model_weights', post_nms_topN_eval=BUDGET, **TF)
    (tmp_path / 'bird_dict.json').write_text(json.dumps({f'Species {i}': i for i in range(1, 151)}))
    a, b = tmp_path / 'route', tmp_path / 'perfile'
    a.mkdir()
    monkeypatch.setattr(nbm_detect, 'BULK_MIN_FILES', 3)
    recordings = {'rec_a.wav': (13.4, 22050)}
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
    nbm_detect.main(common + ['--audio_dir', str(a), '--bulk_batch', '8'])
    assert seen == {'clips': 1, 'recordings': 1}
    nbm_detect.main(common + ['--audio_dir', str(b), '--no_bulk'])
    assert seen == {'clips': 1, 'recordings': 1}                                # --no_bulk took neither route
    names = sorted(p.name for p in a.glob('*.txt'))
    assert len(names) == len(recordings) + nbm_detect.BULK_MIN_FILES + 2 and names == sorted(p.name for p in b.glob('*.txt'))
    for name in names:
        assert (a / name).read_text() == (b / name).read_text(), name
    assert sum(len((a / name).read_text()) > 4 for name in names) > 0           # some file holds detections


# ----------------------------------------------------------------------------------------------- training
_BUILT = []


@pytest.fixture(autouse=True)
def _release_optimisers():
    import gc
    yield
    for opt in _BUILT:
        opt.release()
    _BUILT.clear()
    gc.collect()
    torch.cuda.empty_cache()


def _one_step(**kw):
    """One positive training step at B = 2 with the dropout stream (SEED, 0) -> (losses as floats, model, weights before the step)."""
    from birdsoundclassif_amd.nets import build_model
    args = default_args(device='cuda', **kw)
    model, crit = build_model(args)
    before = filler_state_dict(**TF)
    model.load_state_dict(before)
    model = model.cuda().train()
    crit.train()
    model.head.fast_rcnn.rcnn.set_dropout_stream(SEED, 0)
    opt, _ = build_optimizer(model, args)
    _BUILT.append(opt)
    bb, ids, lengths = synth.label_batch(0, 2)
    img = torch.from_numpy(synth.image_batch(0, 2))
    np.random.seed(4321)
    torch.manual_seed(77)
    loss = train_one_step(model, crit, opt, [img, img, bb, ids, lengths], args.clip_max_norm, 'cuda', negative_sample=False)
    torch.cuda.synchronize()
    return {k: float(v.detach() if torch.is_tensor(v) else v) for k, v in loss.items()}, model, before


def _same_step(a, b):
    (loss_a, model_a, _), (loss_b, model_b, _) = a, b
    assert loss_a == loss_b, (loss_a, loss_b)
    for (name, p), p2 in zip(model_a.head.fast_rcnn.rcnn.named_parameters(), model_b.head.fast_rcnn.rcnn.parameters()):
        assert torch.equal(p, p2), name


TRAIN = dict(rcnn_batch_size=160, dropout=0.1, **TF)


def test_train_step_at_160_rois_with_dropout_repeats_bit_for_bit():
    """`--tf_rcnn --tf_pe_qk --rcnn_batch_size 160 --dropout 0.1`: finite losses, every head parameter moves, and the step's losses
    repeat bit for bit under the same dropout stream.  The parameters after the step are compared in deterministic mode (below): in
    the default mode the bias gradients of the head's linear layers are float atomics over 80 workgroups at these 320 token rows
    (nbm_colsum), and `rois_embedding.0.bias` came out with other last bits in a second run -- with the attention's
    gradients equal, as the weight gradients beside it and tests/test_gpu_mha_long.py::test_long_kernels_repeat_bit_for_bit show."""
    kw = TRAIN
    first = _one_step(**kw)
    loss, model, before = first
    print(loss)
    assert 'sec_class_loss' in loss and all(np.isfinite(v) for v in loss.values())
    head = model.head.fast_rcnn.rcnn
    assert head.dropout_call == 1
    for name, p in head.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name
        assert not torch.equal(p.detach().cpu(), before[PRE + name]), name
    again = _one_step(**kw)
    assert again[0] == loss, (again[0], loss)


def test_train_step_at_160_rois_repeats_bit_for_bit_in_deterministic_mode():
    """`ops.set_deterministic(True)`: the losses and every head parameter after the step, bit for bit."""
    with ops.set_deterministic(True):
        det = _one_step(**TRAIN)
        _same_step(det, _one_step(**TRAIN))
    assert not ops.deterministic() and all(np.isfinite(v) for v in det[0].values())
