"""GPU: the per-file driver (reference run_detection.py / nbm_detect.py): merge_images against the golden fixture from
the real reference, and BASELINE.json configs[0] -- nbm_detect on 8 synthetic 3 s 22.05 kHz wav files with a checkpoint
directory in the reference layout -- against the oracle pipeline."""
import ast
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from birdsoundclassif_amd import synth                                       # noqa: E402
from helpers import filler_state_dict, load_golden                            # noqa: E402
from oracle import frontend_ref as FR, nets_ref as O                          # noqa: E402


def _merge_windows():
    wins = []
    for i in range(4):                              # same synthetic windows as oracle/make_golden.py
        u = synth.uniform(('merge', i), 64)
        d = {str(c): dict(bbox_coord=torch.Tensor(), scores=torch.Tensor()) for c in range(1, 151)}
        for j in range(6):
            c = 1 + int(u[8 * j] * 5)
            x1 = float(np.floor(u[8 * j + 1] * 1000)); w = float(np.floor(10 + u[8 * j + 2] * 300))
            y1 = float(np.floor(u[8 * j + 3] * 300)); h = float(np.floor(10 + u[8 * j + 4] * 60))
            if j == 0:
                x1 = 0.0
            if j == 1:
                x1 = 1023.0 - w
            box = torch.tensor([[x1, y1, min(x1 + w, 1023.0), min(y1 + h, 374.0)]])
            sc = torch.tensor([[float(u[8 * j + 5])]])
            e = d[str(c)]
            d[str(c)] = dict(bbox_coord=box, scores=sc) if len(e['bbox_coord']) == 0 else \
                dict(bbox_coord=torch.cat([e['bbox_coord'], box]), scores=torch.cat([e['scores'], sc], 1))
        wins.append(d)
    return wins


def test_merge_images_vs_reference_golden():
    from birdsoundclassif_amd.run_detection import merge_images
    g = load_golden('merge.npz')
    wins = _merge_windows()
    fp = type('FP', (), dict(W_PIX=1024, HOP_SPECTRO=819, spectrogram_length=819 * 3 + 700))()
    merged = merge_images(fp, [wins[:2], wins[2:]], 150)
    rows = []
    for k, v in merged.items():
        for i in range(len(v['bbox_coord'])):
            rows.append([int(k), *v['bbox_coord'][i].tolist(), float(v['scores'][i])])
    rows = np.array(rows).reshape(-1, 6)
    assert rows.shape == g['merged'].shape and np.allclose(rows, g['merged'], atol=1e-7)


def test_nbm_detect_cli_on_8_wavs(tmp_path):
    from birdsoundclassif_amd import nbm_detect
    from birdsoundclassif_amd.train import default_args
    ck = tmp_path / 'model_weights'
    ck.mkdir()
    args = default_args(device='cuda')
    cfg = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in vars(args).items() if k not in ('scales',)}
    (ck / 'args').write_text(json.dumps(cfg))
    sd = filler_state_dict()
    torch.save({'checkpoints': sd, 'steps': 0, 'epoch': 0, 'best_val_cls_loss': 99}, str(ck / 'model_chkpt.pt'))
    names = {f'Species {i}': i for i in range(1, 151)}
    (tmp_path / 'bird_dict.json').write_text(json.dumps(names))
    audio = tmp_path / 'audio'
    audio.mkdir()
    for i in range(8):
        synth.write_wav(str(audio / f'clip{i}.wav'), synth.clip_pcm16(200 + i), 22050)
    nbm_detect.main(['--ckpt', str(ck), '--audio_dir', str(audio), '--min_score', '0.05', '--batch', '4',
                     '--bird_dict', str(tmp_path / 'bird_dict.json')])
    outs = sorted(audio.glob('*.txt'))
    assert len(outs) == 8
    ocfg = O.make_cfg()
    n_total = 0
    for i in range(8):
        got = ast.literal_eval((audio / f'clip{i}.txt').read_text())
        n_total += sum(len(v['scores']) for v in got.values())
        if i >= 2:
            continue                                                   # oracle check on the first two files (CPU time)
        imgs, meta = FR.process_file(str(audio / f'clip{i}.wav'))
        with torch.no_grad():
            dets = O.forward(sd, ocfg, torch.from_numpy(np.stack(imgs))[:, None], min_score=0.05)
        ref = O.merge_images(meta['W_PIX'], meta['HOP_SPECTRO'], meta['spectrogram_length'], dets, 150)
        ref = {f'Species {j}': v for j, v in ((int(k), v) for k, v in ref.items()) if len(v['bbox_coord']) > 0}
        assert set(got) == set(ref), (i, sorted(got), sorted(ref))
        for k in ref:
            assert np.array_equal(np.array(got[k]['bbox_coord']), ref[k]['bbox_coord'].numpy()), (i, k)
            assert np.allclose(np.array(got[k]['scores']), ref[k]['scores'].numpy(), atol=2e-4)
    assert n_total > 0


def test_cli_bulk_route_writes_the_same_files_as_the_per_file_driver(tmp_path):
    """nbm_detect routes equal-length single-window clips through the pipelined hipGraph loop (bulk.detect_files, every clip an
    independent batch of one) and everything else through the per-file driver: the txt files are byte-identical to a run with
    --no_bulk (per-file driver for every file = the reference's loop, nbm_detect.py:24-28)."""
    import shutil
    from birdsoundclassif_amd import bulk, nbm_detect
    from birdsoundclassif_amd.train import default_args
    ck = tmp_path / 'model_weights'
    ck.mkdir()
    args = default_args(device='cuda')
    cfg = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in vars(args).items() if k not in ('scales',)}
    (ck / 'args').write_text(json.dumps(cfg))
    torch.save({'checkpoints': filler_state_dict(), 'steps': 0, 'epoch': 0, 'best_val_cls_loss': 99}, str(ck / 'model_chkpt.pt'))
    (tmp_path / 'bird_dict.json').write_text(json.dumps({f'Species {i}': i for i in range(1, 151)}))
    a, b = tmp_path / 'bulk', tmp_path / 'perfile'
    a.mkdir()
    for i in range(11):                              # 11 clips: a full batch of 8 + a padded one
        synth.write_wav(str(a / f'clip{i:02d}.wav'), synth.clip_pcm16(400 + i), 22050)
    synth.write_wav(str(a / 'quiet.wav'), (synth.clip_pcm16(420) // 64).astype(np.int16), 22050)    # same length, low level
    long = np.concatenate([synth.clip_pcm16(430), synth.clip_pcm16(431)])
    synth.write_wav(str(a / 'long.wav'), long, 22050)                                               # two windows: per-file route
    synth.write_wav(str(a / 'short.wav'), synth.clip_pcm16(432)[:40000], 22050)                     # other length: alone in its group
    shutil.copytree(str(a), str(b))
    infos = list(bulk.probe_files(sorted(str(p) for p in a.glob('*.wav'))).values())
    groups, rest = dict(bulk.clip_groups(infos)), [i.path for i in infos if not (i.clip and i.int16_route)]
    assert sorted(len(v) for v in groups.values()) == [1, 12] and [os.path.basename(f) for f in rest] == ['long.wav']
    common = ['--ckpt', str(ck), '--min_score', '0.05', '--batch', '4', '--bird_dict', str(tmp_path / 'bird_dict.json')]
    nbm_detect.main(common + ['--audio_dir', str(a), '--bulk_batch', '8'])
    nbm_detect.main(common + ['--audio_dir', str(b), '--no_bulk'])
    names = sorted(p.name for p in a.glob('*.txt'))
    assert len(names) == 14 and names == sorted(p.name for p in b.glob('*.txt'))
    n = 0
    for name in names:
        ta, tb = (a / name).read_text(), (b / name).read_text()
        assert ta == tb, name
        n += sum(len(v['scores']) for v in ast.literal_eval(ta).values())
    assert n > 0


def test_graphed_bulk_detection_matches_per_file_driver(tmp_path):
    """configs[4] in miniature: hipGraph-captured detect loop over a wav shard == the per-file run_detection driver."""
    from birdsoundclassif_amd import bulk
    from birdsoundclassif_amd.nets import build_model
    from birdsoundclassif_amd.run_detection import run_detection
    from birdsoundclassif_amd.train import default_args
    model, _ = build_model(default_args(device='cuda'))
    model.load_state_dict(filler_state_dict())
    model = model.cuda().eval()
    names = {f'Species {i}': i for i in range(1, 151)}
    (tmp_path / 'bird_dict.json').write_text(json.dumps(names))
    files = []
    for i in range(6):
        p = str(tmp_path / f'c{i}.wav')
        synth.write_wav(p, synth.clip_pcm16(300 + i), 22050)
        files.append(p)
    got = bulk.detect_files(model, files, batch=4, min_score=0.05, bird_dict=names, write_txt=False)
    assert len(got) == 6
    n = 0
    for f, g in zip(files, got):
        ref = run_detection(model, model.args, f, str(tmp_path / 'bird_dict.json'), min_score=0.05, bs=4)
        assert set(ref) == set(g)
        for k in ref:
            assert ref[k]['bbox_coord'] == g[k]['bbox_coord']
            assert np.allclose(np.array(ref[k]['scores']).reshape(-1), np.array(g[k]['scores']).reshape(-1), atol=0)
            n += len(g[k]['scores'])
    assert n > 0
    # graph replay is bit-reproducible
    det = bulk.GraphedDetector(model, 4, 66150, 22050, min_score=0.05)
    pcm = torch.from_numpy(synth.clip_batch_pcm16(300, 4))
    det.pcm.copy_(pcm)
    det.replay(); torch.cuda.synchronize()
    a = det.det.clone(), det.n_det.clone()
    det.replay(); torch.cuda.synchronize()
    assert torch.equal(a[0], det.det) and torch.equal(a[1], det.n_det)


def test_two_lanes_in_flight_give_the_single_lane_results(tmp_path):
    """`detect_files(lanes=2)`: batches go through ONE captured graph in pairs -- its capture forks into two parallel detect steps on two
    streams, each with its own static input / outputs and its own persistent scratch and tile-list buffers (ops.lane).  The results
    must be those of the one-lane loop, file by file, bit for bit -- a buffer shared between the lanes would show up as corrupted
    detections here -- also for an odd number of batches (the second lane idles in the last replay)."""
    from birdsoundclassif_amd import bulk, ops
    from birdsoundclassif_amd.nets import build_model
    from birdsoundclassif_amd.train import default_args
    model, _ = build_model(default_args(device='cuda'))
    model.load_state_dict(filler_state_dict())
    model = model.cuda().eval()
    files = []
    for i in range(44):                               # 11 batches of 4: an odd number, the lanes' batches differ in content
        p = str(tmp_path / f'c{i}.wav')
        synth.write_wav(p, synth.clip_pcm16(400 + i % 13), 22050)
        files.append(p)
    one = bulk.detect_files(model, files, batch=4, min_score=0.05, write_txt=False, lanes=1)
    stats = {}
    two = bulk.detect_files(model, files, batch=4, min_score=0.05, write_txt=False, lanes=2, stats=stats)
    assert stats['lanes'] == 2 and len(one) == len(two) == 44
    assert sum(len(v['scores']) for r in one for v in r.values()) > 0
    assert one == two
    # detect_files closed the detector it had built: the second lane's scratch went back to the allocator
    assert {k[1] for k in ops._WINO_SCRATCH if isinstance(k, tuple)} == {0}
    # direct: different inputs in the two lanes, the FIRST replay after the capture and six more against the eager step.  The eager
    # references are computed BEFORE the detector exists, and between the capture and the first replay there is nothing but the
    # device-to-device copy of the inputs (an eager step in between used to hide the failure this test is cited for)
    import gc
    gc.collect()
    pcm = [torch.from_numpy(synth.clip_batch_pcm16(300 + 4 * k, 4)).cuda() for k in range(2)]
    ref = _eager_refs(model, pcm)
    det = bulk.GraphedDetector(model, 4, 66150, 22050, min_score=0.05, lanes=2)
    assert det.census['memset'] == det.census['memcpy'] == 0 and det.census['kernel'] > 300
    # the lanes own different scratch buffers, and the detector holds them as captured
    keys = [k for k in ops._WINO_SCRATCH if isinstance(k, tuple)]
    assert {k[1] for k in keys} >= {0, 1}
    assert len({ops._WINO_SCRATCH[k].data_ptr() for k in keys}) == len(keys)
    assert {ops._WINO_SCRATCH[k].data_ptr() for k in keys if k[1] in det.lane_ids} <= {t.data_ptr() for t in det._held}
    for k in range(2):
        det.pcms[k].copy_(pcm[k])
    for rep in range(7):
        with torch.cuda.stream(det.stream):
            det.replay()
        torch.cuda.synchronize()
        for k in range(2):
            assert torch.equal(ref[k][0], det.dets[k]) and torch.equal(ref[k][1], det.n_dets[k]), (rep, k)
    assert int(ref[0][1].sum()) > 0 and not torch.equal(ref[0][0], ref[1][0])


def _eager_refs(model, pcms, independent=False):
    from birdsoundclassif_amd import ops
    from birdsoundclassif_amd.nbm_datasets.prepare_dataset import SpectrogramFrontEnd
    fe, ref = SpectrogramFrontEnd('cuda'), []
    with torch.no_grad(), ops.lane(9):
        for p_ in pcms:
            imgs, _ = fe(p_, 22050)
            d, n = model.detect(imgs[:, 0][:, None].contiguous(), 0.3, 0.05, independent=independent)
            ref.append((d.clone(), n.clone()))
    torch.cuda.synchronize()
    return ref


def _model():
    from birdsoundclassif_amd.nets import build_model
    from birdsoundclassif_amd.train import default_args
    model, _ = build_model(default_args(device='cuda'))
    model.load_state_dict(filler_state_dict())
    return model.cuda().eval()


def test_several_graph_execs_alive_at_once_replay_correctly():
    """DESIGN 4d, round 5.  Round 4: with two captured detect steps alive in one process one of them returned garbage (B = 64: 0
    detections) or faulted (B = 4).  Cause (scripts/graph_pair_repro.hip, profiles/r05_graph_pair.txt): the HIP runtime torch bundles
    loses MEMSET nodes of replayed graph execs; the proposal stage's counters were zeroed by hipMemsetAsync.  The library zeroes with
    kernels now: three detectors alive together -- every exec's FIRST replay right behind the previous exec's, with nothing in between,
    then interleaved and concurrent replays on their own streams -- all return the eager results bit for bit, and no graph holds a
    memset / memcpy node."""
    from birdsoundclassif_amd import bulk
    model = _model()
    B = 4
    pcm = [torch.from_numpy(synth.clip_batch_pcm16(300 + B * k, B)).cuda() for k in range(4)]
    ref = _eager_refs(model, pcm)
    dets = [bulk.GraphedDetector(model, B, 66150, 22050, min_score=0.05), bulk.GraphedDetector(model, B, 66150, 22050, min_score=0.05),
            bulk.GraphedDetector(model, B, 66150, 22050, min_score=0.05, lanes=2)]
    assert len({k for d in dets for k in d.lane_ids}) == 4          # live detectors never share a lane's scratch
    for d in dets:
        assert d.census['memset'] == d.census['memcpy'] == d.census['host'] == d.census['other'] == 0 and d.census['kernel'] > 100, d.census
    feeds = [(dets[0].pcms[0], 0), (dets[1].pcms[0], 1), (dets[2].pcms[0], 2), (dets[2].pcms[1], 3)]
    for buf, k in feeds:
        buf.copy_(pcm[k])
    torch.cuda.synchronize()

    def check(tag):
        got = [(dets[0].dets[0], dets[0].n_dets[0]), (dets[1].dets[0], dets[1].n_dets[0]), (dets[2].dets[0], dets[2].n_dets[0]),
               (dets[2].dets[1], dets[2].n_dets[1])]
        for k in range(4):
            assert torch.equal(got[k][0], ref[k][0]) and torch.equal(got[k][1], ref[k][1]), (tag, k, int(got[k][1].sum()), int(ref[k][1].sum()))

    for rep in range(3):                                            # back to back, each exec's first replay included
        for d in dets:
            with torch.cuda.stream(d.stream):
                d.replay()
            torch.cuda.synchronize()
        check(('sequential', rep))
    for rep in range(3):                                            # all three in flight together
        for _ in range(2):
            for d in dets:
                with torch.cuda.stream(d.stream):
                    d.replay()
        torch.cuda.synchronize()
        check(('concurrent', rep))
    assert int(ref[0][1].sum()) > 0
    # a detector that is closed gives its lanes back
    dets[1].close()
    d4 = bulk.GraphedDetector(model, B, 66150, 22050, min_score=0.05)
    assert d4.lane_ids == [1]
    d4.pcm.copy_(pcm[1])
    with torch.cuda.stream(d4.stream):
        d4.replay()
    torch.cuda.synchronize()
    assert torch.equal(d4.det, ref[1][0]) and torch.equal(d4.n_det, ref[1][1])


def test_a_captured_step_with_a_memset_node_is_refused():
    """The fence behind the fix: whoever puts a memset node into the captured step (here: a hipMemsetAsync issued through ctypes on the
    runtime torch has loaded), `GraphedDetector` refuses to replay that graph."""
    import ctypes
    from birdsoundclassif_amd import bulk
    path = [l.split()[-1] for l in open('/proc/self/maps') if 'libamdhip64' in l][0]
    hip = ctypes.CDLL(path)
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    hip.hipMemsetAsync.restype = ctypes.c_int
    junk = torch.ones(64, dtype=torch.int32, device='cuda')

    class WithMemset(bulk.GraphedDetector):
        def _run(self, k=0):
            out = super()._run(k)
            assert hip.hipMemsetAsync(junk.data_ptr(), 0, 64, torch.cuda.current_stream().cuda_stream) == 0
            return out

    with pytest.raises(RuntimeError, match='memset'):
        WithMemset(_model(), 2, 66150, 22050, min_score=0.05)
    ok = bulk.GraphedDetector(_model(), 2, 66150, 22050, min_score=0.05)      # the failed capture left nothing behind
    assert ok.census['memset'] == 0 and ok.lane_ids == [0]
