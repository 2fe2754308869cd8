"""GPU: the per-file merge of long recordings on the device (csrc/merge.hip) -- greedy NMS against a scalable CPU greedy up to
the 2^17-box limit, collect + NMS + gather against oracle.nets_ref.merge_images, the dictionary API `merge_images` above the
old 4 096-box ceiling, and `run_detection` end to end on a 10-minute recording."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from birdsoundclassif_amd import ops, synth                                    # noqa: E402
from helpers import filler_state_dict                                          # noqa: E402
from merge_cpu_ref import HOP, W_PIX, greedy_keep, make_boxes                  # noqa: E402
from oracle import nets_ref as O                                               # noqa: E402

NC = 150


def _device_keep(b, thresh=0.3):
    n = len(b)
    boxes = torch.from_numpy(np.ascontiguousarray(b, dtype=np.float32).reshape(-1, 4)).cuda()
    if n == 0:
        boxes = torch.zeros((1, 4), device='cuda')
    n_in = torch.full((1,), n, device='cuda', dtype=torch.int32)
    keep, n_keep = ops.merge_nms(boxes, n_in, thresh, cap=n)
    return keep[:int(n_keep.item())].cpu().tolist()


# ----------------------------------------------------------------------------------------------- 1. NMS kernel
@pytest.mark.parametrize('layout', ['realistic', 'dense', 'scattered'])
@pytest.mark.parametrize('n', [0, 1, 63, 64, 65, 4095, 4096, 4097, 20000, 69250, 131072])
def test_merge_nms_matches_cpu_greedy(layout, n):
    b = make_boxes(layout, n, seed=1000 + n)
    ref = greedy_keep(b, 0.3)
    if n <= 4096:
        assert ref == O.greedy_nms_keep(torch.from_numpy(b), 0.3)
    got = _device_keep(b)
    assert got == ref, (layout, n, len(got), len(ref))


def test_merge_nms_cross_checks_with_oracle_dense():
    b = make_boxes('dense', 2000, seed=3)
    assert _device_keep(b) == O.greedy_nms_keep(torch.from_numpy(b), 0.3) == greedy_keep(b)


def test_merge_nms_above_limit_refused():
    boxes = torch.zeros((ops.MERGE_MAX_N + 1, 4), device='cuda')
    n_in = torch.full((1,), ops.MERGE_MAX_N + 1, device='cuda', dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.merge_nms(boxes, n_in, 0.3)
    # the C entry point itself: over-limit capacity or a null workspace -> NBM_EINVAL, nothing launched
    import ctypes
    lib = ops.lib()
    keep = torch.empty((16,), device='cuda', dtype=torch.int32)
    cnt = torch.empty((1,), device='cuda', dtype=torch.int32)
    args = (ops._ptr(boxes), ops._ptr(n_in))
    assert lib.nbm_merge_nms(*args, ops.MERGE_MAX_N + 1, ctypes.c_float(0.3), ops._ptr(keep), 1 << 40, ops._ptr(keep),
                             ops._ptr(cnt), ops._stream()) == -1
    assert lib.nbm_merge_nms(*args, 64, ctypes.c_float(0.3), None, 1 << 20, ops._ptr(keep), ops._ptr(cnt), ops._stream()) == -1


def test_merge_nms_device_count_clamped_to_capacity():
    b = make_boxes('scattered', 640, seed=9)
    boxes = torch.from_numpy(b).cuda()
    n_in = torch.full((1,), 100000, device='cuda', dtype=torch.int32)        # count above the capacity: clamped to cap
    keep, n_keep = ops.merge_nms(boxes, n_in, 0.3, cap=640)
    assert keep[:int(n_keep.item())].cpu().tolist() == greedy_keep(b)


# ----------------------------------------------------------------------------------------------- 2. collect + NMS + gather
def _synthetic_det(n_img, seed, cap=50):
    """rcnn_post-like rows [n_img, cap, 6] sorted by (class, score desc), n_det [n_img], with the border cases planted."""
    rng = np.random.default_rng(seed)
    det = np.zeros((n_img, cap, 6), np.float32)
    n_det = np.zeros(n_img, np.int32)
    for i in range(n_img):
        if i % 7 == 3:
            continue                                                        # all-empty window
        k = int(rng.integers(1, cap + 1))
        cls = np.sort(rng.choice(np.arange(1, NC + 1), size=k, replace=True))
        x1 = rng.integers(0, 1000, k).astype(np.float32)
        x2 = np.minimum(x1 + rng.integers(5, 400, k), 1023).astype(np.float32)
        y1 = rng.integers(0, 300, k).astype(np.float32)
        y2 = np.minimum(y1 + rng.integers(5, 75, k), 374).astype(np.float32)
        sc = rng.uniform(0.01, 1, k).astype(np.float32)
        # x2 == w_pix - 5, x1 == 4, width exactly float32(0.9 * 205) = 184.5 and one ulp under it, the right edge, near-border widths
        special = [(919, 1019), (4, 150), (10, 194.5), (10, float(np.nextafter(np.float32(194.5), np.float32(0)))),
                   (830, 1015.5), (835, 1023), (0, 183), (0, 185), (850, 1019)]
        for s, (a, bb) in enumerate(special):
            if s < k and rng.uniform() < 0.7:
                x1[s], x2[s] = np.float32(a), np.float32(bb)
        rows = np.stack([cls.astype(np.float32), x1, y1, x2, y2, sc], 1)
        o = np.lexsort((-rows[:, 5], rows[:, 0]))
        det[i, :k] = rows[o]
        n_det[i] = k
    return det, n_det


def _det_to_dicts(det, n_det):
    out = []
    for i in range(len(n_det)):
        d = {str(c): dict(bbox_coord=torch.Tensor(), scores=torch.Tensor()) for c in range(1, NC + 1)}
        rows = torch.from_numpy(det[i, :n_det[i]])
        for c in range(1, NC + 1):
            m = rows[:, 0] == c
            if m.any():
                d[str(c)] = dict(bbox_coord=rows[m, 1:5].clone(), scores=rows[m, 5][None].clone())
        out.append(d)
    return out


def _rows_of(res):
    rows = [[float(j), *res[str(j)]['bbox_coord'][r].tolist(), float(res[str(j)]['scores'].reshape(-1)[r])]
            for j in range(1, NC + 1) for r in range(len(res[str(j)]['bbox_coord']))]
    return np.array(rows, np.float32).reshape(-1, 6)


class _FP:
    def __init__(self, n_img, tail=300):
        self.W_PIX, self.HOP_SPECTRO = W_PIX, HOP
        self.spectrogram_length = HOP * (n_img - 1) + W_PIX - tail


@pytest.mark.parametrize('n_img', [1, 2, 3, 1385])
def test_device_merge_matches_oracle(n_img, monkeypatch):
    from birdsoundclassif_amd.run_detection import merge_device
    det, n_det = _synthetic_det(n_img, seed=n_img)
    fp = _FP(n_img)
    if n_img > 100:
        monkeypatch.setattr(O, 'greedy_nms_keep', greedy_keep)        # the oracle's n x n IoU matrix does not fit at ~40k boxes
    ref = _rows_of(O.merge_images(fp.W_PIX, fp.HOP_SPECTRO, fp.spectrogram_length, _det_to_dicts(det, n_det), NC))
    got = merge_device(fp, torch.from_numpy(det).cuda(), torch.from_numpy(n_det).cuda(), NC).numpy()
    assert got.shape == ref.shape and got.tobytes() == ref.tobytes(), (got.shape, ref.shape)
    if n_img == 1385:
        assert len(ref) > 4096


# ----------------------------------------------------------------------------------------------- 3. dictionary API
def test_merge_images_above_old_ceiling(monkeypatch):
    from birdsoundclassif_amd.run_detection import merge_images
    n_img = 240
    det, n_det = _synthetic_det(n_img, seed=77)
    wins = _det_to_dicts(det, n_det)
    fp = _FP(n_img)
    seen = []
    greedy = O.greedy_nms_keep
    monkeypatch.setattr(O, 'greedy_nms_keep', lambda b, t: seen.append(len(b)) or greedy(b, t))
    ref = O.merge_images(fp.W_PIX, fp.HOP_SPECTRO, fp.spectrogram_length, wins, NC)
    assert seen[0] > 4096                        # collected candidates: the old driver raised NotImplementedError here
    got = merge_images(fp, [wins[s:s + 10] for s in range(0, n_img, 10)], NC)
    assert _rows_of(got).tobytes() == _rows_of(ref).tobytes()


# ----------------------------------------------------------------------------------------------- 4. end to end
@pytest.fixture(scope='module')
def detector(tmp_path_factory):
    from birdsoundclassif_amd.run_detection import load_model
    from birdsoundclassif_amd.train import default_args
    d = tmp_path_factory.mktemp('long')
    ck = d / 'model_weights'
    ck.mkdir()
    args = default_args(device='cuda')
    cfg = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in vars(args).items() if k not in ('scales',)}
    (ck / 'args').write_text(json.dumps(cfg))
    torch.save({'checkpoints': filler_state_dict(), 'steps': 0, 'epoch': 0, 'best_val_cls_loss': 99}, str(ck / 'model_chkpt.pt'))
    (d / 'bird_dict.json').write_text(json.dumps({f'Species {i}': i for i in range(1, NC + 1)}))
    model, cfg = load_model(str(ck))
    return model, cfg, d


def _wav(d, name, seconds, seed):
    p = str(d / name)
    synth.write_wav(p, synth.clip_pcm16(seed, int(22050 * seconds)), 22050)
    return p


def _oracle_run(model, path, min_score, bs):
    """The reference's loop: model(...) per group of bs windows -> flat dicts -> oracle merge_images."""
    from birdsoundclassif_amd.nbm_datasets.prepare_dataset import File_Processor
    fp = File_Processor(path)
    fp.process_file(device='cuda')
    imgs = fp.images_device
    outs = []
    for s in range(0, imgs.shape[0], bs):
        with torch.no_grad():
            outs.extend(model(imgs[s:s + bs][:, None].contiguous(), min_score=min_score))
    n_pre = sum(len(o[str(c)]['bbox_coord']) for o in outs for c in range(1, NC + 1))
    return fp, outs, n_pre


def _named(res, drop_empty=True):
    return {f'Species {j}': {'bbox_coord': res[str(j)]['bbox_coord'].cpu().numpy().tolist(),
                             'scores': res[str(j)]['scores'].reshape(-1).cpu().numpy().tolist()}
            for j in range(1, NC + 1) if len(res[str(j)]['bbox_coord']) > 0}


def test_run_detection_10_minutes_above_old_ceiling(detector, monkeypatch):
    from birdsoundclassif_amd.run_detection import run_detection
    model, cfg, d = detector
    path = _wav(d, 'night.wav', 600, 4242)
    got = run_detection(model, cfg, path, str(d / 'bird_dict.json'), min_score=0.0, bs=10)
    fp, outs, n_pre = _oracle_run(model, path, 0.0, 10)
    assert n_pre > 4096, n_pre
    monkeypatch.setattr(O, 'greedy_nms_keep', greedy_keep)
    ref = O.merge_images(fp.W_PIX, fp.HOP_SPECTRO, fp.spectrogram_length, outs, NC)
    assert got == _named(ref)


def test_run_detection_short_file_same_as_dictionary_route(detector):
    from birdsoundclassif_amd.run_detection import merge_images, run_detection
    model, cfg, d = detector
    path = _wav(d, 'short.wav', 30, 4343)
    got = run_detection(model, cfg, path, str(d / 'bird_dict.json'), min_score=0.05, bs=4)
    fp, outs, n_pre = _oracle_run(model, path, 0.05, 4)
    assert len(outs) > 3 and 0 < n_pre <= 4096
    assert got == _named(merge_images(fp, [outs[s:s + 4] for s in range(0, len(outs), 4)], NC))
    assert got == _named(O.merge_images(fp.W_PIX, fp.HOP_SPECTRO, fp.spectrogram_length, outs, NC))
