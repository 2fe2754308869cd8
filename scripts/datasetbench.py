"""Times the training-input stage at B=128: the host half of an item (`raw_item`) and the device half (`DeviceCollate`:
PNG reconstruction + std + augmentation), and, with `--inflate`, both inflate routes side by side: host zlib against
`nbm_png_inflate` (Img_dataset(device_inflate=True)).

    python scripts/datasetbench.py                 # the two noise routes, as before
    python scripts/datasetbench.py --inflate       # + host against device inflate, REPS repetitions (env REPS, default 7)
    python scripts/datasetbench.py --train         # + the train.py driver's step-to-step time at B, 4 workers, both routes
"""
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from birdsoundclassif_amd import ops, synth                               # noqa: E402
from birdsoundclassif_amd.nbm_datasets.image_dataset import Img_dataset   # noqa: E402
from birdsoundclassif_amd.nbm_datasets.prepare_dataset import encode_png_gray8   # noqa: E402

B = int(os.environ.get('B', 128))
REPS = int(os.environ.get('REPS', 7))


def spread(xs):
    return f'median {statistics.median(xs):.2f} (min {min(xs):.2f}, max {max(xs):.2f}, n={len(xs)})'


def inflate_leg(root):
    """Host zlib against nbm_png_inflate on the same B items; every figure over REPS repetitions after one warm-up."""
    import zlib
    print(f'--- inflate routes, B={B}, 375 x 1024 synthetic spectrogram PNGs, zlib level 6 '
          f'(prepare_dataset.encode_png_gray8 compresses with zlib.compress(raw, 6))')
    res = {}
    for device_inflate in (False, True):
        ds = Img_dataset(root, transform=True, host_noise=False, device_inflate=device_inflate)
        host_ms = []
        for rep in range(REPS + 1):
            np.random.seed(0), torch.manual_seed(0)
            t0 = time.perf_counter()
            items = [ds.raw_item(i % 3) for i in range(B)]
            host_ms.append((time.perf_counter() - t0) / B * 1e3)
        host_ms = host_ms[1:]
        ds.collate(items)
        torch.cuda.synchronize()
        coll_ms = []
        for rep in range(REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = ds.collate(items)
            torch.cuda.synchronize()
            coll_ms.append((time.perf_counter() - t0) * 1e3)
        res[device_inflate] = (items, out, host_ms, coll_ms)
        route = 'device inflate' if device_inflate else 'host inflate  '
        print(f'{route}: raw_item ms/img/thread {spread(host_ms)}; DeviceCollate ms/batch incl. H2D {spread(coll_ms)}')
    assert torch.equal(res[False][1][0], res[True][1][0]) and torch.equal(res[False][1][1], res[True][1][1]), 'routes differ'
    items = res[True][0]
    images = [it['pos'] for it in items] + [it['neg'] for it in items] + [it['hard'] for it in items if 'hard' in it]
    H, W = images[0][1:]
    packed, table = ops.png_payload_pack([im[0] for im in images])
    print(f'{len(images)} streams per batch: payload {packed.size} B against scanlines {len(images) * H * (W + 1)} B '
          f'({packed.size / (len(images) * H * (W + 1)):.3f}x)')
    payload = torch.from_numpy(packed).cuda()
    ops.png_inflate(payload, table, H, W)
    torch.cuda.synchronize()
    kern_ms = []
    for rep in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        raw, status = ops.png_inflate(payload, table, H, W)
        e1.record()
        e1.synchronize()
        kern_ms.append(e0.elapsed_time(e1))
    assert not status.any()
    ref = np.frombuffer(zlib.decompress(images[0][0]), dtype=np.uint8)
    assert np.array_equal(raw[0].cpu().numpy(), ref)
    print(f'nbm_png_inflate, {len(images)} streams (device events around the call, table upload included): ms {spread(kern_ms)}')
    h_host, h_dev = statistics.median(res[False][2]), statistics.median(res[True][2])
    c_host, c_dev = statistics.median(res[False][3]), statistics.median(res[True][3])
    print(f'summary: device inflate frees {(h_host - h_dev) * B:.0f} core-ms per batch of {B} '
          f'({h_host:.2f} -> {h_dev:.2f} ms/img/thread) at a cost of {statistics.median(kern_ms):.1f} ms of device time '
          f'(DeviceCollate {c_host:.1f} -> {c_dev:.1f} ms)')


def train_leg(root):
    """`train.main` at B (default 128), --num_workers 4, on both inflate routes: time from one optimisation step's start to
    the next one's (input wait + collate + step), the first 3 of STEPS (env, default 13) left out."""
    import shutil
    from birdsoundclassif_amd import train as T
    steps = int(os.environ.get('STEPS', 13))
    big = os.path.join(root, 'big')                       # 2 B positives: copies of the three synthetic ones
    shutil.copytree(root, big, ignore=shutil.ignore_patterns('big'))
    d = os.path.join(big, 'positive_files', 'recA')
    rows = open(os.path.join(d, 'annotations.csv')).read().splitlines()
    with open(os.path.join(d, 'annotations.csv'), 'a') as f:
        for i in range(2, 2 * B):
            shutil.copy(os.path.join(d, f'recA__{i % 2}.png'), os.path.join(d, f'recA__{i}.png'))
            f.write(f'{i};' + rows[1 + i % 2].split(';', 1)[1] + '\n')
    real, real_build = T.train_one_step, T.build_optimizer

    def build_with_filler(model, a):      # filler weights: a fresh init may give an RPN that proposes nothing
        from birdsoundclassif_amd.nets import _prep
        model.load_state_dict(synth.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}))
        _prep.bump()
        return real_build(model, a)
    T.build_optimizer = build_with_filler
    print(f'--- train.py driver, batch_size {B}, num_workers 4, host_noise off, {steps} steps per route')
    for device_inflate in (False, True):
        marks = []

        def timed(*a, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = real(*a, **kw)
            torch.cuda.synchronize()
            marks.append((t0, time.perf_counter()))
            return out
        T.train_one_step = timed
        args = T.default_args(device='cuda', data_path=big, save_dir=os.path.join(root, f'models{int(device_inflate)}'),
                              model_name='m', batch_size=B, num_workers=4, validation_prop=0.0, max_steps=steps, seed=1,
                              neg_step_freq=10 ** 6)
        args.val_freq, args.device_inflate = 10 ** 6, device_inflate
        try:
            T.main(args)
        finally:
            T.train_one_step = real
        period = [(b[0] - a[0]) * 1e3 for a, b in zip(marks[3:], marks[4:])]
        step = [(m[1] - m[0]) * 1e3 for m in marks[3:]]
        route = 'device inflate' if device_inflate else 'host inflate  '
        print(f'{route}: step-to-step ms {spread(period)}; train_one_step alone ms {spread(step)}')


with tempfile.TemporaryDirectory() as root:
    synth.write_image_dataset(root, encode_png_gray8)
    for host_noise in (True, False):
        ds = Img_dataset(root, transform=True, host_noise=host_noise)
        np.random.seed(0), torch.manual_seed(0)
        t0 = time.perf_counter()
        items = [ds.raw_item(i % 3) for i in range(B)]
        t_host = time.perf_counter() - t0
        ds.collate(items)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            out = ds.collate(items)
        torch.cuda.synchronize()
        t_dev = (time.perf_counter() - t0) / 5
        print(f'host_noise={host_noise}: raw_item {t_host / B * 1e3:.2f} ms/img (inflate + labels + RNG, 1 thread); '
              f'collate B={B}: {t_dev * 1e3:.1f} ms = {B / t_dev:.0f} img/s incl. H2D')
    if '--inflate' in sys.argv[1:]:
        inflate_leg(root)
    if '--train' in sys.argv[1:]:
        train_leg(root)
