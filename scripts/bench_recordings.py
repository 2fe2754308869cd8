"""Throughput of the recording route (bulk.detect_recordings) against the per-file driver (run_detection) on a shard of
synthetic night recordings; prints one JSON line.

    python scripts/bench_recordings.py [--files 64] [--seconds 600] [--batch 64] [--bs 4] [--min_score 0.2] [--skip_per_file]
                                       [--tf_rcnn [--tf_pe_qk] [--tf_num_encoder_layers N]] [--clips N]

--tf_rcnn: the transformer head instead of the conv head (filler weights either way).  --clips N: N more 3 s clips go through
the clip route (bulk.detect_files, --batch clips per replay, capture included in its wall time) and through the per-file driver.

The recordings are rotations of a few distinct synthetic signals (synth.clip_pcm16, generated in a process pool), written as
mono 16-bit wav at 22.05 kHz into a temporary directory.  The graph capture is timed on its own; the route's wall time starts
when the detector exists.  Both drivers' per-file dictionaries are compared (equal_outputs)."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from birdsoundclassif_amd import synth  # noqa: E402

SR = 22050


def _signal(args):
    seed, n = args
    return synth.clip_pcm16(seed, n, SR)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--files', type=int, default=64)
    p.add_argument('--seconds', type=float, default=600)
    p.add_argument('--distinct', type=int, default=8, help='distinct signals; the other files are rotations of them')
    p.add_argument('--batch', type=int, default=64)
    p.add_argument('--bs', type=int, default=4)
    p.add_argument('--min_score', type=float, default=0.2)
    p.add_argument('--skip_per_file', action='store_true')
    p.add_argument('--tf_rcnn', action='store_true')
    p.add_argument('--tf_pe_qk', action='store_true')
    p.add_argument('--tf_num_encoder_layers', type=int, default=6)
    p.add_argument('--clips', type=int, default=0, help='3 s clips for the clip route (0: skip that leg)')
    a = p.parse_args()

    n = int(SR * a.seconds)
    d = tempfile.mkdtemp(prefix='nbm_rec_')
    try:
        t0 = time.perf_counter()
        k = min(a.distinct, a.files)
        with Pool(min(k, 16)) as pool:
            base = pool.map(_signal, [(9000 + i, n) for i in range(k)])
        files = []
        for i in range(a.files):
            x = np.roll(base[i % k], (i // k) * 7919 * 13)
            f = os.path.join(d, f'night{i:03d}.wav')
            synth.write_wav(f, x, SR)
            files.append(f)
        t_gen = time.perf_counter() - t0

        import torch
        from birdsoundclassif_amd import bulk
        from birdsoundclassif_amd.nets import build_model
        from birdsoundclassif_amd.run_detection import run_detection
        from birdsoundclassif_amd.train import default_args
        torch.cuda.set_device(0)
        head = dict(tf_rcnn=True, tf_pe_qk=a.tf_pe_qk, tf_num_encoder_layers=a.tf_num_encoder_layers) if a.tf_rcnn else {}
        model, _ = build_model(default_args(device='cuda', **head))
        model.load_state_dict(synth.fill_state_dict({kk: tuple(v.shape) for kk, v in model.state_dict().items()}))
        model = model.cuda().eval()
        names = {f'Species {i}': i for i in range(1, model.args.num_classes + 1)}
        bird_dict = os.path.join(d, 'bird_dict.json')
        with open(bird_dict, 'w') as f:
            json.dump(names, f)

        torch.cuda.synchronize()
        t0 = time.perf_counter()
        det = bulk.RecordingDetector(model, a.batch, min_score=a.min_score)
        torch.cuda.synchronize()
        t_capture = time.perf_counter() - t0
        stats = {}
        t0 = time.perf_counter()
        got = bulk.detect_recordings(model, files, batch=a.batch, bs=a.bs, min_score=a.min_score, bird_dict=names,
                                     write_txt=False, stats=stats, detector=det)
        torch.cuda.synchronize()
        t_route = time.perf_counter() - t0
        det.close()
        windows = stats['windows']
        res = {'head': head or 'conv', 'files': a.files, 'seconds_per_file': a.seconds, 'windows': windows, 'batch': a.batch, 'bs': a.bs,
               'min_score': a.min_score, 'generate_s': round(t_gen, 2), 'capture_s': round(t_capture, 3),
               'route_s': round(t_route, 3), 'route_windows_per_s': round(windows / t_route, 1),
               'route_stats': {kk: (round(v, 4) if isinstance(v, float) else v) for kk, v in stats.items()}}
        if not a.skip_per_file:
            run_detection(model, model.args, files[0], bird_dict, min_score=a.min_score, bs=a.bs)     # warm
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ref = [run_detection(model, model.args, f, bird_dict, min_score=a.min_score, bs=a.bs) for f in files]
            torch.cuda.synchronize()
            t_pf = time.perf_counter() - t0
            res.update(per_file_s=round(t_pf, 3), per_file_windows_per_s=round(windows / t_pf, 1),
                       speedup=round(t_pf / t_route, 3), equal_outputs=all(str(x) == str(y) for x, y in zip(got, ref)))
        if a.clips:
            clips = []
            for i in range(a.clips):
                f = os.path.join(d, f'clip{i:04d}.wav')
                synth.write_wav(f, np.roll(base[i % k][:3 * SR], (i // k) * 7919), SR)
                clips.append(f)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = bulk.detect_files(model, clips, batch=a.batch, min_score=a.min_score, bird_dict=names, write_txt=False)
            torch.cuda.synchronize()
            t_clip = time.perf_counter() - t0
            res.update(clips=a.clips, clip_route_s=round(t_clip, 3), clip_route_clips_per_s=round(a.clips / t_clip, 1))
            if not a.skip_per_file:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ref = [run_detection(model, model.args, f, bird_dict, min_score=a.min_score, bs=a.bs) for f in clips]
                torch.cuda.synchronize()
                t_pf = time.perf_counter() - t0
                res.update(clips_per_file_s=round(t_pf, 3), clips_per_file_clips_per_s=round(a.clips / t_pf, 1),
                           clips_equal_outputs=all(str(x) == str(y) for x, y in zip(got, ref)))
        print(json.dumps(res))
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == '__main__':
    main()
