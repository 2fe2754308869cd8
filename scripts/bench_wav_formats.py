"""The device wav decoder (nbm_wav_decode) and the bulk routes on file formats other than mono 16-bit PCM at 22.05 / 44.1 kHz;
prints one JSON line per leg.

    python scripts/bench_wav_formats.py [--files 64] [--seconds 600] [--batch 64] [--bs 4] [--clips 8,64,256,1024]
                                        [--clip_lanes N] [--control_runs 3] [--skip_per_file]

1. decoder alone: HIP events around 20 launches (after 3 warm-up launches) on one --seconds row per format; GB/s = (bytes read +
   bytes written) / time, next to the 6.3 TB/s achievable-HBM figure of the project's roofline.
2. recording route (bulk.detect_recordings) on --files synthetic --seconds recordings (rotations of a few distinct signals, like
   scripts/bench_recordings.py) stored as (a) mono PCM16 22.05 kHz -- the control, run --control_runs times, its spread is the
   yardstick -- (b) mono PCM16 48 kHz, (c) stereo 24-bit 96 kHz: windows/s of the route and of the per-file driver on the same
   files, with the route's stage times; and, per format, the GPU time of the stages in front of the STFT on one file, HIP
   events around each: H2D copy of the payload, decode, 44.1 kHz waveform (half-band interpolator or polyphase resampler),
   and the whole spectrogram_db.
3. clip route (bulk.detect_files, capture included in its wall time, replay batch chosen like the CLI: min(--batch, group size
   rounded up to 8)) on 2.9 s clips of formats (a) and (b) for every group size of --clips, against the per-file driver."""
import argparse
import json
import os
import shutil
import struct
import sys
import tempfile
import time
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from birdsoundclassif_amd import synth  # noqa: E402

FORMATS = {'a_pcm16_22k_mono': (22050, 16, 1), 'b_pcm16_48k_mono': (48000, 16, 1), 'c_pcm24_96k_stereo': (96000, 24, 2)}


def _signal(args):
    seed, n, sr = args
    return synth.clip_pcm16(seed, n, sr)


def write_pcm(path, x, sr, bits, channels):
    """int16 mono signal -> PCM wav: 16 bits as it is; 24 bits shifted up by 8; stereo = the signal and its half-level delay."""
    x = np.asarray(x, dtype=np.int16)
    ch = np.stack([np.roll(x, 7 * c) // (c + 1) for c in range(channels)], 1).astype(np.int32)
    if bits == 16:
        payload = ch.astype('<i2').tobytes()
    else:
        payload = ((ch << 8) & 0xFFFFFF).astype('<u4').view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    fb = channels * bits // 8
    with open(path, 'wb') as f:
        f.write(b'RIFF' + struct.pack('<I', 36 + len(payload)) + b'WAVEfmt ' +
                struct.pack('<IHHIIHH', 16, 1, channels, sr, sr * fb, fb, bits) + b'data' + struct.pack('<I', len(payload)))
        f.write(payload)


def decoder_leg(seconds):
    import torch
    from birdsoundclassif_amd import ops
    out = []
    for (tag, bits), ch, sr in [((1, 8), 1, 22050), ((1, 16), 1, 48000), ((1, 16), 2, 44100), ((1, 24), 1, 96000), ((1, 24), 2, 96000),
                                ((1, 32), 2, 96000), ((3, 32), 1, 96000), ((3, 32), 8, 48000), ((3, 64), 2, 96000)]:
        n = int(sr * seconds)
        nbytes = n * ch * (bits // 8)
        raw = torch.randint(0, 256, (1, nbytes), dtype=torch.uint8, device='cuda')
        dst = torch.empty((1, n), dtype=torch.float32, device='cuda')
        for _ in range(3):
            ops.wav_decode(raw, tag, bits, ch, n, out=dst)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            ops.wav_decode(raw, tag, bits, ch, n, out=dst)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 20
        out.append({'tag': tag, 'bits': bits, 'channels': ch, 'rate': sr, 'frames': n, 'MB_in': round(nbytes / 1e6, 1),
                    'MB_out': round(4 * n / 1e6, 1), 'us': round(ms * 1e3, 1), 'GB_per_s': round((nbytes + 4 * n) / ms / 1e6, 1)})
    print(json.dumps({'leg': 'decoder', 'hbm_achievable_GB_per_s': 6300, 'rows': out}), flush=True)


def _events(fn, reps=5):
    """Mean GPU milliseconds of fn() over `reps` runs after one warm-up run."""
    import torch
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / reps, 3)


def stage_leg(label, path, fe):
    """GPU time per file of what the recording route runs in front of the STFT."""
    import torch
    from birdsoundclassif_amd import bulk, ops
    fmt, sr, n, raw = bulk.read_payload(path)
    pin = torch.from_numpy(raw)[None]
    pin = pin.pin_memory() if not pin.is_pinned() else pin
    dev = torch.empty(pin.shape, dtype=torch.uint8, device='cuda')
    res = {'leg': 'stages_ms_per_file', 'format': label, 'payload_MB': round(pin.shape[1] / 1e6, 1)}
    res['h2d'] = _events(lambda: dev.copy_(pin, non_blocking=True))
    if bulk.is_pcm16_mono(fmt, sr):
        x = dev.view(torch.int16)
        res['decode'] = 0.0
    else:
        res['decode'] = _events(lambda: ops.wav_decode(dev, *fmt, n))
        x = ops.wav_decode(dev, *fmt, n)
    src = fe._source(x.dtype, x.shape[1], sr)
    ld = -(-(src[1] + 2 * (fe.WIN_LENGTH // 2) + fe.WIN_LENGTH) // 4) * 4
    lead = fe.WIN_LENGTH // 2
    if src[0] == 'pcm16':
        res['to_44k_wave'] = _events(lambda: ops.pcm16_to_wave(x, ld, lead, src[2], fe.hq))
    else:
        res['to_44k_wave'] = _events(lambda: ops.resample_to_wave(x, ld, lead, src[2][0], src[2][1], src[2][2]))
    res['spectrogram_db'] = _events(lambda: fe.spectrogram_db(x, sr))
    print(json.dumps(res), flush=True)


def clip_leg(model, names, bird_dict, sub, label, base, sr, bits, ch, sizes, a):
    import torch
    from birdsoundclassif_amd import bulk
    from birdsoundclassif_amd.run_detection import run_detection
    k = len(base)
    clips = []
    for i in range(max(sizes)):
        f = os.path.join(sub, f'clip{i:04d}.wav')
        write_pcm(f, np.roll(base[i % k][:int(2.9 * sr)], (i // k) * 7919), sr, bits, ch)
        clips.append(f)
    ref, t_pf = [], []
    if not a.skip_per_file:
        run_detection(model, model.args, clips[0], bird_dict, min_score=a.min_score, bs=a.bs)     # warm
        torch.cuda.synchronize()
        for f in clips:
            t0 = time.perf_counter()
            ref.append(run_detection(model, model.args, f, bird_dict, min_score=a.min_score, bs=a.bs))
            torch.cuda.synchronize()
            t_pf.append(time.perf_counter() - t0)
    for size in sizes:
        batch = min(a.batch, -(-size // 8) * 8)
        stats = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = bulk.detect_files(model, clips[:size], batch=batch, min_score=a.min_score, bird_dict=names, write_txt=False, stats=stats,
                                lanes=a.clip_lanes)
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        cres = {'leg': 'clips', 'format': label, 'clips': size, 'batch': batch, 'lanes': stats['lanes'], 'clip_route_s': round(t, 3),
                'of_which_loop_s': round(stats['wall_s'], 3), 'clip_route_clips_per_s': round(size / t, 1)}
        if ref:
            cres.update(per_file_s=round(sum(t_pf[:size]), 3), per_file_clips_per_s=round(size / sum(t_pf[:size]), 1),
                        equal_outputs=all(str(x) == str(y) for x, y in zip(got, ref[:size])))
        print(json.dumps(cres), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--files', type=int, default=64)
    p.add_argument('--seconds', type=float, default=600)
    p.add_argument('--distinct', type=int, default=4)
    p.add_argument('--batch', type=int, default=64)
    p.add_argument('--bs', type=int, default=4)
    p.add_argument('--min_score', type=float, default=0.2)
    p.add_argument('--clips', type=str, default='8,64,256,1024', help='clip group sizes for the clip route ("": skip that leg)')
    p.add_argument('--clip_lanes', type=int, default=None, help="lanes of the clip route (default: detect_files' own choice)")
    p.add_argument('--control_runs', type=int, default=3)
    p.add_argument('--skip_per_file', action='store_true')
    a = p.parse_args()

    import torch
    from birdsoundclassif_amd import bulk
    from birdsoundclassif_amd.nets import build_model
    from birdsoundclassif_amd.run_detection import run_detection
    from birdsoundclassif_amd.train import default_args
    torch.cuda.set_device(0)
    decoder_leg(a.seconds)

    model, _ = build_model(default_args(device='cuda'))
    model.load_state_dict(synth.fill_state_dict({kk: tuple(v.shape) for kk, v in model.state_dict().items()}))
    model = model.cuda().eval()
    names = {f'Species {i}': i for i in range(1, model.args.num_classes + 1)}
    d = tempfile.mkdtemp(prefix='nbm_fmt_')
    try:
        bird_dict = os.path.join(d, 'bird_dict.json')
        with open(bird_dict, 'w') as f:
            json.dump(names, f)
        det = bulk.RecordingDetector(model, a.batch, min_score=a.min_score)
        sizes = sorted(int(v) for v in a.clips.split(',') if v)
        k = min(a.distinct, a.files)
        for label, (sr, bits, ch) in FORMATS.items():
            sub = os.path.join(d, label)
            os.makedirs(sub)
            n = int(sr * a.seconds)
            with Pool(min(k, 16)) as pool:
                base = pool.map(_signal, [(9000 + i, n, sr) for i in range(k)])
            files = []
            for i in range(a.files):
                f = os.path.join(sub, f'night{i:03d}.wav')
                write_pcm(f, np.roll(base[i % k], (i // k) * 7919 * 13), sr, bits, ch)
                files.append(f)
            res = {'leg': 'recordings', 'format': label, 'rate': sr, 'bits': bits, 'channels': ch, 'files': a.files,
                   'seconds_per_file': a.seconds, 'MB_per_file': round(os.path.getsize(files[0]) / 1e6, 1), 'runs': []}
            for _ in range(a.control_runs if label.startswith('a_') else 1):
                stats = {}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = bulk.detect_recordings(model, files, batch=a.batch, bs=a.bs, min_score=a.min_score, bird_dict=names,
                                             write_txt=False, stats=stats, detector=det)
                torch.cuda.synchronize()
                t = time.perf_counter() - t0
                res['windows'] = stats['windows']
                res['runs'].append({'route_s': round(t, 3), 'route_windows_per_s': round(stats['windows'] / t, 1),
                                    'rejected': len(stats['rejected']),
                                    **{kk: round(stats[kk], 3) for kk in ('reader_busy_s', 'front_end_host_s', 'main_waited_for_reader_s')}})
            if not a.skip_per_file:
                run_detection(model, model.args, files[0], bird_dict, min_score=a.min_score, bs=a.bs)     # warm
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ref = [run_detection(model, model.args, f, bird_dict, min_score=a.min_score, bs=a.bs) for f in files]
                torch.cuda.synchronize()
                t = time.perf_counter() - t0
                res.update(per_file_s=round(t, 3), per_file_windows_per_s=round(res['windows'] / t, 1),
                           equal_outputs=all(str(x) == str(y) for x, y in zip(got, ref)))
            print(json.dumps(res), flush=True)
            stage_leg(label, files[0], det.fe)
            if sizes and label[0] in 'ab':
                clip_leg(model, names, bird_dict, sub, label, base, sr, bits, ch, sizes, a)
            shutil.rmtree(sub, ignore_errors=True)
        det.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == '__main__':
    main()
