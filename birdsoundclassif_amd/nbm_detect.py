"""CLI of the reference's nbm_detect.py (nbm_model/nbm_detect.py:8-29): same flags, same `<wav>.txt = str(dict)`
outputs; `bird_dict.json` is looked up in the CWD like the reference, or given with --bird_dict.

Route: the headers of the shard are read once (`bulk.probe_files`) and each file's `bulk.WavInfo` decides.  `clip`: equal-length
single-window clips (<= 3.06 s) of one format and rate go through the pipelined hipGraph loop of `bulk.detect_files` in batches of
--bulk_batch, every clip an independent batch of one -- exactly what the reference's per-file loop computes for them.  `recording`:
what is left in the formats the device decoder takes, small clip groups included, goes through `bulk.detect_recordings` if it holds
RECORDINGS_MIN_WINDOWS windows: the per-file driver's --batch-window model calls as segments of --bulk_batch-window graph replays.
Everything else (with --no_bulk: every file) goes through that driver, `run_detection`, like the reference.
Multi-GPU: launch one process per GPU (torchrun); files are sharded `files[rank::world]`, no collective."""
import argparse
import functools
import glob
import json
import os

import torch
from . import bulk
from .run_detection import load_model, run_detection

BULK_MIN_FILES = 8          # below this a graph capture (3 batch-sized steps) costs more than it saves
# Clip groups in formats other than mono PCM16 at 22.05 / 44.1 kHz (those keep `detect_files`' own choice) go through the graph
# one batch at a time: capturing two lanes costs seconds, which a group below several hundred clips does not earn back, and the
# replay loop was no faster with two lanes (profiles/wav_formats.txt, clip legs).
FORMAT_GROUP_LANES = 1
RECORDINGS_MIN_WINDOWS = 256   # the recording route's capture (3 launches of --bulk_batch windows) pays off past a few launches


def clip_route(model, infos, args, bird_dict, report):
    """Clip groups of at least BULK_MIN_FILES files through `bulk.detect_files` -> the WavInfos left over."""
    left = [info for info in infos if not info.clip]
    for (tag, bits, nch, sr, n), group in bulk.clip_groups(infos):
        if len(group) < BULK_MIN_FILES:
            left += group
            continue
        int16, paths = group[0].int16_route, [info.path for info in group]
        kw = dict(batch=min(args.bulk_batch, -(-len(group) // 8) * 8), min_score=args.min_score, bird_dict=bird_dict(), write_txt=True, keep_results=False)
        try:
            try:
                bulk.detect_files(model, paths, lanes=None if int16 else FORMAT_GROUP_LANES, **kw)
            except torch.cuda.OutOfMemoryError:     # two lanes = a second set of scratch and activations: degrade to one batch in flight
                torch.cuda.empty_cache()
                print(f'bulk route: out of device memory with two batches in flight; retrying the group of {len(group)} clips with one lane')
                bulk.detect_files(model, paths, lanes=1, **kw)
        except (ValueError, NotImplementedError, OSError) as exc:
            # e.g. a header that disagrees with its data, a changing file: the per-file driver takes the group and rewrites its txt files
            print(f'bulk route gave up on a group of {len(group)} clips ({type(exc).__name__}: {exc}); they go through the per-file driver')
            left += group
            continue
        what = f'{n} samples @ {sr} Hz' + ('' if int16 else f', format tag {tag}, {bits} bits, {nch} channels')
        report(len(group), f'bulk route: {len(group)} clips of {what}')
    return left


def recording_route(model, infos, args, bird_dict, report):
    """The `recording` files through `bulk.detect_recordings`, if they hold RECORDINGS_MIN_WINDOWS windows -> the paths left over."""
    take = sorted(info.path for info in infos if info.recording)
    if sum(info.windows for info in infos if info.recording) < RECORDINGS_MIN_WINDOWS:
        return [info.path for info in infos]
    stats = {}
    try:
        bulk.detect_recordings(model, take, batch=max(args.bulk_batch, args.batch), bs=args.batch, min_score=args.min_score,
                               bird_dict=bird_dict(), write_txt=True, keep_results=False, stats=stats)
    except (ValueError, NotImplementedError, OSError, torch.cuda.OutOfMemoryError) as exc:
        torch.cuda.empty_cache()    # the per-file driver (= the reference's behaviour) takes them all and rewrites what the route finished
        print(f'recording route gave up on {len(take)} files ({type(exc).__name__}: {exc}); they go through the per-file driver')
        return [info.path for info in infos]
    n = len(take) - len(stats['rejected'])
    report(n, f'recording route: {stats["windows"]} windows of {n} files in {stats["replays"]} launches')
    return [info.path for info in infos if not info.recording] + stats['rejected']


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--ckpt', type=str, help='directory with the json `args` and model_chkpt.pt')
    parser.add_argument('--audio_dir', type=str)
    parser.add_argument('--min_score', type=float, default=0.2)
    parser.add_argument('--batch', type=int, default=4)
    parser.add_argument('--bird_dict', type=str, default='bird_dict.json')
    parser.add_argument('--bulk_batch', type=int, default=64, help='clips per graph replay on the bulk route')
    parser.add_argument('--no_bulk', action='store_true', help='per-file driver for every file')
    args = parser.parse_args(argv)
    rank, world = int(os.environ.get('RANK', 0)), int(os.environ.get('WORLD_SIZE', 1))
    torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', 0)))
    model, config = load_model(args.ckpt)
    files, done = sorted(glob.glob(os.path.join(args.audio_dir, '*.wav')))[rank::world], 0

    def report(n, route=None):
        nonlocal done
        done += n
        print(f'{done} / {len(files)} processed~' + (f' ({route})' if route else ''))

    @functools.cache
    def bird_dict():                                     # read once, and only if a bulk route runs
        with open(args.bird_dict, 'r') as f:
            return json.load(f)
    rest = files
    if not args.no_bulk:
        probed = bulk.probe_files(files)
        left = clip_route(model, [info for info in probed.values() if info], args, bird_dict, report)
        rest = [f for f in files if probed[f] is None] + recording_route(model, left, args, bird_dict, report)
    for wav_path in sorted(rest):
        output = run_detection(model, config, wav_path, args.bird_dict, min_score=args.min_score, bs=args.batch)
        report(1)
        bulk.write_result(wav_path, output)


if __name__ == '__main__':
    main()
