"""CLI of the reference's nbm_detect.py (nbm_model/nbm_detect.py:8-29): same flags, same `<wav>.txt = str(dict)`
outputs; `bird_dict.json` is looked up in the CWD like the reference, or given with --bird_dict.

Route: files that are equal-length single-window clips (<= 3.06 s) of one format and rate -- mono 16-bit PCM at 22.05 / 44.1 kHz
(`bulk.bulk_groups`), or any other format the device decoder takes: 8- / 16- / 24- / 32-bit PCM, 32- / 64-bit float, extensible
headers of those, 1 to 8 channels, any sample rate (`bulk.format_groups`) -- go through the pipelined hipGraph loop of
`bulk.detect_files` in batches of --bulk_batch, every clip an independent batch of one -- exactly what the reference's per-file
loop computes for them; everything else goes through the per-file `run_detection` driver with --batch windows per model call,
like the reference -- or, when the recordings in those formats among them (`bulk.recording_files`, `bulk.decodable_recordings`;
plus clip groups too small for the clip route) hold at least RECORDINGS_MIN_WINDOWS windows, through the graph-replayed
recording route `bulk.detect_recordings`: the same --batch-window model calls as segments of --bulk_batch-window launches.  On
both routes the payload bytes go to the GPU undecoded (`nbm_wav_decode`).  Compressed formats, more than 8 channels, files past
the 1.5e8-sample limit and unreadable files stay with the per-file driver.  --no_bulk forces the per-file driver.
Multi-GPU: launch one process per GPU (torchrun); files are sharded `files[rank::world]`, no collective."""
import argparse
import glob
import json
import os

BULK_MIN_FILES = 8          # below this a graph capture (3 batch-sized steps) costs more than it saves
# Clip groups in the formats of `bulk.format_groups` go through the graph one batch at a time: the capture of a two-lane graph
# costs seconds, which a group below several hundred clips does not earn back, and the replay loop was no faster with two lanes
# (profiles/wav_formats.txt, clip legs).  Mono PCM16 groups keep `detect_files`' own choice.
FORMAT_GROUP_LANES = 1
RECORDINGS_MIN_WINDOWS = 256   # the recording route's capture (3 launches of --bulk_batch windows) pays off past a few launches


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
    import torch
    rank, world = int(os.environ.get('RANK', 0)), int(os.environ.get('WORLD_SIZE', 1))
    torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', 0)))
    from . import bulk
    from .run_detection import load_model, run_detection
    model, config = load_model(args.ckpt)
    files = sorted(glob.glob(os.path.join(args.audio_dir, '*.wav')))[rank::world]
    groups, rest = ({}, files) if args.no_bulk else bulk.bulk_groups(files)
    if not args.no_bulk:                                 # clips in the other formats the device decoder takes
        more, rest = bulk.format_groups(rest)
        groups.update(more)
    done = 0
    bird_dict = None
    if groups:
        with open(args.bird_dict, 'r') as f:
            bird_dict = json.load(f)
    for key, group in sorted(groups.items(), key=lambda kv: (len(kv[0]), kv[0])):
        if len(group) < BULK_MIN_FILES:
            rest.extend(group)
            continue
        batch = min(args.bulk_batch, -(-len(group) // 8) * 8)
        try:
            try:
                bulk.detect_files(model, group, batch=batch, min_score=args.min_score, bird_dict=bird_dict, write_txt=True,
                                  keep_results=False, lanes=FORMAT_GROUP_LANES if len(key) == 5 else None)
            except torch.cuda.OutOfMemoryError:
                # two lanes = a second set of persistent scratch and graph-pool activations: degrade to one batch in flight
                torch.cuda.empty_cache()
                print(f'bulk route: out of device memory with two batches in flight; retrying the group of {len(group)} clips with one lane')
                bulk.detect_files(model, group, batch=batch, min_score=args.min_score, bird_dict=bird_dict, write_txt=True,
                                  keep_results=False, lanes=1)
        except (ValueError, NotImplementedError, OSError) as exc:
            # a file whose header disagrees with its data, a truncated or changing file, a decode the bulk reader does not do: the
            # per-file driver (= the reference's behaviour) takes the whole group (it rewrites the txt files the bulk route finished)
            print(f'bulk route gave up on a group of {len(group)} clips ({type(exc).__name__}: {exc}); they go through the per-file driver')
            rest.extend(group)
            continue
        done += len(group)
        what = f'{key[1]} samples @ {key[0]} Hz' if len(key) == 2 else \
            f'{key[4]} samples @ {key[3]} Hz, format tag {key[0]}, {key[1]} bits, {key[2]} channels'
        print(f'{done} / {len(files)} processed~ (bulk route: {len(group)} clips of {what})')
    if not args.no_bulk:
        take, others = bulk.recording_files(sorted(rest))
        more, others = bulk.decodable_recordings(others)     # recordings in the other formats the device decoder takes
        take = sorted(take + more)
        if sum(w for _, w in take) >= RECORDINGS_MIN_WINDOWS:
            take = [f for f, _ in take]
            if bird_dict is None:
                with open(args.bird_dict, 'r') as f:
                    bird_dict = json.load(f)
            stats = {}
            try:
                bulk.detect_recordings(model, take, batch=max(args.bulk_batch, args.batch), bs=args.batch,
                                       min_score=args.min_score, bird_dict=bird_dict, write_txt=True, keep_results=False,
                                       stats=stats)
                rest = others + stats['rejected']
                done += len(take) - len(stats['rejected'])
                print(f'{done} / {len(files)} processed~ (recording route: {stats["windows"]} windows of '
                      f'{len(take) - len(stats["rejected"])} files in {stats["replays"]} launches)')
            except (ValueError, NotImplementedError, OSError, torch.cuda.OutOfMemoryError) as exc:
                # the per-file driver (= the reference's behaviour) takes them all and rewrites what the route finished
                torch.cuda.empty_cache()
                print(f'recording route gave up on {len(take)} files ({type(exc).__name__}: {exc}); they go through the per-file driver')
    for wav_path in sorted(rest):
        output = run_detection(model, config, wav_path, args.bird_dict, min_score=args.min_score, bs=args.batch)
        done += 1
        print(f'{done} / {len(files)} processed~')
        with open(wav_path.replace('.wav', '.txt'), 'w') as f:
            f.write(f'{str(output)}')


if __name__ == '__main__':
    main()
