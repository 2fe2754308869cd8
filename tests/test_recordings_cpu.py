"""CPU: the host side of the recording route (bulk.detect_recordings) -- the segment packer, the segment table, the window count
from a wav header, which files the route takes, and the C ABI entries it binds."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from birdsoundclassif_amd import _lib, bulk, ops, synth
from birdsoundclassif_amd.nbm_datasets.prepare_dataset import window_columns


def _windows(replays):
    """Every (file, window) in slot order, replay by replay."""
    return [(k, w) for r in replays for k, w0, n in r for w in range(w0, w0 + n)]


@pytest.mark.parametrize('batch,bs', [(64, 4), (24, 3), (8, 4), (4, 4), (5, 3), (7, 1)])
def test_packer_keeps_segments_whole_and_in_order(batch, bs):
    sizes = [244, 1, 7, 13, 1, 1, 35, 2, 4, 5, 61]
    p = bulk.SegmentPacker(batch, bs)
    replays = []
    for k, n in enumerate(sizes):
        replays += p.add(k, n)
    replays += p.flush()
    assert p.flush() == []
    # every window exactly once, files and windows in order
    assert _windows(replays) == [(k, w) for k, n in enumerate(sizes) for w in range(n)]
    for r in replays:
        assert 0 < sum(n for _, _, n in r) <= batch
        for k, w0, n in r:
            # a segment is the per-file driver's model call: windows [j*bs, min((j+1)*bs, n_img)), never split
            assert w0 % bs == 0 and n == min(bs, sizes[k] - w0)
        seg = bulk.SegmentPacker.segment_sizes(r, batch)
        assert sum(seg) == batch and seg[:len(r)] == [n for _, _, n in r]
    # a replay is closed only when the next segment does not fit
    for r, nxt in zip(replays, replays[1:]):
        assert sum(n for _, _, n in r) + nxt[0][2] > batch


def test_packer_shares_replays_between_files_and_pads_the_tail():
    p = bulk.SegmentPacker(24, 4)
    replays = p.add('a', 10) + p.add('b', 9) + p.add('c', 1) + p.flush()
    assert [[(k, w0, n) for k, w0, n in r] for r in replays] == [
        [('a', 0, 4), ('a', 4, 4), ('a', 8, 2), ('b', 0, 4), ('b', 4, 4), ('b', 8, 1), ('c', 0, 1)]]
    assert bulk.SegmentPacker.segment_sizes(replays[0], 24) == [4, 4, 2, 4, 4, 1, 1] + [1] * 4


def test_packer_needs_a_batch_that_holds_a_segment():
    with pytest.raises(ValueError):
        bulk.SegmentPacker(3, 4)


def test_segment_table_layout():
    t = ops.segment_table([4, 1, 3, 4, 2], 'cpu')
    assert t.dtype == torch.int32 and tuple(t.shape) == (2, 14)
    assert t[0].tolist() == [0, 0, 0, 0, 4, 5, 5, 5, 8, 8, 8, 8, 12, 12]
    assert t[1].tolist() == [4, 4, 4, 4, 1, 3, 3, 3, 4, 4, 4, 4, 2, 2]
    with pytest.raises(ValueError):
        ops.segment_table([2, 0, 1], 'cpu')


@pytest.mark.parametrize('sr', [22050, 44100])
@pytest.mark.parametrize('n', [1, 66150, 66151, 100000, 441000, 13230000, 26460000, int(5e7) - 1, int(5e7) + 12345,
                               int(6e7) + 7])
def test_recording_windows_matches_the_front_end_window_count(sr, n):
    n44 = n * (2 if sr == 22050 else 1)
    chunk = int(5e7)
    if n44 < chunk:
        Ls = [1 + n44 // 132]
    else:
        Ls = [1 + (min(n44, (k + 1) * chunk) - k * chunk) // 132 for k in range(int(n44 / chunk) + 1)]
    assert bulk.recording_windows(sr, n) == window_columns(Ls, 1024, 819)[0]


def test_int16_route_recordings_and_their_window_counts(tmp_path):
    d = str(tmp_path)
    synth.write_wav(os.path.join(d, 'clip.wav'), synth.clip_pcm16(1), 22050)
    synth.write_wav(os.path.join(d, 'rec.wav'), np.zeros(22050 * 40, np.int16), 22050)
    synth.write_wav(os.path.join(d, 'rec44.wav'), np.zeros(44100 * 7, np.int16), 44100)
    synth.write_wav(os.path.join(d, 'odd_rate.wav'), np.zeros(16000 * 10, np.int16), 16000)
    import wave
    with wave.open(os.path.join(d, 'stereo.wav'), 'wb') as f:
        f.setnchannels(2), f.setsampwidth(2), f.setframerate(22050)
        f.writeframes(np.zeros(2 * 22050 * 5, '<i2').tobytes())
    open(os.path.join(d, 'junk.wav'), 'wb').write(b'not a wav')
    files = sorted(os.path.join(d, f) for f in os.listdir(d))
    infos = bulk.probe_files(files)
    assert list(infos) == files
    take = [(os.path.basename(f), i.windows) for f, i in infos.items() if i and i.int16_route and i.recording]
    assert take == [('clip.wav', 1), ('rec.wav', 17), ('rec44.wav', 3)]
    rest = {os.path.basename(f): i for f, i in infos.items() if not (i and i.int16_route and i.recording)}
    assert sorted(rest) == ['junk.wav', 'odd_rate.wav', 'stereo.wav'] and rest['junk.wav'] is None
    # the other two are recordings of the decoder's formats
    assert [(n, rest[n].recording, rest[n].windows) for n in ('odd_rate.wav', 'stereo.wav')] == \
        [('odd_rate.wav', True, bulk.recording_windows(16000, 160000)), ('stereo.wav', True, bulk.recording_windows(22050, 110250))]


def test_proposal_entry_points_take_a_segment_table():
    assert 'nbm_spec_windows_table' in _lib.SIGNATURES
    # one proposal-count mode: the segment table is a required argument of the two proposal entry points
    for name in ('nbm_rpn_select_seg', 'nbm_nms_batched_seg'):
        assert name not in _lib.SIGNATURES
    for name in ('nbm_rpn_select', 'nbm_nms_batched'):
        assert _lib.SIGNATURES[name][-2:] == [C.c_void_p, C.c_void_p]          # (pointer seg, pointer stream)
    assert ops.WINDOW_ENTRY_WORDS * 8 == 40          # sizeof(struct nbm_window_entry)
