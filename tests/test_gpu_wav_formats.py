"""GPU: wav payloads decoded on the device (nbm_wav_decode) -- the decoder bit for bit against `read_wav`, and every readable
format on the two captured routes (bulk.detect_recordings, bulk.detect_files) and the CLI against the per-file driver."""
import ast
import json
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from birdsoundclassif_amd import bulk, ops, synth                              # noqa: E402
from birdsoundclassif_amd.nbm_datasets.prepare_dataset import read_wav          # noqa: E402
from birdsoundclassif_amd.train import default_args                            # noqa: E402
from helpers import filler_state_dict                                          # noqa: E402
import wavfmt                                                                  # noqa: E402

NC = 150
LENGTHS = [1, 15, 16, 17, 4099]
CHANNELS = [1, 2, 3, 4, 5, 6, 7, 8]


def _payload(tag, bits, n, channels, seed):
    """Interleaved payload bytes of n frames with random samples and the extremes of the format among them."""
    rng = np.random.default_rng(seed)
    m = n * channels
    if tag == 1 and bits == 8:
        v = rng.integers(0, 256, m).astype(np.uint8)
        v[:4] = [0, 255, 128, 127][:len(v[:4])]
        return v.tobytes()
    if tag == 1 and bits in (16, 24, 32):
        lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
        v = rng.integers(lo, hi + 1, m, dtype=np.int64)
        ext = [lo, hi, -1, 0, 1, lo + 1, (1 << 24) + 1, -(1 << 24) - 1, (1 << 25) + 2, 0x7FFFFF7F, 0x7FFFFF80, 0x7FFFFFC0]
        ext = [e for e in ext if lo <= e <= hi]
        k = min(m, len(ext))
        v[rng.permutation(m)[:k]] = ext[:k]
        v[0] = lo                                                             # the most negative integer is always present
        return wavfmt.pack24(v) if bits == 24 else v.astype('<i2' if bits == 16 else '<i4').tobytes()
    if tag == 3 and bits == 32:
        v = rng.standard_normal(m).astype(np.float32) * np.float32(0.4)
        ext = np.array([1.0, -1.0, 0.0, -0.0, 1e-40, 3.0e38, np.float32(1) - np.float32(2) ** -24], np.float32)
        k = min(m, len(ext))
        v[rng.permutation(m)[:k]] = ext[:k]
        return v.astype('<f4').tobytes()
    v = rng.standard_normal(m) * 0.4
    one_ulp = float(np.float32(2) ** -23)
    ext = [1.0, -1.0, 1.0 + 0.5 * one_ulp + 1e-12, 1.0 + 1.5 * one_ulp, 1.0 + 0.5 * one_ulp, -(1.0 + 0.75 * one_ulp),
           float(np.finfo(np.float32).max), 1e-300, 0.1,                      # values that round up into float32, ties to even
           1e-40, -3e-42, 2.0 ** -149, 1.5 * 2.0 ** -149, 2.5 * 2.0 ** -149, 0.5 * 2.0 ** -149, 0.5000001 * 2.0 ** -149,
           2.0 ** -126 * (1 - 2.0 ** -25)]                                    # float32 subnormals: results, ties, the step into normals
    k = min(m, len(ext))
    v[rng.permutation(m)[:k]] = ext[:k]
    return v.astype('<f8').tobytes()


def _decode(payload, tag, bits, channels, n):
    raw = torch.frombuffer(bytearray(payload), dtype=torch.uint8)[None].cuda()
    out = ops.wav_decode(raw, tag, bits, channels, n)
    torch.cuda.synchronize()
    return out[0].cpu().numpy()


def _read_wav_f32(path):
    x, sr = read_wav(path)
    return (x.astype(np.float32) * np.float32(1.0 / 32768.0) if x.dtype == np.int16 else x), sr


@pytest.mark.parametrize('tag,bits', wavfmt.FORMATS)
@pytest.mark.parametrize('extensible', [False, True])
def test_decoder_equals_read_wav_bit_for_bit(tmp_path, tag, bits, extensible):
    """Every format x channels 1 .. 8 x lengths 1, 15, 16, 17, 4 099 frames, plain and extensible headers.  Offsets
    are 64-bit in the kernel (row * pitch, span * span bytes, frame * frame bytes, all `long long`); byte offsets beyond 2^32
    would need a buffer no test should allocate, and the entry point has no frame-offset argument: that arithmetic is
    reviewed, not tested."""
    for channels in CHANNELS:
        for n in LENGTHS:
            payload = _payload(tag, bits, n, channels, 1000 * bits + 10 * channels + n)
            path = str(tmp_path / f'f_{channels}_{n}.wav')
            open(path, 'wb').write(wavfmt.riff(payload, 48000, tag, bits, channels, extensible=extensible))
            want, _ = _read_wav_f32(path)
            h = bulk.wav_header(path)
            assert (h[0], h[1], h[3], h[4]) == (tag, channels, bits, n)
            got = _decode(payload, h[0], h[3], h[1], n)
            assert got.dtype == np.float32 and got.shape == want.shape
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (tag, bits, channels, n,
                                                                               np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:8])


def test_float_bit_patterns_pass_through(tmp_path):
    """Mono float32: NaN payloads (quiet and signalling), infinities, denormals arrive bit for bit; infinities survive the
    down-mix like in numpy."""
    bits = np.array([0x7FC00000, 0x7F800001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x3F800000] * 5 + [0x7FA00000],
                    dtype='<u4')
    got = _decode(bits.tobytes(), 3, 32, 1, len(bits))
    assert np.array_equal(got.view(np.uint32), bits)
    path = str(tmp_path / 'nan.wav')
    open(path, 'wb').write(wavfmt.riff(bits.tobytes(), 44100, 3, 32, 1))
    assert np.array_equal(read_wav(path)[0].view(np.uint32), bits)
    st = np.array([np.inf, 1.0, -np.inf, -2.0, 0.5, np.inf, 3.0e38, 3.0e38] * 5, dtype='<f4')      # the last pair overflows the sum
    open(path, 'wb').write(wavfmt.riff(st.tobytes(), 44100, 3, 32, 2))
    with np.errstate(over='ignore'):
        want = read_wav(path)[0]
    assert np.array_equal(_decode(st.tobytes(), 3, 32, 2, 20).view(np.uint32), want.view(np.uint32))


def test_extreme_values_of_every_width():
    assert _decode(bytes([0, 255]), 1, 8, 1, 2).tolist() == [-1.0, 127 / 128]
    assert _decode(np.array([-32768, 32767], '<i2').tobytes(), 1, 16, 1, 2).tolist() == [-1.0, 32767 / 32768]
    assert _decode(wavfmt.pack24([-(1 << 23), (1 << 23) - 1]), 1, 24, 1, 2).tolist() == [-1.0, 8388607 / 8388608]
    assert _decode(np.array([-(1 << 31), (1 << 31) - 1], '<i4').tobytes(), 1, 32, 1, 2).tolist() == [-1.0, 1.0]
    assert _decode(np.array([1.0, -1.0], '<f4').tobytes(), 3, 32, 1, 2).tolist() == [1.0, -1.0]
    assert _decode(np.array([1.0, -1.0], '<f8').tobytes(), 3, 64, 1, 2).tolist() == [1.0, -1.0]


@pytest.mark.parametrize('tag,bits,channels,n,out_pitch', [(1, 24, 2, 4099, 4104), (1, 16, 3, 1001, 1003), (3, 64, 8, 37, 64),
                                                           (1, 8, 1, 50, 52), (1, 32, 7, 333, 333)])
def test_batch_of_rows_with_pitch_writes_nothing_else(tag, bits, channels, n, out_pitch):
    """Several rows whose pitch (input: bytes, output: elements) is larger than the row: every row equals its own decode and
    what lies behind the n samples of an output row stays NaN.  out_pitch % 4 != 0 takes the kernel's unaligned-store path."""
    batch, fb = 5, channels * (bits // 8)
    pitch = bulk.payload_pitch((tag, bits, channels), n) + 32
    rows = [_payload(tag, bits, n, channels, 77 + b) for b in range(batch)]
    host = np.full((batch, pitch), 0xA5, np.uint8)
    for b, r in enumerate(rows):
        host[b, :n * fb] = np.frombuffer(r, np.uint8)
    out = torch.full((batch, out_pitch), float('nan'), device='cuda')
    got = ops.wav_decode(torch.from_numpy(host).cuda(), tag, bits, channels, n, out=out)
    torch.cuda.synchronize()
    assert got.shape == (batch, n) and got.data_ptr() == out.data_ptr()
    o = out.cpu().numpy()
    assert np.isnan(o[:, n:]).all()
    for b, r in enumerate(rows):
        assert np.array_equal(o[b, :n].view(np.uint32), _decode(r, tag, bits, channels, n).view(np.uint32)), b


def test_unreadable_formats_are_refused():
    raw = torch.zeros((1, 64), dtype=torch.uint8, device='cuda')
    for tag, bits, ch in [(6, 8, 1), (7, 8, 1), (1, 12, 1), (3, 16, 1), (0xFFFE, 16, 1), (1, 16, 9), (1, 16, 0)]:
        with pytest.raises(NotImplementedError):
            ops.wav_decode(raw, tag, bits, ch, 4)
        rc = ops.lib().nbm_wav_decode(ops._ptr(raw), 64, 1, tag, bits, ch, 4, ops._ptr(torch.zeros(4, device='cuda')), 4, ops._stream())
        assert rc == -3, (tag, bits, ch, rc)
    with pytest.raises(ValueError):
        ops.wav_decode(raw, 1, 16, 2, 17)                                     # 68 bytes do not fit the row
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.wav_decode(raw.cpu(), 1, 16, 1, 4)


# ----------------------------------------------------------------------------------------------- routes
def _model(**kw):
    from birdsoundclassif_amd.nets import build_model
    m, _ = build_model(default_args(device='cuda', **kw))
    m.load_state_dict(filler_state_dict(**kw))
    return m.cuda().eval()


@pytest.fixture(scope='module')
def models():
    return {'conv': _model(), 'tf': _model(tf_rcnn=True, tf_pe_qk=True, tf_num_encoder_layers=2)}


RECORDINGS = {   # name: (seed, seconds, rate, tag, bits, channels)
    'r48.wav': (901, 11.3, 48000, 1, 16, 1), 'r44st.wav': (902, 8.7, 44100, 1, 16, 2), 'r96st24.wav': (903, 9.4, 96000, 1, 24, 2),
    'r32f.wav': (904, 12.1, 32000, 3, 32, 1), 'r22u8.wav': (905, 7.9, 22050, 1, 8, 1),
    'p22.wav': (906, 10.2, 22050, 1, 16, 1), 'p44.wav': (907, 6.6, 44100, 1, 16, 1)}


def _write_recordings(d):
    files = []
    for name, (seed, sec, sr, tag, bits, ch) in sorted(RECORDINGS.items()):
        x = synth.clip_pcm16(seed, int(sr * sec), sr)
        wavfmt.write(str(d / name), wavfmt.channels_of(x, ch), sr, tag, bits)
        files.append(str(d / name))
    return files


def _same(got, ref, what):
    assert set(got) == set(ref), what
    for k in ref:
        assert got[k]['bbox_coord'] == ref[k]['bbox_coord'] and got[k]['scores'] == ref[k]['scores'], (what, k)


@pytest.mark.parametrize('head', ['conv', 'tf'])
@pytest.mark.parametrize('bs', [4, 3])
def test_recording_route_takes_every_format(tmp_path, models, head, bs):
    from birdsoundclassif_amd.run_detection import run_detection
    model = models[head]
    names = {f'Species {i}': i for i in range(1, NC + 1)}
    (tmp_path / 'bird_dict.json').write_text(json.dumps(names))
    files = _write_recordings(tmp_path)
    stats = {}
    got = bulk.detect_recordings(model, files, batch=16, bs=bs, min_score=0.05, bird_dict=names, write_txt=False, stats=stats)
    assert stats['rejected'] == []
    assert stats['files'] == len(files) and stats['shared_replays'] > 0
    assert stats['windows'] == sum(bulk.recording_windows(sr, int(sr * sec)) for _, sec, sr, _, _, _ in RECORDINGS.values())
    n = 0
    for f, g in zip(files, got):
        ref = run_detection(model, model.args, f, str(tmp_path / 'bird_dict.json'), min_score=0.05, bs=bs)
        _same(g, ref, os.path.basename(f))
        n += sum(len(v['scores']) for v in g.values())
    assert n > 0


@pytest.mark.parametrize('sr,tag,bits,channels', [(48000, 1, 16, 1), (44100, 1, 24, 2)])
def test_clip_route_takes_other_formats(tmp_path, models, sr, tag, bits, channels):
    from birdsoundclassif_amd.run_detection import run_detection
    model = models['conv']
    names = {f'Species {i}': i for i in range(1, NC + 1)}
    (tmp_path / 'bird_dict.json').write_text(json.dumps(names))
    n = int(2.9 * sr)
    files = []
    for i in range(10):
        p = str(tmp_path / f'c{i}.wav')
        wavfmt.write(p, wavfmt.channels_of(synth.clip_pcm16(300 + i, n, sr), channels), sr, tag, bits)
        files.append(p)
    infos = list(bulk.probe_files(files).values())
    groups, rest = dict(bulk.clip_groups(infos)), [i.path for i in infos if not i.clip]
    assert list(groups) == [(tag, bits, channels, sr, n)] and rest == []
    got = bulk.detect_files(model, files, batch=4, min_score=0.05, bird_dict=names, write_txt=False)
    total = 0
    for f, g in zip(files, got):
        _same(g, run_detection(model, model.args, f, str(tmp_path / 'bird_dict.json'), min_score=0.05, bs=4), os.path.basename(f))
        total += sum(len(v['scores']) for v in g.values())
    assert total > 0
    # the captured graph: kernels only (decode and resampler in front of the detector included), replays repeat themselves
    det = bulk.GraphedDetector(model, 4, n, sr, min_score=0.05, independent=True, fmt=(tag, bits, channels))
    try:
        assert {k for k, v in det.census.items() if v} <= {'kernel', 'empty'} and det.census['kernel'] > 100, det.census
        assert det.pcm.dtype == torch.uint8 and det.pcm.shape == (4, bulk.payload_pitch((tag, bits, channels), n))
        for j in range(4):
            raw = bulk.read_payload(files[j])[3]
            det.pcm[j, :len(raw)].copy_(torch.from_numpy(raw))
        with torch.cuda.stream(det.stream):
            det.replay()
            a = det.det.clone(), det.n_det.clone()
            det.replay()
        det.stream.synchronize()
        assert torch.equal(a[0], det.det) and torch.equal(a[1], det.n_det) and int(a[1].sum()) > 0
    finally:
        det.close()


def test_cli_mixed_formats_write_the_same_files_as_the_per_file_driver(tmp_path, monkeypatch):
    from birdsoundclassif_amd import nbm_detect
    ck = tmp_path / 'model_weights'
    ck.mkdir()
    args = default_args(device='cuda')
    cfg = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in vars(args).items() if k not in ('scales',)}
    (ck / 'args').write_text(json.dumps(cfg))
    torch.save({'checkpoints': filler_state_dict(), 'steps': 0, 'epoch': 0, 'best_val_cls_loss': 99}, str(ck / 'model_chkpt.pt'))
    (tmp_path / 'bird_dict.json').write_text(json.dumps({f'Species {i}': i for i in range(1, NC + 1)}))
    a, b = tmp_path / 'route', tmp_path / 'perfile'
    a.mkdir()
    _write_recordings(a)
    clip_groups = {'k48_': (48000, 1, 16, 1), 'k24_': (44100, 1, 24, 2), 'kp_': (22050, 1, 16, 1)}
    for prefix, (sr, tag, bits, ch) in clip_groups.items():
        for i in range(8):
            x = synth.clip_pcm16(500 + i, int(2.9 * sr), sr)
            wavfmt.write(str(a / f'{prefix}{i}.wav'), wavfmt.channels_of(x, ch), sr, tag, bits)
    open(str(a / 'alaw.wav'), 'wb').write(wavfmt.riff(bytes(range(256)) * 64, 8000, 6, 8, 1))
    open(str(a / 'junk.wav'), 'wb').write(b'RIFF\x04\x00\x00\x00WAVE')
    shutil.copytree(str(a), str(b))

    monkeypatch.setattr(nbm_detect, 'RECORDINGS_MIN_WINDOWS', 16)
    seen_rec, seen_clip = [], []
    real_rec, real_clip = bulk.detect_recordings, bulk.detect_files

    def spy_rec(model, files, **kw):
        out = real_rec(model, files, **kw)
        seen_rec.append((sorted(os.path.basename(f) for f in files), dict(kw['stats'])))
        return out

    def spy_clip(model, files, **kw):
        out = real_clip(model, files, **kw)
        seen_clip.append(sorted(os.path.basename(f) for f in files))
        return out

    monkeypatch.setattr(bulk, 'detect_recordings', spy_rec)
    monkeypatch.setattr(bulk, 'detect_files', spy_clip)
    common = ['--ckpt', str(ck), '--min_score', '0.05', '--batch', '4', '--bird_dict', str(tmp_path / 'bird_dict.json')]
    nbm_detect.main(common + ['--audio_dir', str(a), '--bulk_batch', '8'])
    routed = (len(seen_rec), len(seen_clip))
    nbm_detect.main(common + ['--audio_dir', str(b), '--no_bulk'])
    assert (len(seen_rec), len(seen_clip)) == routed == (1, 3)                  # --no_bulk: neither route

    assert sorted(seen_clip) == sorted([f'{p}{i}.wav' for i in range(8)] for p in clip_groups)
    files, st = seen_rec[0]
    assert files == sorted(RECORDINGS) and st['rejected'] == [] and st['files'] == len(RECORDINGS)
    names = sorted(p.name for p in a.glob('*.txt'))
    # junk.wav and alaw.wav: the per-file driver writes what it writes for an unreadable file, on both sides
    assert names == sorted(p.name for p in b.glob('*.txt')) and len(names) >= len(RECORDINGS) + 24
    total = 0
    for name in names:
        ta = (a / name).read_text()
        assert ta == (b / name).read_text(), name
        total += sum(len(v['scores']) for v in ast.literal_eval(ta).values())
    assert total > 0
