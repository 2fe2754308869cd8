"""Bulk inference over many equal-length clips (BASELINE.json configs[4]): wav shard per GPU, the whole detect step
(front end + detector + device post-processing) captured once in a hipGraph and replayed per batch.

The graph is legal because `NbmModel.detect` never syncs with the host: every data-dependent size (kept anchors, NMS
survivors, RoI count, detections per clip) lives in fixed-capacity device buffers with device-side counters.

`detect_files` is a three-stage software pipeline around the graph, so that the GPU never waits for a file or a dict:

    reader thread   wav files -> rows of a pinned batch buffer (a ring of `depth` slots): int16 samples for mono 16-bit PCM at
                    22.05 / 44.1 kHz, the undecoded payload bytes for every other format (`read_payload`); those are decoded on
                    the GPU inside the captured step (`ops.wav_decode`: 8- / 16- / 24- / 32-bit PCM, 32- / 64-bit float, up to 8
                    channels, any rate the resampler takes), bit for bit what `read_wav` gives the per-file driver
    main thread     H2D copy of the slot -> graph replay -> D2H copy of the compact [B,50,6] detection rows + counts into the
                    slot's pinned result buffers, all on the graph's stream; batch i+1 is queued before the host waits for
                    batch i
    writer thread   rows -> the reference's per-file output dictionary (single-window `merge_images`) -> `<wav>.txt`

The clips of a batch are INDEPENDENT (`NbmModel.detect_calls` with `ops.batch_segments(B, 1)`, either head): the reference CLI runs one file per model call
(nbm_detect.py:24-28 -> run_detection.py:49-55, a 3 s clip is a batch of one window), so the batch-coupled proposal counts of
the reference's ProposalLayer / nms (min over the batch, layers.py:287, nets_utils.py:236) must not couple files that merely
share a launch here: every clip is a segment of its own (`ops.batch_segments(B, 1)`) and keeps its own counts, exactly as if it
had been run alone.

Multi-GPU: one process per GPU, files sharded `files[rank::world]`, no data-path collective (`nbm_detect.py` does the sharding).
"""
import itertools
import os
import queue
import struct
import threading
import time
from typing import NamedTuple

import numpy as np
import torch

from .nbm_datasets.prepare_dataset import SpectrogramFrontEnd, read_wav_pcm16, resample_ratio, resample_table_size


def check_head_segment(model, count, flag):
    """The transformer head's default flavour attends across the images of a model call (`ops.mha_segments`, ACROSS_IMAGES):
    a call = a segment of a bulk launch holds at most ops.MHA_SMAX images."""
    from . import ops
    a = model.args
    if getattr(a, 'tf_rcnn', False) and not getattr(a, 'tf_pe_qk', False) and count > ops.MHA_SMAX:
        raise ValueError(f'{flag} = {count}: the transformer head (--tf_rcnn) attends across the images of a model call, '
                         f'at most {ops.MHA_SMAX} of them')


class GraphedDetector:
    """Captures `front end -> model.detect_calls` for a fixed (batch, n_samples, sample rate) and replays it.

    `lanes` > 1: ONE graph whose capture forks into that many parallel branches (one stream each, joined before the capture ends),
    every branch a complete detect step on its own static input / outputs and its own persistent scratch (`ops.lane`): a replay
    processes `lanes` batches that are in flight on the GPU TOGETHER, so the tail of one step's kernels (a launch's last, partly
    filled round of workgroups; the latency-bound proposal / NMS kernels) is filled by the other's: 65.2 instead of 68.9 ms per
    B = 64 batch (profiles/r04_two_lanes.txt).

    Fence (profiles/r05_graph_pair.txt): the HIP runtime that torch 2.10+rocm7.0 bundles (7.0.51831) loses MEMSET nodes of a
    replayed graph exec -- round 4's "second graph exec computes garbage / faults" was the proposal stage's counters, zeroed by
    hipMemsetAsync = memset nodes, keeping the previous replay's values.  The library zeroes with kernels now, and the capture is
    refused unless its graph consists of kernel (and empty fork / join) nodes only (`ops.graph_census`), whoever issued the others.
    The persistent scratch / tile-list buffers of the lanes are held as captured (`self._held`), so no later growth or release can
    recycle memory this graph writes to.  Several detectors may be alive at a time (`tests/test_gpu_detect_cli.py`)."""

    def __init__(self, model, batch, n_samples, sr, min_score=0.2, nms_thresh=0.3, device='cuda', independent=False, lanes=1,
                 fmt=None):
        """`fmt` = (format tag, bits, channels) of the clips' payload (`wav_header`): the static inputs `pcms` are then uint8
        [batch, row bytes rounded up to 16] batches of raw payload rows, and `ops.wav_decode` + the float front end (resampler
        for any rate but 44.1 kHz) are captured in front of the detector.  None = mono 16-bit PCM given as int16 samples."""
        self.sr, self.n_samples, self.independent, lanes = sr, int(n_samples), independent, max(1, int(lanes))
        self.fmt = tuple(int(v) for v in fmt) if fmt is not None else None
        if self.fmt is not None and not decodable(*self.fmt):
            raise NotImplementedError(f'wav format tag {fmt[0]} with {fmt[1]} bits per sample and {fmt[2]} channels')
        if not independent:
            check_head_segment(model, batch, 'clip batch (--bulk_batch)')
        self.n44, self.n_img = samples_44k(sr, n_samples), 1
        if not single_window(self.n44):
            raise NotImplementedError('GraphedDetector handles clips that fit one 1024-column window (<= 3.06 s)')
        shape, dtype = ((batch, n_samples), torch.int16) if fmt is None else ((batch, payload_pitch(self.fmt, n_samples)), torch.uint8)
        self.pcms = [torch.zeros(shape, dtype=dtype, device=device) for _ in range(lanes)]   # static graph inputs
        self.pcm = self.pcms[0]
        self._start(model, batch, lanes, device, min_score, nms_thresh)

    def _start(self, model, batch, lanes, device, min_score, nms_thresh):
        """What every detector is made of besides its static inputs (which exist by now: the warm-up reads them): a front end
        per lane, the streams, the lanes' scratch, and the captured graph."""
        from . import ops
        self.model, self.batch, self.lanes = model.eval(), batch, lanes
        self.min_score, self.nms_thresh = min_score, nms_thresh
        self.fes = [SpectrogramFrontEnd(device) for _ in range(self.lanes)]
        self.fe = self.fes[0]
        self.stream = torch.cuda.Stream()
        self.side = [torch.cuda.Stream() for _ in range(self.lanes - 1)]
        self.lane_ids = self._claim_lanes(self, self.lanes)
        try:
            self._capture(ops)
        except BaseException:
            self.close()                                          # a refused / failed capture leaves no lane claimed and no graph behind
            raise

    def _capture(self, ops):
        with torch.no_grad(), torch.cuda.stream(self.stream):
            for _ in range(2):                                   # warm-up: fills every weight / anchor / table cache, sizes the lanes' scratch
                self._run_all()
            self.stream.synchronize()
            for s_ in self.side:
                s_.synchronize()
            self.graph = torch.cuda.CUDAGraph(keep_graph=True)
            with torch.cuda.graph(self.graph, stream=self.stream):
                outs = self._run_all()                            # static graph outputs
        self.census = ops.graph_census(self.graph.raw_cuda_graph())
        bad = {k: v for k, v in self.census.items() if v and k not in ('kernel', 'empty')}
        if bad or not self.census['kernel']:
            raise RuntimeError(f'the captured detect step holds graph nodes other than kernels: {bad} (census {self.census}).  Memset '
                               'nodes are not replayed reliably by the HIP runtime torch bundles (DESIGN 4d): refusing to replay this graph')
        self.graph.instantiate()
        self._held = ops.lane_buffers(set(self.lane_ids))
        self.dets, self.n_dets = [o[0] for o in outs], [o[1] for o in outs]
        self.det, self.n_det = self.dets[0], self.n_dets[0]

    # lanes in use by live detectors: a second detector alive beside the first gets scratch of its own instead of sharing buffers
    # whose addresses both graphs would write through (two replays on two streams would race on them)
    _LANES_IN_USE = {}

    @classmethod
    def _claim_lanes(cls, owner, n):
        import weakref
        for k in [k for k, ref in cls._LANES_IN_USE.items() if ref() is None]:
            del cls._LANES_IN_USE[k]
        ids, k = [], 0
        while len(ids) < n:
            if k not in cls._LANES_IN_USE:
                ids.append(k)
                cls._LANES_IN_USE[k] = weakref.ref(owner)
            k += 1
        return ids

    def close(self):
        """Drops the graph, its static buffers and its hold on the lanes' scratch; lanes other than 0 are released to the allocator."""
        from . import ops
        self.graph = None
        self._held = []
        self.pcms = self.dets = self.n_dets = []
        self.pcm = self.det = self.n_det = None
        for k in getattr(self, 'lane_ids', []):
            ref = self._LANES_IN_USE.get(k)
            if ref is not None and ref() in (self, None):
                del self._LANES_IN_USE[k]
        self.lane_ids = []
        others = set(self._LANES_IN_USE)
        ops.release_lane_scratch(keep=tuple(others | {0}))

    def _run(self, k=0):
        from . import ops
        x = self.pcms[k] if self.fmt is None else ops.wav_decode(self.pcms[k], *self.fmt, self.n_samples)
        imgs, _ = self.fes[k](x, self.sr)
        segments = ops.batch_segments(self.batch, 1, imgs.device) if self.independent else None
        return self.model.detect_calls(imgs[:, 0][:, None].contiguous(), segments, self.nms_thresh, self.min_score)

    def _run_all(self):
        """Lane 0 on the current (main) stream, every other lane on its side stream between a fork and a join."""
        from . import ops
        main = torch.cuda.current_stream()
        outs = [None] * self.lanes
        for k, s_ in enumerate(self.side, start=1):
            s_.wait_stream(main)                                  # fork
            with torch.cuda.stream(s_), ops.lane(self.lane_ids[k]):
                outs[k] = self._run(k)
        with ops.lane(self.lane_ids[0]):
            outs[0] = self._run(0)
        for s_ in self.side:
            main.wait_stream(s_)                                  # join
        return outs

    def replay(self):
        """Runs the captured step(s) on the current content of `self.pcms`; results land in `self.dets`, `self.n_dets`."""
        self.graph.replay()

    def __call__(self, pcm):
        """pcm int16 [batch, n] (host or device) -> list[batch] of the reference's per-clip dictionaries (lane 0)."""
        from .nets.layers import FastRCNN
        self.pcm.copy_(pcm, non_blocking=True)
        self.replay()
        return FastRCNN.dets_to_dicts(self.det, self.n_det, self.model.args.num_classes)


def wav_header(path):
    """(format tag, channels, sample rate, bits, n_samples per channel, byte offset of the samples) of a RIFF/WAVE file, reading
    the chunk headers only."""
    with open(path, 'rb') as f:
        head = f.read(12)
        if len(head) < 12 or head[:4] != b'RIFF' or head[8:12] != b'WAVE':
            raise ValueError(f'{path}: not a RIFF/WAVE file')
        fmt = None
        while True:
            ch = f.read(8)
            if len(ch) < 8:
                raise ValueError(f'{path}: wav file without fmt / data chunk')
            cid, size = ch[:4], struct.unpack('<I', ch[4:])[0]
            if cid == b'fmt ':
                fmt = f.read(size + (size & 1))[:size]
            elif cid == b'data':
                if fmt is None:
                    raise ValueError(f'{path}: data chunk in front of the fmt chunk')
                tag, nch, sr, _, _, bits = struct.unpack('<HHIIHH', fmt[:16])
                if tag == 0xFFFE and len(fmt) >= 26:
                    tag = struct.unpack('<H', fmt[24:26])[0]
                off = f.tell()
                size = min(size, os.fstat(f.fileno()).st_size - off)
                return tag, nch, sr, bits, size // max(1, nch * (bits // 8)), off
            else:
                f.seek(size + (size & 1), 1)


def decodable(tag, bits, channels):
    """Does the device decoder (`ops.wav_decode`) take this payload format?  Everything `read_wav` reads, up to 8 channels."""
    from . import ops
    return (tag, bits) in ops.WAV_FORMATS and 1 <= channels <= ops.WAV_MAX_CHANNELS


def is_pcm16_mono(fmt, sr):
    """The format with an exact-integer front end of its own (`nbm_pcm16_to_wave`): its payload IS the int16 sample row."""
    return tuple(fmt) == (1, 16, 1) and sr in (22050, 44100)


def payload_pitch(fmt, n):
    """Bytes of a payload row of n frames, rounded up to the 16 bytes the decoder wants between the rows of a batch."""
    return -(-n * fmt[2] * (fmt[1] // 8) // 16) * 16


MAX_RESAMPLE_TABLE = 1 << 23      # taps (float64) of a resampler table the routes are willing to build: 64 MiB


def samples_44k(sr, n):
    """Length of the 44.1 kHz signal the front end makes of n samples at `sr` (SpectrogramFrontEnd._source): n L / M rounded
    up, L / M = 44100 / sr reduced -- n for 44.1 kHz, 2 n for 22.05 kHz."""
    L, M = resample_ratio(sr, SpectrogramFrontEnd.FREQ)
    return -(-n * L // M)


def rate_ok(sr):
    """A rate whose polyphase table (`resample_taps`) is of a sane size."""
    return sr >= 1 and resample_table_size(sr, SpectrogramFrontEnd.FREQ) <= MAX_RESAMPLE_TABLE


# the front end's default geometry (SpectrogramFrontEnd(dt=0.003, overlap_spectro=0.2, w_pix=1024): STFT hop, columns of a window,
# columns between windows), which both routes and the CLI run with; chunk and file limits are SpectrogramFrontEnd's own
HOP_LENGTH, W_PIX, HOP_SPECTRO = int(SpectrogramFrontEnd.FREQ * 0.003), 1024, int(0.8 * 1024)


def single_window(n44):
    """Does a 44.1 kHz signal of n44 samples fill exactly one spectrogram window (prepare_dataset.py:126,267)?"""
    return 1 + n44 // HOP_LENGTH <= W_PIX


def recording_windows(sr, n):
    """Number of spectrogram windows of a file of n samples per channel at any rate `sr` (prepare_dataset.py:267, per-chunk
    frame counts of the STFT above 5e7 samples of the 44.1 kHz signal like SpectrogramFrontEnd.spectrogram_db)."""
    n44, chunk = samples_44k(sr, n), SpectrogramFrontEnd.MAX_CHUNK
    if n44 < chunk:
        L = 1 + n44 // HOP_LENGTH
    else:
        L = sum(1 + (min(n44, (k + 1) * chunk) - k * chunk) // HOP_LENGTH for k in range(int(n44 / chunk) + 1))
    return max(1, int(1 + np.ceil((L - W_PIX) / HOP_SPECTRO)))


class WavInfo(NamedTuple):
    """What the chunk headers of a wav file say (`wav_header`), and every routing decision that follows from them."""
    path: str
    fmt: tuple             # (format tag, bits, channels)
    sr: int
    n: int                 # frames = samples per channel
    offset: int            # byte offset of the samples

    @classmethod
    def probe(cls, path):
        tag, nch, sr, bits, n, off = wav_header(path)
        return cls(path, (tag, bits, nch), sr, n, off)

    @property
    def nbytes(self):
        return self.n * self.fmt[2] * (self.fmt[1] // 8)

    @property
    def n44(self):
        return samples_44k(self.sr, self.n)

    @property
    def decodable(self):
        """A payload the device decoder and the resampler take: both bulk routes read nothing else."""
        return decodable(*self.fmt) and rate_ok(self.sr) and self.n > 0

    @property
    def int16_route(self):
        """Mono PCM16 at 22.05 / 44.1 kHz: the samples go to the exact-integer front end as they are, undecoded."""
        return is_pcm16_mono(self.fmt, self.sr)

    @property
    def clip(self):
        """A file of one spectrogram window: the clip route (`detect_files`) takes groups of equal `group_key`."""
        return self.decodable and single_window(self.n44)

    @property
    def recording(self):
        """A file of any number of windows (a clip too) up to the 1.5e8-sample limit past which the reference splits the file
        (process_long_file): the recording route (`detect_recordings`) takes it."""
        return self.decodable and self.n44 <= SpectrogramFrontEnd.MAX_ONE_PASS

    @property
    def windows(self):
        return recording_windows(self.sr, self.n)

    @property
    def group_key(self):
        return (*self.fmt, self.sr, self.n)


def probe_files(files):
    """{file: its WavInfo, or None for a header that cannot be read}; every file is opened once.  Whatever is None, neither
    `clip` nor `recording`, stays with the per-file driver: compressed formats, more than 8 channels, longer files."""
    infos = {}
    for f in files:
        try:
            infos[f] = WavInfo.probe(f)
        except (OSError, ValueError, struct.error):
            infos[f] = None
    return infos


def clip_groups(infos):
    """[(group_key, [WavInfo by path])] of the `clip` files among the WavInfos, in the order the CLI takes the groups: mono PCM16
    at 22.05 / 44.1 kHz (`int16_route`) first, then the other formats, each by ascending key."""
    clips = sorted((i for i in infos if i.clip), key=lambda i: (not i.int16_route, i.group_key, i.path))
    return [(key, list(group)) for key, group in itertools.groupby(clips, key=lambda i: i.group_key)]


def read_payload(path, out=None):
    """The sample bytes of a wav file, undecoded: -> ((tag, bits, channels), sample rate, frames, uint8 buffer [frames * frame
    bytes]).  The chunk headers are parsed (`wav_header`; a WavInfo in place of the path spares that) and the payload is read
    straight into `out` (a writable uint8 numpy array, e.g. a row of a pinned batch; it must be large enough) or, by default,
    into a fresh pinned tensor, whose numpy view is returned -- no decode, no per-sample work.  A truncated payload gives its
    whole frames, like `read_wav`."""
    info = path if isinstance(path, WavInfo) else WavInfo.probe(path)
    path, nbytes = info.path, info.nbytes
    if not decodable(*info.fmt):
        tag, bits, nch = info.fmt
        raise NotImplementedError(f'{path}: wav format tag {tag} with {bits} bits per sample and {nch} channels')
    if out is None:
        pin = torch.empty((max(1, nbytes),), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        out = pin.numpy()
    if out.dtype != np.uint8 or out.ndim != 1 or len(out) < nbytes:
        raise ValueError(f'{path}: a payload of {nbytes} bytes does not fit the buffer')
    with open(path, 'rb', buffering=0) as f:
        f.seek(info.offset)
        got, view = 0, memoryview(out)[:nbytes]
        while got < nbytes:
            k = f.readinto(view[got:])
            if not k:
                raise ValueError(f'{path}: the file shrank while it was read')
            got += k
    return info.fmt, info.sr, info.n, out[:nbytes]


def rows_to_result(rows, n, w_pix, hop, spectrogram_length, names=None):
    """Detection rows of ONE single-window file -> the per-file output dictionary of run_detection (reference
    run_detection.py:69-84 after `merge_images`, :163-249).  rows: float32 [>= n, 6] = {class, x1, y1, x2, y2, score} sorted by
    (class, score desc).  For a file that is one window `merge_images` applies the first-window border rule (:195-196) and the
    end-of-file rule (:213); its file-level NMS (:233) cannot suppress anything, because the detector's own class-agnostic NMS ran
    at the same threshold on the same boxes (all surviving pairs have IoU < 0.3).
    -> {species | class id: {'bbox_coord': [[x1,y1,x2,y2]...], 'scores': [...]}}, classes ascending."""
    res = {}
    if n <= 0:
        return res
    r = rows[:n]
    keep = ~((r[:, 3] >= w_pix - 5) & ((r[:, 3] - r[:, 1]) < np.float32(0.9 * (w_pix - hop)))) & ~(r[:, 3] >= spectrogram_length)
    r = r[keep]
    if len(r) == 0:
        return res
    cls = r[:, 0].astype(np.int64)
    starts = np.flatnonzero(np.r_[True, cls[1:] != cls[:-1]])
    ends = np.r_[starts[1:], len(r)]
    for s0, e0 in zip(starts.tolist(), ends.tolist()):
        k = int(cls[s0])
        res[names[k] if names else str(k)] = {'bbox_coord': r[s0:e0, 1:5].tolist(), 'scores': r[s0:e0, 5].tolist()}
    return res


def single_window_merge(d, w_pix, hop, spectrogram_length, names=None):
    """`rows_to_result` for one entry of `FastRCNN.dets_to_dicts` (the reference's per-image dictionary)."""
    rows = [np.concatenate([np.full((len(v['bbox_coord']), 1), float(k), dtype=np.float32), v['bbox_coord'].numpy(),
                            v['scores'].reshape(-1, 1).numpy()], 1) for k, v in d.items() if len(v['bbox_coord'])]
    if not rows:
        return {}
    rows = np.concatenate(rows).astype(np.float32)
    return rows_to_result(rows, len(rows), w_pix, hop, spectrogram_length, names)


def txt_path(wav_path):
    return wav_path.replace('.wav', '.txt')          # like the reference CLI (nbm_detect.py:27)


def write_result(wav_path, res):
    with open(txt_path(wav_path), 'w') as fh:
        fh.write(str(res))


def detect_files(model, files, batch=64, min_score=0.2, bird_dict=None, write_txt=True, depth=5, keep_results=True,
                 independent=True, stats=None, detector=None, lanes=None):
    """Detects over equal-length wav files of one format and rate (single-window clips of one `WavInfo.group_key`: mono
    16-bit PCM at 22.05 / 44.1 kHz as int16 samples, everything else the device decoder takes as payload bytes): -> list of per-file output
    dicts in `files` order (None entries with keep_results=False); `<wav>.txt = str(dict)` written when `write_txt`.
    The last, partial batch is padded with silence and its padding results are dropped.  `stats` (dict) receives the stage
    times.  `detector`: a GraphedDetector to reuse (same batch / clip length / rate / lanes).
    `lanes` (default: the detector's, else NBM_BULK_LANES, else 2 when the shard has at least 4 batches): batches go through the graph
    in groups of that many, in flight on the GPU together (see GraphedDetector)."""
    if not files:
        return []
    first = WavInfo.probe(files[0])
    sr, n = first.sr, first.n
    fmt = None if first.int16_route else first.fmt                              # None: the int16 samples themselves
    n_batches = -(-len(files) // batch)
    if lanes is None:
        lanes = detector.lanes if detector is not None else int(os.environ.get('NBM_BULK_LANES', '2' if n_batches >= 4 else '1'))
    lanes = max(1, int(lanes))
    det = detector or GraphedDetector(model, batch, n, sr, min_score=min_score, independent=independent, lanes=lanes, fmt=fmt)
    own_det = detector is None
    if (det.batch, det.n_samples, det.sr, det.fmt) != (batch, n, sr, fmt) or det.lanes != lanes:
        if own_det:
            det.close()
        raise ValueError('the GraphedDetector handed in was captured for another batch / clip length / sample rate / format / '
                         'number of lanes')
    fe = det.fe
    L = fe.n_frames(det.n44)
    names = None
    if bird_dict is not None:
        names = {v: k for k, v in bird_dict.items()}
        names[0] = 'Non bird sound'
    depth = max(3, depth, 3 * lanes)
    cap = det.det.shape[1]
    slots = [(torch.zeros(det.pcm.shape, dtype=det.pcm.dtype).pin_memory(), torch.zeros((batch, cap, 6), dtype=torch.float32).pin_memory(),
              torch.zeros((batch,), dtype=torch.int32).pin_memory()) for _ in range(depth)]
    free_q, ready_q, done_q = queue.Queue(), queue.Queue(), queue.Queue()
    for s in range(depth):
        free_q.put(s)
    out = [None] * len(files)
    err = []
    t_read, t_write = [0.0], [0.0]

    def reader():
        try:
            for i in range(n_batches):
                s = free_q.get()
                if s is None:                        # the writer failed (or the main loop is shutting down): pass it on
                    ready_q.put(None)
                    return
                t0 = time.perf_counter()
                chunk = files[i * batch:(i + 1) * batch]
                host = slots[s][0].numpy()
                for j, f in enumerate(chunk):
                    if fmt is None:
                        p, sr_i = read_wav_pcm16(f)
                        if sr_i != sr or len(p) != n:
                            raise ValueError(f'{f}: bulk detection needs clips of identical length and rate')
                        host[j] = p
                    else:                            # the payload bytes, undecoded, straight into the pinned row
                        if read_payload(f, host[j])[:3] != (fmt, sr, n):
                            raise ValueError(f'{f}: bulk detection needs clips of identical format, length and rate')
                if len(chunk) < batch:
                    host[len(chunk):] = 0
                t_read[0] += time.perf_counter() - t0
                ready_q.put((i, s, len(chunk)))
        except BaseException as exc:                 # noqa: BLE001 -- handed to the main thread
            err.append(exc)
            ready_q.put(None)

    def writer():
        try:
            while True:
                item = done_q.get()
                if item is None:
                    return
                i, s, cnt = item
                t0 = time.perf_counter()
                rows, nd = slots[s][1].numpy(), slots[s][2].numpy()
                for j in range(cnt):
                    res = rows_to_result(rows[j], int(nd[j]), fe.W_PIX, fe.HOP_SPECTRO, L, names)
                    f = files[i * batch + j]
                    if keep_results:
                        out[i * batch + j] = res
                    if write_txt:
                        write_result(f, res)
                t_write[0] += time.perf_counter() - t0
                free_q.put(s)
        except BaseException as exc:                 # noqa: BLE001
            err.append(exc)
            free_q.put(None)

    th_r, th_w = threading.Thread(target=reader, daemon=True), threading.Thread(target=writer, daemon=True)
    t_start = time.perf_counter()
    th_r.start(), th_w.start()
    inflight = []
    t_wait_in = 0.0
    try:
        with torch.no_grad(), torch.cuda.stream(det.stream):
            k, stop = 0, False
            while k < n_batches and not stop:
                group = []
                for j in range(min(lanes, n_batches - k)):      # the lanes' inputs: H2D on the graph's stream, in front of the replay
                    t0 = time.perf_counter()
                    item = ready_q.get()
                    t_wait_in += time.perf_counter() - t0
                    if item is None or err:
                        stop = True
                        break
                    det.pcms[j].copy_(slots[item[1]][0], non_blocking=True)
                    group.append(item)
                if not group:
                    break
                det.replay()                                    # a lane without a batch (odd tail) recomputes its previous input: ignored
                for j, (i, s, cnt) in enumerate(group):
                    slots[s][1].copy_(det.dets[j], non_blocking=True)
                    slots[s][2].copy_(det.n_dets[j], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(det.stream)
                inflight.append((group, ev))
                k += len(group)
                if len(inflight) >= 2:             # the GPU has the next group queued: now wait for the previous one
                    g0, e0 = inflight.pop(0)
                    e0.synchronize()
                    for it in g0:
                        done_q.put(it)
            for g0, e0 in inflight:
                e0.synchronize()
                for it in g0:
                    done_q.put(it)
    finally:
        done_q.put(None)
        free_q.put(None)                            # unblocks a reader that waits for a slot after an error
        th_w.join()
        th_r.join(timeout=5)
        if own_det:                                 # graph, static buffers and the extra lanes' scratch (tens of GB at B = 64) go now,
            torch.cuda.synchronize()                # not whenever the caller's frame dies: the per-file driver may run right behind this
            det.close()
    if err:
        raise err[0]
    if stats is not None:
        stats.update(wall_s=time.perf_counter() - t_start, reader_busy_s=t_read[0], writer_busy_s=t_write[0],
                     gpu_loop_waited_for_input_s=t_wait_in, batches=n_batches, depth=depth, lanes=lanes)
    return out


# =========================================================================== multi-window recordings
# The per-file driver (`run_detection`) makes one model call per group of `bs` windows of one file.  The recording route runs the
# same calls as SEGMENTS of one graph-replayed launch of `batch` windows: segment k of a file = its windows [k*bs, (k+1)*bs), the
# proposal counts (and the transformer head's attention) coupled within the segment only (`NbmModel.detect_calls`), so every window comes out as the
# per-file driver's call computes it, while windows of several files fill one launch.


class SegmentPacker:
    """Packs the segments of successive files into replays of `batch` window slots.  A segment (one model call of the per-file
    driver: windows [k*bs, min((k+1)*bs, n_img)) of a file) is never split across two replays; a replay that cannot take the
    next segment whole is closed and its free slots padded.  Replays are lists of (file key, first window, window count)."""

    def __init__(self, batch, bs):
        if bs < 1 or batch < bs:
            raise ValueError(f'a replay of {batch} windows cannot hold a segment of {bs}: the recording route needs batch >= bs')
        self.batch, self.bs = int(batch), int(bs)
        self.cur, self.fill = [], 0

    def add(self, key, n_img):
        """-> the replays that became full while the file's segments were placed."""
        full = []
        for w0 in range(0, n_img, self.bs):
            n = min(self.bs, n_img - w0)
            if self.fill + n > self.batch:
                full.append(self.cur)
                self.cur, self.fill = [], 0
            self.cur.append((key, w0, n))
            self.fill += n
        return full

    def flush(self):
        """-> [the last, partly filled replay] or []."""
        out = [self.cur] if self.cur else []
        self.cur, self.fill = [], 0
        return out

    @staticmethod
    def segment_sizes(replay, batch):
        """Segment sizes of a replay in slot order, every padding slot a segment of its own."""
        sizes = [n for _, _, n in replay]
        return sizes + [1] * (batch - sum(sizes))


class RecordingDetector(GraphedDetector):
    """Captures `window-table gather -> model.detect(..., segments=...)` for a fixed (batch, min_score) and replays it.

    Static graph inputs: `table` (int64 [batch, ops.WINDOW_ENTRY_WORDS], one `ops.window_entry` per slot: the dB plane, min/max,
    last-window columns and window index of a file; zero rows are padding) and `seg` (the int32 [2, batch] segment table, rewritten
before every replay: a tensor of its own, never one of the shared `ops.batch_segments` tables).  The
    planes are ordinary device tensors whose addresses travel in the table, so windows of files of any length share a replay
    without an image tensor per file.  One stream, no forked branches (one lane): the HIP runtime has been seen to crash
    replaying graphs with parallel branches.  Census check, lane claim and hold rules are GraphedDetector's."""

    def __init__(self, model, batch, min_score=0.2, nms_thresh=0.3, device='cuda'):
        from . import ops
        self.table = torch.zeros((int(batch), ops.WINDOW_ENTRY_WORDS), dtype=torch.int64, device=device)
        self.seg = ops.segment_table([1] * int(batch), device)
        self._start(model, int(batch), 1, device, min_score, nms_thresh)

    def _run(self, k=0):
        from . import ops
        fe = self.fe
        imgs = ops.spec_windows_table(self.table, fe.H_PIX, fe.W_PIX, fe.HOP_SPECTRO)
        return self.model.detect_calls(imgs[:, None], self.seg, self.nms_thresh, self.min_score)

    def close(self):
        super().close()
        self.table = self.seg = None


# Payload bytes the reader of the recording route may have read and not yet handed to the main thread.  A limit on reading
# ahead, not on pinned memory: a buffer the main thread has taken stays busy until its queued H2D copy has run (the main thread
# is at most 3 replays ahead of the GPU), and torch's host allocator keeps freed pinned blocks for reuse.
RECORDING_AHEAD_BYTES = 4 << 30


def detect_recordings(model, files, batch=64, bs=4, min_score=0.2, bird_dict=None, write_txt=True, keep_results=True,
                      stats=None, detector=None, depth=4, ahead_bytes=RECORDING_AHEAD_BYTES):
    """Detects over recordings of any number of windows, in any format the device decoder takes and at any sample rate
    (`WavInfo.recording`), through one captured graph:
    -> list of per-file output dicts in `files` order, each exactly `run_detection(model, cfg, f, ..., bs=bs)`'s (None for
    keep_results=False and for rejected files); `<wav>.txt = str(dict)` written when `write_txt`.

        reader thread   wav payload bytes -> pinned uint8 buffer, undecoded (`read_payload`; at most `depth` files and
                        `ahead_bytes` bytes ahead of the main thread, one file always allowed)
        main thread     per file: H2D of the bytes, `ops.wav_decode` (mono PCM16 at 22.05 / 44.1 kHz: the bytes ARE the int16
                        row of the exact-integer front end), spectrogram_db + column map on the graph's stream; its segments go
                        to the SegmentPacker;
                        per full replay: window / segment tables H2D -> replay -> the slots' rows D2D into each file's row
                        buffer; per finished file: merge_device_async + D2H into pinned memory, an event behind it
        writer thread   waits for a file's event -> dict -> txt

    Everything the GPU does runs on one stream in issue order, so a dB plane or row buffer released by the host after its
    last use is only handed out again to work queued behind that use.  At most 3 replays are in flight.
    A file whose format the decoder does not take (or whose front end refuses it, e.g. for its length) is skipped and listed
    in stats['rejected'] for the per-file driver.  `stats` (dict) also receives counts and stage times.  `detector`: a
    RecordingDetector to reuse (same batch / min_score)."""
    from . import ops
    from .run_detection import merge_device_async, rows_to_output, species_names
    from types import SimpleNamespace
    if not files:
        if stats is not None:
            stats.update(files=0, windows=0, replays=0, padded_slots=0, shared_replays=0, rejected=[])
        return []
    check_head_segment(model, bs, 'windows per model call (--batch)')
    packer = SegmentPacker(batch, bs)
    det = detector or RecordingDetector(model, batch, min_score=min_score)
    own_det = detector is None
    if det.batch != batch or det.min_score != min_score:
        raise ValueError('the RecordingDetector handed in was captured for another batch / min_score')
    fe, stream, num_classes = det.fe, det.stream, model.args.num_classes
    names = species_names(bird_dict or {})
    out = [None] * len(files)
    rejected, err = [], []
    read_q, done_q = queue.Queue(maxsize=max(1, depth)), queue.Queue()
    t_read, t_write = [0.0], [0.0]
    stop = threading.Event()
    room = threading.Condition()
    held = [0]                                     # payload bytes read and not yet taken over by the main thread

    def reader():
        try:
            for i, f in enumerate(files):
                if stop.is_set():
                    break
                t0 = time.perf_counter()
                try:
                    info = WavInfo.probe(f)
                    if not info.decodable:
                        raise ValueError(f'{f}: format tag {info.fmt[0]}, {info.fmt[1]} bits, {info.fmt[2]} channels, {info.sr} Hz, '
                                         f'{info.n} frames is not a recording the route takes')
                    nbytes = info.nbytes
                    t_read[0] += time.perf_counter() - t0
                    with room:                     # one file may always be held, whatever its size
                        while held[0] and held[0] + nbytes > ahead_bytes and not stop.is_set():
                            room.wait(0.05)
                        held[0] += nbytes
                    t0 = time.perf_counter()
                    try:
                        try:
                            pin = torch.empty((1, nbytes), dtype=torch.uint8, pin_memory=True)
                        except RuntimeError as exc:           # no pinned memory of that size: the per-file driver reads the file
                            raise OSError(f'{f}: {exc}') from None
                        fmt, sr, n, _ = read_payload(info, pin.numpy()[0])
                    except BaseException:
                        with room:
                            held[0] -= nbytes
                        raise
                except (OSError, ValueError, NotImplementedError, struct.error):
                    rejected.append(f)
                    continue
                finally:
                    t_read[0] += time.perf_counter() - t0
                read_q.put((i, pin, fmt, sr, n))
        except BaseException as exc:                 # noqa: BLE001 -- handed to the main thread
            err.append(exc)
        finally:
            read_q.put(None)

    def writer():
        try:
            while True:
                item = done_q.get()
                if item is None:
                    return
                i, host, ev = item
                ev.synchronize()
                t0 = time.perf_counter()
                res = rows_to_output(ops.unpack_merged(host), num_classes, names)
                if keep_results:
                    out[i] = res
                if write_txt:
                    write_result(files[i], res)
                t_write[0] += time.perf_counter() - t0
        except BaseException as exc:                 # noqa: BLE001
            err.append(exc)

    live = {}              # file index -> dict(fp, rows, n, left, keep = tensors the queued work reads)
    inflight = []
    n_rep, n_pad, n_win, n_files, n_shared = 0, 0, 0, 0, 0
    t_fe, t_wait = 0.0, 0.0
    cap = det.det.shape[1]

    def launch(replay):
        nonlocal n_rep, n_pad, n_shared
        n_shared += len({key for key, _, _ in replay}) > 1
        table = np.zeros((batch, ops.WINDOW_ENTRY_WORDS), dtype=np.int64)
        slot = 0
        for key, w0, n in replay:
            r = live[key]
            for w in range(w0, w0 + n):
                table[slot] = ops.window_entry(r['db'], r['mm'], r['cols'], w, r['n_img'])
                slot += 1
        n_pad += batch - slot
        det.table.copy_(torch.from_numpy(table).pin_memory(), non_blocking=True)
        det.seg.copy_(ops.segment_table(SegmentPacker.segment_sizes(replay, batch), 'cpu').pin_memory(), non_blocking=True)
        det.replay()
        slot = 0
        for key, w0, n in replay:
            r = live[key]
            r['rows'][w0:w0 + n].copy_(det.det[slot:slot + n])
            r['n'][w0:w0 + n].copy_(det.n_det[slot:slot + n])
            slot += n
            r['left'] -= n
            if r['left'] == 0:
                finish(key)
        ev = torch.cuda.Event()
        ev.record(stream)
        inflight.append(ev)
        n_rep += 1

    def finish(key):
        r = live.pop(key)
        fp = SimpleNamespace(W_PIX=fe.W_PIX, HOP_SPECTRO=fe.HOP_SPECTRO, spectrogram_length=r['L'])
        buf = merge_device_async(fp, r['rows'], r['n'], num_classes)
        host = torch.empty(buf.shape, dtype=buf.dtype, pin_memory=True)
        host.copy_(buf, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(stream)
        done_q.put((key, host, ev))

    th_r, th_w = threading.Thread(target=reader, daemon=True), threading.Thread(target=writer, daemon=True)
    t_start = time.perf_counter()
    th_r.start(), th_w.start()
    try:
        with torch.no_grad(), torch.cuda.stream(stream):
            while not err:
                t0 = time.perf_counter()
                item = read_q.get()
                t_wait += time.perf_counter() - t0
                if item is None:
                    break
                i, pin, fmt, sr, n = item
                t0 = time.perf_counter()
                raw = pin.to('cuda', non_blocking=True)
                with room:
                    held[0] -= pin.shape[1]
                    room.notify()
                del pin
                try:
                    x = raw.view(torch.int16) if is_pcm16_mono(fmt, sr) else ops.wav_decode(raw, *fmt, n)
                    del raw
                    db, mm, Ls = fe.spectrogram_db(x, sr)
                    del x
                except (ValueError, NotImplementedError):      # e.g. a length the reference's chunked STFT fails on
                    rejected.append(files[i])
                    continue
                L = int(sum(Ls))
                n_img, cols = fe.last_window_columns(Ls)
                live[i] = dict(db=db[0], mm=mm[0], cols=cols, n_img=n_img, L=L, left=n_img,
                               rows=torch.empty((n_img, cap, 6), device=db.device, dtype=torch.float32),
                               n=torch.empty((n_img,), device=db.device, dtype=torch.int32))
                n_win += n_img
                n_files += 1
                t_fe += time.perf_counter() - t0
                for replay in packer.add(i, n_img):
                    launch(replay)
                    while len(inflight) > 2:                   # keep the host at most 3 replays ahead of the GPU
                        inflight.pop(0).synchronize()
            if not err:
                for replay in packer.flush():
                    launch(replay)
    finally:
        stop.set()
        while th_r.is_alive():                                # unblock a reader waiting for room in the queue
            try:
                read_q.get_nowait()
            except queue.Empty:
                pass
            th_r.join(timeout=0.05)
        done_q.put(None)
        th_w.join()
        if own_det:
            torch.cuda.synchronize()
            det.close()
    if err:
        raise err[0]
    if stats is not None:
        stats.update(files=n_files, windows=n_win, replays=n_rep, padded_slots=n_pad, shared_replays=n_shared, rejected=sorted(rejected),
                     wall_s=time.perf_counter() - t_start, reader_busy_s=t_read[0], writer_busy_s=t_write[0],
                     front_end_host_s=t_fe, main_waited_for_reader_s=t_wait, batch=batch, bs=bs)
    return out
