"""GPU: the attention kernels of the transformer head at head dims above 64 (csrc/mha.hip, "wide heads": 64-column chunks of K and
V through LDS) -- forward and backward with and without dropout against float64 with the mask injected, segments against
`ops.mha_small` bit for bit, the limit hd <= 512, and the narrow kernels (hd <= 64) untouched by a wide launch in the same process.
Inputs are `synth.normal` draws; nothing here uses torch's generator."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from birdsoundclassif_amd import ops                            # noqa: E402
from birdsoundclassif_amd._lib import NbmHipError               # noqa: E402
from birdsoundclassif_amd.nets import functional as Fn          # noqa: E402
from test_gpu_tf_dropout_kernels import SEED, attention_f64, close, rnd   # noqa: E402

HEADS = {65: (65, 1), 128: (256, 2), 129: (129, 1), 192: (384, 2), 512: (512, 1)}          # hd -> (E, NH)
GEOMS = [(True, 128, 2, None), (False, 65, 2, 37), (False, 3, 3, 3), (True, 1, 2, None)]   # (seq_major, S, N, n_valid)
CASES = [(hd, g) for hd in (128, 512) for g in GEOMS] + [(hd, g) for hd in (65, 129, 192) for g in GEOMS[:2]]


def attention_f32(qkv, go, seq_major, S, N, n_use, keep, scale, NH):
    """`attention_f64` restated in float32 torch on the CPU: what a float32 implementation with torch's blocked sums gives."""
    E = go.shape[1]
    HD = E // NH
    qkv = qkv.float().requires_grad_(True)
    t = qkv.view(S, N, 3 * E) if seq_major else qkv.view(N, S, 3 * E).transpose(0, 1)
    q, k, v = (t[..., i * E:(i + 1) * E].reshape(S, N * NH, HD).transpose(0, 1) for i in range(3))
    prob = torch.softmax((q[:, :n_use] @ k[:, :n_use].transpose(1, 2)) * np.float32(1.0 / np.sqrt(HD)), -1)
    m = keep.view(N * NH, S, S)[:, :n_use, :n_use]
    att = torch.where(m, prob * np.float32(scale), torch.zeros_like(prob)) @ v[:, :n_use]
    out = att.transpose(0, 1).reshape(n_use, N, E)
    g = go.float().view(S, N, E) if seq_major else go.float().view(N, S, E).transpose(0, 1)
    out.backward(g[:n_use])
    return out.detach(), qkv.grad


def rel_err(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).abs().max()) / (float(ref.abs().max()) + 1e-12)


def bounded(got, ref, tol, name, restated):
    """The project's bound `tol` (relative to the largest reference value); a case that misses it is held to 4 x the error of the
    float32 torch restatement of the same inputs (`restated()`): 4 covers a sequential 512-term sum against torch's blocked one."""
    err = rel_err(got, ref)
    if err <= tol:
        print(f'{name}: relative error {err:.3e} (bound {tol:.1e})')
        return
    e32 = rel_err(restated(), ref)
    print(f'{name}: relative error {err:.3e} misses {tol:.1e}; float32 torch restatement {e32:.3e}, bound {4 * e32:.3e}')
    assert err <= 4 * e32, f'{name}: {err:.3e} vs 4 x {e32:.3e}'


def _valid_rows(seq_major, S, N, n_use):
    valid = torch.zeros(S, N, 1)
    valid[:n_use] = 1
    return (valid if seq_major else valid.transpose(0, 1)).reshape(S * N, 1)


@pytest.mark.parametrize('p', [0.0, 0.5])
@pytest.mark.parametrize('hd,geom', CASES)
def test_wide_heads_forward_and_backward_against_float64(hd, geom, p):
    """3e-6 forward and 3e-5 gradients relative to the largest reference value, the bounds of the hd = 64 tests
    (tests/test_gpu_tf_dropout_kernels.py); rows >= n_valid are exactly zero, outputs and gradients."""
    (E, NH), (seq_major, S, N, nv) = HEADS[hd], geom
    call, site = 4, 8
    qkv = torch.from_numpy(rnd(('mhawide', hd, seq_major, S), S * N, 3 * E))
    go = torch.from_numpy(rnd(('mhawideg', hd, seq_major, S), S * N, E))
    n_use = S if nv is None else nv
    if p:
        keep = torch.from_numpy(ops.dropout_keep_reference(SEED, call, site, N * NH * S * S, p)).view(N, NH, S, S)
        scale = ops.dropout_params(p)[1]
    else:
        keep, scale = torch.ones(N, NH, S, S, dtype=torch.bool), 1.0
    ref, gref = attention_f64(qkv, go, seq_major, S, N, n_use, keep, scale, NH)
    memo = []

    def f32(i):
        if not memo:
            memo.append(attention_f32(qkv, go, seq_major, S, N, n_use, keep, scale, NH))
        return memo[0][i]

    qd = qkv.cuda().requires_grad_(True)
    cnt = None if nv is None else torch.tensor([nv], dtype=torch.int32, device='cuda')
    ss, bs = (N, 1) if seq_major else (1, S)
    q, k, v = qd[:, :E], qd[:, E:2 * E], qd[:, 2 * E:]
    out = Fn.MhaSmallDrop.apply(q, k, v, S, N, NH, ss, bs, cnt, p, SEED, call, site) if p else Fn.MhaSmall.apply(q, k, v, S, N, NH, ss, bs, cnt)
    got = out.view(S, N, E) if seq_major else out.view(N, S, E).transpose(0, 1)
    bounded(got[:n_use], ref, 3e-6, f'hd {hd} p {p} fwd', lambda: f32(0))
    valid = _valid_rows(seq_major, S, N, n_use)
    out.backward((go * valid).cuda())
    bounded(qd.grad, gref, 3e-5, f'hd {hd} p {p} dqkv', lambda: f32(1))
    assert torch.isfinite(out).all() and torch.isfinite(qd.grad).all()
    if (valid == 0).any():
        assert float(qd.grad.cpu()[valid[:, 0] == 0].abs().max()) == 0.0
        assert float(out.detach().cpu()[valid[:, 0] == 0].abs().max()) == 0.0


def test_wide_heads_repeat_bit_for_bit():
    """hd = 128: the same (seed, call, site) twice gives the same bits, forward and backward, with and without dropout."""
    (E, NH), (S, N, nv), p = HEADS[128], (65, 2, 37), 0.5
    qkv = torch.from_numpy(rnd('mhawiderep', S * N, 3 * E)).cuda()
    go = torch.from_numpy(rnd('mhawiderepg', S * N, E)).cuda()
    cnt = torch.tensor([nv], dtype=torch.int32, device='cuda')
    q, k, v = qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:]
    runs = []
    for _ in range(2):
        runs.append([ops.mha_small(q, k, v, S, N, NH, 1, S, cnt), ops.mha_small_drop(q, k, v, S, N, NH, 1, S, cnt, p, SEED, 3, 4),
                     *ops.mha_small_bwd(q, k, v, go, S, N, NH, 1, S, cnt),
                     *ops.mha_small_drop_bwd(q, k, v, go, S, N, NH, 1, S, cnt, p, SEED, 3, 4)])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert not torch.equal(runs[0][0], runs[0][1])
    assert not torch.equal(ops.mha_small_drop(q, k, v, S, N, NH, 1, S, cnt, p, SEED, 4, 4), runs[0][1])     # another call, another mask


def test_wide_mha_small_drop_with_threshold_0_is_mha_small():
    """The two forms round differently (e / sum before or after the product with V), as at hd = 64: 3e-6."""
    p = 1e-12
    assert ops.dropout_params(p) == (0, 1.0)
    (E, NH), (S, N, nv) = HEADS[128], (65, 2, 37)
    qkv = torch.from_numpy(rnd('mhawide0', S * N, 3 * E)).cuda()
    cnt = torch.tensor([nv], dtype=torch.int32, device='cuda')
    q, k, v = qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:]
    close(ops.mha_small_drop(q, k, v, S, N, NH, 1, S, cnt, p, SEED, 0, 0), ops.mha_small(q, k, v, S, N, NH, 1, S, cnt), 3e-6, 'thr 0')


SEGMENTS = [(128, [1] * 8, [50, 0, 37, 1, 50, 12, 3, 49]), (128, [4, 4, 3, 1, 2], [37, 0, 50, 5, 1]), (128, [64], [41]),
            (512, [4, 1], [5, 3])]


@pytest.mark.parametrize('mode', [ops.MHA_ACROSS_ROIS, ops.MHA_ACROSS_IMAGES])
@pytest.mark.parametrize('hd,sizes,counts', SEGMENTS)
def test_wide_mha_segments_is_mha_small_on_each_segment(hd, sizes, counts, mode):
    """Segments of 1 .. 64 images (the wave-local branch up to 8 images and the workgroup one) and 0 .. 50 RoIs of 50 slots: every
    valid row holds the bits `ops.mha_small` gives on its segment alone, every other row is zero."""
    (E, NH), R = HEADS[hd], 50 if hd == 128 else 5
    qkv = torch.from_numpy(rnd(('mhawideseg', hd, len(sizes)), sum(sizes) * R, 3 * E)).cuda()
    n_roi = torch.tensor(np.repeat(counts, sizes), dtype=torch.int32, device='cuda')
    out = ops.mha_segments(qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:], R, NH, mode, ops.segment_table(sizes), n_roi)
    s = 0
    for m, n in zip(sizes, counts):
        part = qkv[s * R:(s + m) * R]
        q, k, v = part[:, :E], part[:, E:2 * E], part[:, 2 * E:]
        if mode == ops.MHA_ACROSS_ROIS:                            # m sequences of the image's n RoIs
            ref = ops.mha_small(q, k, v, R, m, NH, 1, R, torch.tensor([n], dtype=torch.int32, device='cuda'))
        else:                                                      # R sequences of the segment's m images, n of them real
            ref = ops.mha_small(q, k, v, m, R, NH, R, 1)
        ok = (torch.arange(m * R, device='cuda') % R) < n
        assert torch.equal(out[s * R:(s + m) * R][ok], ref[ok]), (s, m, n)
        assert not out[s * R:(s + m) * R][~ok].any()
        s += m
    assert torch.isfinite(out).all()


def test_head_dim_513_is_refused_by_every_entry_point():
    """NBM_EINVAL and nothing launched: NaN-filled outputs stay NaN.  hd = 512 with the same buffers is accepted.  The segmented
    entry point for these head dims is `nbm_mha_segments_wide` (what `ops.mha_segments` calls); `nbm_mha_segments` keeps refusing
    everything above 64, which tests/test_gpu_tf_segments.py pins at hd = 128."""
    S, N = 2, 1
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    lib, thr, scale = ops.lib(), *ops.dropout_params(0.5)
    qkv = torch.from_numpy(rnd('mha513', S * N, 3 * 513)).cuda()
    go = torch.from_numpy(rnd('mha513g', S * N, 513)).cuda()
    table = ops.segment_table([1, 1])
    n_roi = torch.ones(2, dtype=torch.int32, device='cuda')
    for hd, want in ((513, -1), (512, 0)):
        outs = [torch.full((S * N, 513), float('nan'), device='cuda') for _ in range(9)]
        ws = torch.empty((N, 2, S, S), device='cuda')
        x, ld = (p(qkv),) * 3, (3 * 513,) * 3
        rcs = [lib.nbm_mha_small(*x, *ld, p(outs[0]), 513, S, N, 1, hd, 1, S, None, 0.05, None),
               lib.nbm_mha_small_drop(*x, *ld, p(outs[1]), 513, S, N, 1, hd, 1, S, None, 0.05, thr, scale, SEED, 0, 0, None),
               lib.nbm_mha_small_bwd(*x, p(go), *ld, 513, p(outs[2]), p(outs[3]), p(outs[4]), 513, 513, 513, p(ws), S, N, 1, hd, 1, S,
                                     None, 0.05, None),
               lib.nbm_mha_small_drop_bwd(*x, p(go), *ld, 513, p(outs[5]), p(outs[6]), p(outs[7]), 513, 513, 513, p(ws), S, N, 1, hd, 1,
                                          S, None, 0.05, thr, scale, SEED, 0, 0, None),
               lib.nbm_mha_segments_wide(*x, *ld, p(outs[8]), 513, 2, 1, 1, hd, ops.MHA_ACROSS_IMAGES, p(table), p(n_roi), 2, 0.05,
                                         None)]
        torch.cuda.synchronize()
        assert rcs == [want] * 5, (hd, rcs)
        for o in outs:
            assert bool(torch.isnan(o[:, :hd]).all()) == (hd == 513)
        old = torch.full((S * N, 513), float('nan'), device='cuda')
        assert lib.nbm_mha_segments(*x, *ld, p(old), 513, 2, 1, 1, hd, ops.MHA_ACROSS_IMAGES, p(table), p(n_roi), 2, 0.05, None) == -1
        torch.cuda.synchronize()
        assert bool(torch.isnan(old).all())
    q1 = torch.zeros((4, 1026), device='cuda')
    for call in (lambda: ops.mha_small(q1, q1, q1, 2, 2, 2, 2, 1),
                 lambda: ops.mha_small_bwd(q1, q1, q1, q1, 2, 2, 2, 2, 1),
                 lambda: ops.mha_small_drop(q1, q1, q1, 2, 2, 2, 2, 1, None, 0.5, SEED, 0, 0),
                 lambda: ops.mha_small_drop_bwd(q1, q1, q1, q1, 2, 2, 2, 2, 1, None, 0.5, SEED, 0, 0),
                 lambda: ops.mha_segments(q1, q1, q1, 2, 2, ops.MHA_ACROSS_ROIS, table, n_roi)):
        with pytest.raises(NbmHipError, match='NBM_EINVAL'):
            call()


@pytest.mark.parametrize('E,NH', [(512, 8), (96, 4)])
def test_narrow_heads_are_untouched_by_a_wide_launch(E, NH):
    """hd = 64 and hd = 24: `ops.mha_small` / `ops.mha_small_bwd` give the same bits before and after the wide kernels have run in
    this process (shared LDS, attribute state).  That these are the parent's bits is what the golden and segment tests hold."""
    S, N, nv = 50, 3, 37
    qkv = torch.from_numpy(rnd(('mhanarrow', E), S * N, 3 * E)).cuda()
    go = torch.from_numpy(rnd(('mhanarrowg', E), S * N, E)).cuda()
    cnt = torch.tensor([nv], dtype=torch.int32, device='cuda')
    q, k, v = qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:]
    before = ops.mha_small(q, k, v, S, N, NH, 1, S, cnt)
    gbefore = torch.cat(ops.mha_small_bwd(q, k, v, go, S, N, NH, 1, S, cnt), 1)
    WE, WNH = HEADS[128]
    w = torch.from_numpy(rnd('mhanarroww', S * N, 3 * WE)).cuda()
    wide = ops.mha_small(w[:, :WE], w[:, WE:2 * WE], w[:, 2 * WE:], S, N, WNH, 1, S, cnt)
    ops.mha_small_drop_bwd(w[:, :WE], w[:, WE:2 * WE], w[:, 2 * WE:], wide, S, N, WNH, 1, S, cnt, 0.5, SEED, 0, 0)
    assert torch.isfinite(wide).all()
    assert torch.equal(ops.mha_small(q, k, v, S, N, NH, 1, S, cnt), before)
    assert torch.equal(torch.cat(ops.mha_small_bwd(q, k, v, go, S, N, NH, 1, S, cnt), 1), gbefore)
