"""GPU: the attention kernels of the transformer head at sequences of 129 .. 1 024 tokens (csrc/mha.hip, "long sequences": K and V
through LDS in blocks of 128 keys, the score rows of 8 queries in LDS, a plain softmax over the whole row) -- forward and backward
with and without dropout against float64 with the mask injected, the kept set against `ops.dropout_keep_reference`, segments
against `ops.mha_small` bit for bit, the limit S <= 1 024, and the short kernels untouched by long launches in the same process.
Inputs are `synth.normal` draws; nothing here uses torch's generator.

Bounds: the project's (3e-6 forward, 3e-5 gradients, relative to the largest reference value) or, where larger, 3 x the error float32
torch on the CPU makes on the same inputs against the same float64 reference -- a sequential fmaf chain over up to 1 024 keys
accumulates its roundings linearly where torch's blocked sums do not.  Both errors are printed for every case."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tf_segments_ref as TS                                    # noqa: E402
from birdsoundclassif_amd import ops                            # noqa: E402
from birdsoundclassif_amd._lib import NbmHipError               # noqa: E402
from birdsoundclassif_amd.nets import functional as Fn          # noqa: E402
from test_gpu_mha_head_dims import attention_f32, rel_err       # noqa: E402
from test_gpu_tf_dropout_kernels import SEED, attention_f64, close, rnd   # noqa: E402

HEADS = {24: (96, 4), 64: (128, 2), 65: (65, 1), 128: (256, 2), 512: (512, 1)}          # hd -> (E, NH); 65, 128, 512 as the wide tests
# (hd, seq_major, S, N, n_valid): a covering subset of S x head dim x n_valid, not the cross product -- every S meets every head dim
# below 512 and every n_valid of {None, 1, 128, 129, S - 1}, every head dim meets every n_valid, both token geometries at every S,
# N = 1 .. 3; hd = 512 at S = 129 only, S = 1 024 at N = 1 and head dims 64 and 128
CASES = [(24, True, 129, 2, None), (64, False, 129, 3, 128), (65, True, 129, 1, 1), (128, False, 129, 2, 129),
         (512, False, 129, 1, 128), (512, True, 129, 2, None), (512, True, 129, 1, 1), (512, False, 129, 2, 129),
         (24, False, 192, 2, 191), (64, True, 192, 2, 129), (65, False, 192, 3, 128), (128, True, 192, 1, 1), (128, False, 192, 2, None),
         (24, True, 257, 1, 256), (64, False, 257, 2, None), (65, True, 257, 2, 129), (128, False, 257, 3, 128), (64, True, 257, 1, 1),
         (64, False, 1024, 1, 1023), (128, True, 1024, 1, None), (64, True, 1024, 1, 129),
         (128, False, 1024, 1, 128), (64, True, 1024, 1, 1)]


def bounded(got, ref, tol, name, restated):
    err, e32 = rel_err(got, ref), rel_err(restated(), ref)
    bound = max(tol, 3 * e32)
    print(f'{name}: relative error {err:.3e}; float32 torch {e32:.3e}; bound {bound:.3e}')
    assert err <= bound, f'{name}: {err:.3e} vs max({tol:.1e}, 3 x {e32:.3e})'


def _valid_rows(seq_major, S, N, n_use):
    valid = torch.zeros(S, N, 1)
    valid[:n_use] = 1
    return (valid if seq_major else valid.transpose(0, 1)).reshape(S * N, 1)


def _split(t, E):
    return t[:, :E], t[:, E:2 * E], t[:, 2 * E:]


@pytest.mark.parametrize('p', [0.0, 0.5])
@pytest.mark.parametrize('hd,seq_major,S,N,nv', CASES)
def test_long_forward_and_backward_against_float64(hd, seq_major, S, N, nv, p):
    """Rows >= n_valid are exactly zero, outputs and gradients; at p = 0.5 the mask of `ops.dropout_keep_reference` is injected into
    the reference, so a single differing mask element (a probability of about 1 / S times a value of V) would miss the bound."""
    assert ops.mha_plan(S, hd).family == 'long'
    (E, NH), call, site = HEADS[hd], 4, 8
    qkv = torch.from_numpy(rnd(('mhalong', hd, seq_major, S), S * N, 3 * E))
    go = torch.from_numpy(rnd(('mhalongg', hd, seq_major, S), S * N, E))
    n_use = S if nv is None else nv
    if p:
        keep = torch.from_numpy(ops.dropout_keep_reference(SEED, call, site, N * NH * S * S, p)).view(N, NH, S, S)
        scale = ops.dropout_params(p)[1]
    else:
        keep, scale = torch.ones(N, NH, S, S, dtype=torch.bool), 1.0
    ref, gref = attention_f64(qkv, go, seq_major, S, N, n_use, keep, scale, NH)
    f32 = attention_f32(qkv.clone(), go, seq_major, S, N, n_use, keep, scale, NH)     # a copy: it turns its float32 argument into a leaf

    qd = qkv.cuda().requires_grad_(True)
    cnt = None if nv is None else torch.tensor([nv], dtype=torch.int32, device='cuda')
    ss, bs = (N, 1) if seq_major else (1, S)
    q, k, v = _split(qd, E)
    out = Fn.MhaSmallDrop.apply(q, k, v, S, N, NH, ss, bs, cnt, p, SEED, call, site) if p else Fn.MhaSmall.apply(q, k, v, S, N, NH, ss, bs, cnt)
    got = out.view(S, N, E) if seq_major else out.view(N, S, E).transpose(0, 1)
    tag = f'S {S} hd {hd} nv {nv} p {p}'
    bounded(got[:n_use], ref, 3e-6, tag + ' fwd', lambda: f32[0])
    valid = _valid_rows(seq_major, S, N, n_use)
    out.backward((go * valid).cuda())
    bounded(qd.grad, gref, 3e-5, tag + ' dqkv', lambda: f32[1])
    assert torch.isfinite(out).all() and torch.isfinite(qd.grad).all()
    if (valid == 0).any():
        assert float(qd.grad.cpu()[valid[:, 0] == 0].abs().max()) == 0.0
        assert float(out.detach().cpu()[valid[:, 0] == 0].abs().max()) == 0.0


@pytest.mark.parametrize('seq_major,nv', [(False, None), (True, 150)])
def test_long_dropout_keeps_the_reference_set(seq_major, nv):
    """V = one-hot rows (hd = S = 192, one head): out[r][j] is the dropped probability of (r, j), positive where kept and zero where
    dropped -- the zero pattern is the mask of a dense [N, 1, S, S] tensor with the launch's S, whatever n_valid."""
    S, N, E, p, call, site = 192, 2, 192, 0.5, 7, 5
    qk = torch.from_numpy(rnd(('mhalongkeep', seq_major), S * N, 2 * E)).cuda()
    eye = torch.eye(S, device='cuda')
    v = (eye[:, None, :].expand(S, N, E) if seq_major else eye[None].expand(N, S, E)).reshape(S * N, E).contiguous()
    cnt = None if nv is None else torch.tensor([nv], dtype=torch.int32, device='cuda')
    ss, bs = (N, 1) if seq_major else (1, S)
    out = ops.mha_small_drop(qk[:, :E], qk[:, E:], v, S, N, 1, ss, bs, cnt, p, SEED, call, site)
    got = (out.view(S, N, E).transpose(0, 1) if seq_major else out.view(N, S, E)).cpu()       # [N, r, j]
    keep = torch.from_numpy(ops.dropout_keep_reference(SEED, call, site, N * S * S, p)).view(N, S, S).clone()
    n_use = S if nv is None else nv
    keep[:, n_use:] = False
    keep[:, :, n_use:] = False
    assert torch.equal(got > 0, keep) and bool((got >= 0).all())
    assert 0.45 < float(keep[:, :n_use, :n_use].float().mean()) < 0.55


def test_long_kernels_repeat_bit_for_bit():
    """The same (seed, call, site) twice gives the same bits, forward and backward, with and without dropout: no atomics."""
    (E, NH), (S, N, nv), p = HEADS[128], (257, 2, 200), 0.5
    qkv = torch.from_numpy(rnd('mhalongrep', S * N, 3 * E)).cuda()
    go = torch.from_numpy(rnd('mhalongrepg', S * N, E)).cuda()
    cnt = torch.tensor([nv], dtype=torch.int32, device='cuda')
    q, k, v = _split(qkv, E)
    runs = []
    for _ in range(2):
        runs.append([ops.mha_small(q, k, v, S, N, NH, 1, S, cnt), ops.mha_small_drop(q, k, v, S, N, NH, 1, S, cnt, p, SEED, 3, 4),
                     *ops.mha_small_bwd(q, k, v, go, S, N, NH, 1, S, cnt),
                     *ops.mha_small_drop_bwd(q, k, v, go, S, N, NH, 1, S, cnt, p, SEED, 3, 4)])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert not torch.equal(runs[0][0], runs[0][1])
    assert not torch.equal(ops.mha_small_drop(q, k, v, S, N, NH, 1, S, cnt, p, SEED, 4, 4), runs[0][1])     # another call, another mask


@pytest.mark.parametrize('hd', [64, 128])
def test_long_mha_small_drop_with_threshold_0_is_mha_small(hd):
    """The two forms round differently (e / sum before or after the product with V), as in the short kernels: 3e-6."""
    p = 1e-12
    assert ops.dropout_params(p) == (0, 1.0)
    (E, NH), (S, N, nv) = HEADS[hd], (192, 2, 150)
    qkv = torch.from_numpy(rnd(('mhalong0', hd), S * N, 3 * E)).cuda()
    cnt = torch.tensor([nv], dtype=torch.int32, device='cuda')
    q, k, v = _split(qkv, E)
    close(ops.mha_small_drop(q, k, v, S, N, NH, 1, S, cnt, p, SEED, 0, 0), ops.mha_small(q, k, v, S, N, NH, 1, S, cnt), 3e-6, 'thr 0')


R_LONG = 160
ROI_LAYOUTS = [(64, [1] * 8, [0, 1, 128, 129, 160, 37, 160, 5]), (128, [3, 2, 1, 2], [129, 0, 160, 1])]


@pytest.mark.parametrize('hd,sizes,counts', ROI_LAYOUTS)
def test_mha_segments_across_rois_with_160_slots_is_mha_small_on_each_image(hd, sizes, counts):
    """Every valid row holds the bits `ops.mha_small(q, k, v, R, m, NH, 1, R, n)` gives on its segment's images alone (the long
    kernels, S = R = 160, whatever the count), every other row is zero; and the rows agree with the float64 statement of the groups."""
    (E, NH), R = HEADS[hd], R_LONG
    qkv = torch.from_numpy(rnd(('mhalongseg', hd), sum(sizes) * R, 3 * E)).cuda()
    n_roi = torch.tensor(np.repeat(counts, sizes), dtype=torch.int32, device='cuda')
    out = ops.mha_segments(*_split(qkv, E), R, NH, ops.MHA_ACROSS_ROIS, ops.segment_table(sizes), n_roi)
    s = 0
    for m, n in zip(sizes, counts):
        ref = ops.mha_small(*_split(qkv[s * R:(s + m) * R], E), R, m, NH, 1, R, torch.tensor([n], dtype=torch.int32, device='cuda'))
        ok = (torch.arange(m * R, device='cuda') % R) < n
        assert torch.equal(out[s * R:(s + m) * R][ok], ref[ok]), (s, m, n)
        assert not out[s * R:(s + m) * R][~ok].any()
        s += m
    assert torch.isfinite(out).all()
    groups = TS.token_groups(TS.ACROSS_ROIS, TS.table_of(sizes), TS.image_counts(sizes, counts), R)
    q, k, v = (t.cpu().numpy() for t in _split(qkv, E))
    close(out, torch.from_numpy(TS.attention_f64(q, k, v, groups, NH)), 3e-6, 'segments vs float64')


def test_mha_segments_across_images_with_160_slots_keeps_the_short_kernels():
    """ACROSS_IMAGES: the sequence is a segment's images (<= 128), the 160 slots are batch entries -- `ops.mha_small` on each segment
    with S = its images, bit for bit, at a narrow and a wide head dim."""
    for hd, sizes, counts in ((64, [4, 1, 3], [160, 129, 37]), (128, [9, 2], [130, 160])):
        (E, NH), R = HEADS[hd], R_LONG
        qkv = torch.from_numpy(rnd(('mhalongimg', hd), sum(sizes) * R, 3 * E)).cuda()
        n_roi = torch.tensor(np.repeat(counts, sizes), dtype=torch.int32, device='cuda')
        out = ops.mha_segments(*_split(qkv, E), R, NH, ops.MHA_ACROSS_IMAGES, ops.segment_table(sizes), n_roi)
        s = 0
        for m, n in zip(sizes, counts):
            assert ops.mha_plan(m, hd).family != 'long'
            ref = ops.mha_small(*_split(qkv[s * R:(s + m) * R], E), m, R, NH, R, 1)
            ok = (torch.arange(m * R, device='cuda') % R) < n
            assert torch.equal(out[s * R:(s + m) * R][ok], ref[ok]), (hd, s, m, n)
            assert not out[s * R:(s + m) * R][~ok].any()
            s += m


def test_sequences_of_1025_are_refused_by_every_entry_point():
    """NBM_EINVAL and nothing launched: NaN-filled outputs stay NaN.  S = 1 024 with the same buffers is accepted.  The older symbol
    `nbm_mha_segments` keeps refusing more than 128 slots in ACROSS_ROIS."""
    E, N = 8, 1
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    lib, thr, scale = ops.lib(), *ops.dropout_params(0.5)
    qkv = torch.from_numpy(rnd('mha1025', 1025 * N, 3 * E)).cuda()
    go = torch.from_numpy(rnd('mha1025g', 1025 * N, E)).cuda()
    table = ops.segment_table([1])
    for S, want in ((1025, -1), (1024, 0)):
        n_roi = torch.full((1,), S, dtype=torch.int32, device='cuda')
        outs = [torch.full((1025 * N, E), float('nan'), device='cuda') for _ in range(9)]
        ws = torch.empty((N, 2, 1025, 1025), device='cuda')
        x, ld = (p(qkv),) * 3, (3 * E,) * 3
        rcs = [lib.nbm_mha_small(*x, *ld, p(outs[0]), E, S, N, 1, E, 1, S, None, 0.3, None),
               lib.nbm_mha_small_drop(*x, *ld, p(outs[1]), E, S, N, 1, E, 1, S, None, 0.3, thr, scale, SEED, 0, 0, None),
               lib.nbm_mha_small_bwd(*x, p(go), *ld, E, p(outs[2]), p(outs[3]), p(outs[4]), E, E, E, p(ws), S, N, 1, E, 1, S, None, 0.3,
                                     None),
               lib.nbm_mha_small_drop_bwd(*x, p(go), *ld, E, p(outs[5]), p(outs[6]), p(outs[7]), E, E, E, p(ws), S, N, 1, E, 1, S, None,
                                          0.3, thr, scale, SEED, 0, 0, None),
               lib.nbm_mha_segments_wide(*x, *ld, p(outs[8]), E, 1, S, 1, E, ops.MHA_ACROSS_ROIS, p(table), p(n_roi), 1, 0.3, None)]
        torch.cuda.synchronize()
        assert rcs == [want] * 5, (S, rcs)
        for o in outs:
            assert bool(torch.isnan(o[:S]).all()) == (S == 1025)
            assert bool(torch.isnan(o[S:]).all())
        old = torch.full((1025 * N, E), float('nan'), device='cuda')
        assert lib.nbm_mha_segments(*x, *ld, p(old), E, 1, S, 1, E, ops.MHA_ACROSS_ROIS, p(table), p(n_roi), 1, 0.3, None) == -1
        torch.cuda.synchronize()
        assert bool(torch.isnan(old).all())
    q1 = torch.zeros((1025, 8), device='cuda')
    n1 = torch.ones(1, dtype=torch.int32, device='cuda')
    for call in (lambda: ops.mha_small(q1, q1, q1, 1025, 1, 1, 1, 1025),
                 lambda: ops.mha_small_bwd(q1, q1, q1, q1, 1025, 1, 1, 1, 1025),
                 lambda: ops.mha_small_drop(q1, q1, q1, 1025, 1, 1, 1, 1025, None, 0.5, SEED, 0, 0),
                 lambda: ops.mha_small_drop_bwd(q1, q1, q1, q1, 1025, 1, 1, 1, 1025, None, 0.5, SEED, 0, 0),
                 lambda: ops.mha_segments(q1, q1, q1, 1025, 1, ops.MHA_ACROSS_ROIS, table, n1)):
        with pytest.raises(NbmHipError, match='NBM_EINVAL'):
            call()


@pytest.mark.parametrize('hd,S', [(64, 128), (128, 65)])
def test_short_sequences_are_untouched_by_long_launches(hd, S):
    """hd = 64 at S = 128 (narrow) and hd = 128 at S = 65 (wide): `ops.mha_small`, `ops.mha_small_drop` and both backwards give the
    same bits before and after the long kernels have run in this process (LDS size, attribute state).  That these are the parent's
    bits is what the golden and segment tests hold."""
    (E, NH), N, nv, p = HEADS[hd] if hd != 64 else (512, 8), 3, 37, 0.5
    assert ops.mha_plan(S, hd).family == ('narrow' if hd == 64 else 'wide')
    qkv = torch.from_numpy(rnd(('mhashort', hd), S * N, 3 * E)).cuda()
    go = torch.from_numpy(rnd(('mhashortg', hd), S * N, E)).cuda()
    cnt = torch.tensor([nv], dtype=torch.int32, device='cuda')
    q, k, v = _split(qkv, E)

    def short():
        return [ops.mha_small(q, k, v, S, N, NH, 1, S, cnt), ops.mha_small_drop(q, k, v, S, N, NH, 1, S, cnt, p, SEED, 1, 2),
                *ops.mha_small_bwd(q, k, v, go, S, N, NH, 1, S, cnt), *ops.mha_small_drop_bwd(q, k, v, go, S, N, NH, 1, S, cnt, p, SEED, 1, 2)]

    before = short()
    LS = 200
    w = torch.from_numpy(rnd(('mhashortw', hd), LS * N, 3 * E)).cuda()
    lq, lk, lv = _split(w, E)
    long_out = ops.mha_small(lq, lk, lv, LS, N, NH, 1, LS, cnt)
    ops.mha_small_drop_bwd(lq, lk, lv, long_out, LS, N, NH, 1, LS, cnt, p, SEED, 0, 0)
    ops.mha_segments(lq, lk, lv, LS, NH, ops.MHA_ACROSS_ROIS, ops.segment_table([N]), torch.full((N,), 150, dtype=torch.int32, device='cuda'))
    assert torch.isfinite(long_out).all()
    assert all(torch.equal(a, b) for a, b in zip(short(), before))
