"""GPU: the dropout kernels of the transformer head (csrc/dropout.hip, csrc/mha.hip) against their specification -- `nbm_dropout` bit for bit
against NumPy float32 with the mask of `ops.dropout_keep_reference`, `nbm_mha_small_drop` and its backward against float64 torch
attention with that mask injected on the probabilities.  Deterministic: no statistics, no use of torch's generator."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from birdsoundclassif_amd import ops, synth                     # noqa: E402
from birdsoundclassif_amd._lib import NbmHipError               # noqa: E402
from birdsoundclassif_amd.nets import functional as Fn          # noqa: E402

SEED = 0x5EEDC0FFEE123457


def rnd(key, *shape):
    return synth.normal(key, int(np.prod(shape))).astype(np.float32).reshape(shape)


def bits(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).view(np.uint32)


def expected(x, res, keep, scale):
    """res + where(keep, x * scale, 0) in NumPy float32, one rounding per operation."""
    v = np.where(keep, x * np.float32(scale), np.float32(0))
    return v if res is None else res + v


def raw_dropout(x, res, y, n, p, call, site):
    thr, scale = ops.dropout_params(p)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    return ops.lib().nbm_dropout(ptr(x), ptr(res), ptr(y), n, thr, scale, SEED, call, site, None)


@pytest.mark.parametrize('with_res', [False, True])
@pytest.mark.parametrize('p', [0.1, 0.5])
@pytest.mark.parametrize('n', [4, 12, 1028, 1031])
def test_dropout_bit_for_bit_and_tail(n, p, with_res):
    call, site, pad = 3, 5, 9
    x = rnd(('dropx', n), n)
    res = rnd(('dropr', n), n) if with_res else None
    keep = ops.dropout_keep_reference(SEED, call, site, n, p)
    want = expected(x, res, keep, ops.dropout_params(p)[1])
    xd = torch.from_numpy(x).cuda()
    rd = torch.from_numpy(res).cuda() if with_res else None
    y = torch.full((n + pad,), float('nan'), device='cuda')
    assert raw_dropout(xd, rd, y, n, p, call, site) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(y[:n]), bits(want))
    assert bool(torch.isnan(y[n:]).all())                            # nothing behind element n - 1 is written
    again = ops.dropout(xd, p, SEED, call, site, residual=rd)       # the public wrapper, and the same bits a second time
    assert np.array_equal(bits(again), bits(want))
    if n >= 1028:                                                    # another call, another mask
        assert not np.array_equal(bits(ops.dropout(xd, p, SEED, call + 1, site, residual=rd)), bits(want))


def test_dropout_p0_is_the_identity_and_arguments_are_checked():
    x = torch.from_numpy(rnd('dropid', 1031)).cuda()
    assert torch.equal(ops.dropout(x, 0.0, SEED, 0, 0), x)
    buf = torch.zeros(1040, device='cuda')
    out = torch.zeros(1040, device='cuda')
    assert raw_dropout(buf[1:], None, out, 1028, 0.1, 0, 0) == -2     # NBM_EALIGN: x
    assert raw_dropout(buf, None, out[1:], 1028, 0.1, 0, 0) == -2     # y
    assert raw_dropout(buf, buf[2:], out, 1028, 0.1, 0, 0) == -2      # residual
    assert raw_dropout(buf, None, out, 0, 0.1, 0, 0) == -1            # NBM_EINVAL
    assert raw_dropout(buf, None, out, -4, 0.1, 0, 0) == -1
    assert raw_dropout(None, None, out, 4, 0.1, 0, 0) == -1
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0                              # nothing was launched
    with pytest.raises(NbmHipError):
        ops.dropout(buf[:0], 0.1, SEED, 0, 0)
    with pytest.raises(ValueError, match='--dropout'):
        ops.dropout(buf, 1.0, SEED, 0, 0)
    with pytest.raises(ValueError):
        ops.dropout(buf, 0.1, SEED, 0, 0, residual=out[:8])


@pytest.mark.parametrize('p', [0.1, 0.5])
def test_fn_dropout_backward_is_the_mask_on_the_gradient(p):
    M, E, call, site = 37, 28, 2, 7                                   # 1036 elements
    x, r, g = (torch.from_numpy(rnd(('fdrop', k), M, E)).cuda() for k in 'xrg')
    keep = ops.dropout_keep_reference(SEED, call, site, M * E, p).reshape(M, E)
    scale = ops.dropout_params(p)[1]
    xd, rd = x.clone().requires_grad_(True), r.clone().requires_grad_(True)
    y = Fn.Dropout.apply(xd, rd, p, SEED, call, site)
    assert np.array_equal(bits(y), bits(expected(x.cpu().numpy(), r.cpu().numpy(), keep, scale)))
    y.backward(g)
    assert np.array_equal(bits(xd.grad), bits(expected(g.cpu().numpy(), None, keep, scale)))
    assert torch.equal(rd.grad, g)
    xd2 = x.clone().requires_grad_(True)                              # without a residual
    y2 = Fn.Dropout.apply(xd2, None, p, SEED, call, site)
    assert np.array_equal(bits(y2), bits(expected(x.cpu().numpy(), None, keep, scale)))
    y2.backward(g)
    assert np.array_equal(bits(xd2.grad), bits(xd.grad))


NH, E = 8, 512
HD = E // NH
GEOMS = [(True, 128, 5, None), (False, 16, 7, 16), (False, 50, 3, 37), (True, 3, 16, None), (False, 65, 2, 65)]


def close(got, ref, tol, name):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = float(ref.abs().max()) + 1e-12
    err = float((got - ref).abs().max())
    print(f'{name}: max err {err:.3e}, scale {scale:.3e}, relative {err / scale:.3e} (bound {tol:.1e})')
    assert err <= tol * scale, f'{name}: max err {err:.3e} vs scale {scale:.3e}'


def attention_f64(qkv, go, seq_major, S, N, n_use, keep, scale, NH=NH):
    """float64 attention with the keep mask [N, NH, S, S] on the probabilities -> (out [n_use, N, E], d/dqkv [S*N, 3E])."""
    E = go.shape[1]
    HD = E // NH
    qkv = qkv.double().requires_grad_(True)
    t = qkv.view(S, N, 3 * E) if seq_major else qkv.view(N, S, 3 * E).transpose(0, 1)
    q, k, v = (t[..., i * E:(i + 1) * E].reshape(S, N * NH, HD).transpose(0, 1) for i in range(3))
    prob = torch.softmax((q[:, :n_use] @ k[:, :n_use].transpose(1, 2)) / HD ** 0.5, -1)
    m = keep.view(N * NH, S, S)[:, :n_use, :n_use]
    att = torch.where(m, prob * scale, torch.zeros_like(prob)) @ v[:, :n_use]
    ref = att.transpose(0, 1).reshape(n_use, N, E)
    gref = go.double().view(S, N, E) if seq_major else go.double().view(N, S, E).transpose(0, 1)
    ref.backward(gref[:n_use])
    return ref.detach(), qkv.grad


@pytest.mark.parametrize('p', [0.1, 0.5])
@pytest.mark.parametrize('seq_major,S,N,nv', GEOMS)
def test_mha_small_drop_forward_and_backward(seq_major, S, N, nv, p):
    """Bounds of the p = 0 test (tests/test_gpu_train.py test_mha_small_backward): 3e-6 forward, 3e-5 gradients, relative to the
    largest reference value."""
    call, site = 4, 8
    qkv = torch.from_numpy(rnd(('mhadrop', seq_major, S), S * N, 3 * E))
    go = torch.from_numpy(rnd(('mhadropg', seq_major, S), S * N, E))
    n_use = S if nv is None else nv
    keep = torch.from_numpy(ops.dropout_keep_reference(SEED, call, site, N * NH * S * S, p)).view(N, NH, S, S)
    ref, gref = attention_f64(qkv, go, seq_major, S, N, n_use, keep, ops.dropout_params(p)[1])
    qd = qkv.cuda().requires_grad_(True)
    cnt = None if nv is None else torch.tensor([nv], dtype=torch.int32, device='cuda')
    ss, bs = (N, 1) if seq_major else (1, S)
    out = Fn.MhaSmallDrop.apply(qd[:, :E], qd[:, E:2 * E], qd[:, 2 * E:], S, N, NH, ss, bs, cnt, p, SEED, call, site)
    got = out.view(S, N, E) if seq_major else out.view(N, S, E).transpose(0, 1)
    close(got[:n_use], ref, 3e-6, 'mha drop fwd')
    valid = torch.zeros(S, N, 1)
    valid[:n_use] = 1
    valid = (valid if seq_major else valid.transpose(0, 1)).reshape(S * N, 1)
    out.backward((go * valid).cuda())
    close(qd.grad, gref, 3e-5, 'mha drop dqkv')
    if (valid == 0).any():
        assert float(qd.grad.cpu()[valid[:, 0] == 0].abs().max()) == 0.0
        assert float(out.detach().cpu()[valid[:, 0] == 0].abs().max()) == 0.0
    # the same (seed, call, site) again: the same bits, forward and backward
    out2 = ops.mha_small_drop(qd.detach()[:, :E], qd.detach()[:, E:2 * E], qd.detach()[:, 2 * E:], S, N, NH, ss, bs, cnt, p, SEED, call, site)
    assert torch.equal(out2, out.detach())
    g2 = ops.mha_small_drop_bwd(qd.detach()[:, :E], qd.detach()[:, E:2 * E], qd.detach()[:, 2 * E:], (go * valid).cuda(), S, N, NH,
                                ss, bs, cnt, p, SEED, call, site)
    assert torch.equal(torch.cat(g2, 1), qd.grad)


# hd = 24: lanes 24 .. 63 of a wave own no output column and a staged K / V row is 24 floats; S = 66 crosses the 64 lanes of a score row
GEOMS_HD24 = [(False, 5, 2, 3), (True, 66, 1, None)]


@pytest.mark.parametrize('seq_major,S,N,nv', GEOMS_HD24)
def test_mha_small_and_drop_with_a_head_dimension_below_64(seq_major, S, N, nv):
    """E = 96, 4 heads.  Bounds of the hd = 64 tests: 3e-6 forward, 3e-5 gradients, relative to the largest reference value (sums
    of 24 instead of 64 products cannot need more)."""
    E, NH, p, call, site = 96, 4, 0.5, 6, 2
    qkv = torch.from_numpy(rnd(('mha24', seq_major, S), S * N, 3 * E))
    go = torch.from_numpy(rnd(('mha24g', seq_major, S), S * N, E))
    n_use = S if nv is None else nv
    cnt = None if nv is None else torch.tensor([nv], dtype=torch.int32, device='cuda')
    ss, bs = (N, 1) if seq_major else (1, S)
    valid = torch.zeros(S, N, 1)
    valid[:n_use] = 1
    valid = (valid if seq_major else valid.transpose(0, 1)).reshape(S * N, 1)
    every = torch.ones(N, NH, S, S, dtype=torch.bool)
    dropped = torch.from_numpy(ops.dropout_keep_reference(SEED, call, site, N * NH * S * S, p)).view(N, NH, S, S)
    for name, keep, scale in (('mha hd24', every, 1.0), ('mha drop hd24', dropped, ops.dropout_params(p)[1])):
        ref, gref = attention_f64(qkv, go, seq_major, S, N, n_use, keep, scale, NH)
        qd = qkv.cuda().requires_grad_(True)
        q, k, v = qd[:, :E], qd[:, E:2 * E], qd[:, 2 * E:]
        if keep is every:
            out = Fn.MhaSmall.apply(q, k, v, S, N, NH, ss, bs, cnt)
        else:
            out = Fn.MhaSmallDrop.apply(q, k, v, S, N, NH, ss, bs, cnt, p, SEED, call, site)
        got = out.view(S, N, E) if seq_major else out.view(N, S, E).transpose(0, 1)
        close(got[:n_use], ref, 3e-6, name + ' fwd')
        out.backward((go * valid).cuda())
        close(qd.grad, gref, 3e-5, name + ' dqkv')
        if (valid == 0).any():
            assert float(qd.grad.cpu()[valid[:, 0] == 0].abs().max()) == 0.0
            assert float(out.detach().cpu()[valid[:, 0] == 0].abs().max()) == 0.0


@pytest.mark.parametrize('mode', [ops.MHA_ACROSS_ROIS, ops.MHA_ACROSS_IMAGES])
def test_mha_segments_is_mha_small_with_a_head_dimension_below_64(mode):
    """Two segments of 2 and 1 images, 5 RoI slots, 3 and 5 of them filled: every valid row holds the bits `ops.mha_small` gives on
    its segment alone, every other row is zero."""
    E, NH, R, sizes, counts = 96, 4, 5, [2, 1], [3, 5]
    qkv = torch.from_numpy(rnd(('mha24seg', mode), sum(sizes) * R, 3 * E)).cuda()
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


@pytest.mark.parametrize('seq_major,S,N,nv', [GEOMS[2], GEOMS[4]])
def test_mha_small_drop_with_threshold_0_is_mha_small(seq_major, S, N, nv):
    p = 1e-12
    assert ops.dropout_params(p) == (0, 1.0)
    qkv = torch.from_numpy(rnd(('mhadrop0', S), S * N, 3 * E)).cuda()
    cnt = torch.tensor([nv], dtype=torch.int32, device='cuda')
    q, k, v = qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:]
    close(ops.mha_small_drop(q, k, v, S, N, NH, 1, S, cnt, p, SEED, 0, 0), ops.mha_small(q, k, v, S, N, NH, 1, S, cnt), 3e-6, 'thr 0')


def test_mha_small_is_untouched_by_the_dropout_kernels():
    """`ops.mha_small` / `ops.mha_small_bwd` give the bits of `Fn.MhaSmall` before and after the dropout kernels have run."""
    S, N, nv = 50, 3, 37
    qkv = torch.from_numpy(rnd('mhasame', S * N, 3 * E)).cuda()
    go = torch.from_numpy(rnd('mhasameg', S * N, E)).cuda()
    cnt = torch.tensor([nv], dtype=torch.int32, device='cuda')
    q, k, v = qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:]
    before = ops.mha_small(q, k, v, S, N, NH, 1, S, cnt)
    gbefore = torch.cat(ops.mha_small_bwd(q, k, v, go, S, N, NH, 1, S, cnt), 1)
    dropped = ops.mha_small_drop(q, k, v, S, N, NH, 1, S, cnt, 0.5, SEED, 0, 0)
    ops.mha_small_drop_bwd(q, k, v, go, S, N, NH, 1, S, cnt, 0.5, SEED, 0, 0)
    assert not torch.equal(dropped, before)
    qd = qkv.clone().requires_grad_(True)
    out = Fn.MhaSmall.apply(qd[:, :E], qd[:, E:2 * E], qd[:, 2 * E:], S, N, NH, 1, S, cnt)
    out.backward(go)
    assert torch.equal(out.detach(), before) and torch.equal(qd.grad, gbefore)
    assert torch.equal(ops.mha_small(q, k, v, S, N, NH, 1, S, cnt), before)
    assert torch.equal(torch.cat(ops.mha_small_bwd(q, k, v, go, S, N, NH, 1, S, cnt), 1), gbefore)


@pytest.mark.parametrize('rows,width', [(80, 512), (1030, 512), (7, 96)])
def test_layernorm_bwd_det_is_layernorm_bwd_with_ordered_sums(rows, width):
    """gx: the bits of `ops.layernorm_bwd`; gw / gb: within 2e-5 of float64 (the bound of the LayerNorm case of
    tests/test_gpu_train.py) and the same bits on every call -- also past 256 workgroups, where a wave takes several rows."""
    import torch.nn.functional as F
    x = torch.from_numpy(rnd(('lndx', rows), rows, width))
    w = torch.from_numpy(1 + 0.1 * rnd(('lndw', rows), width))
    b = torch.from_numpy(0.1 * rnd(('lndb', rows), width))
    go = torch.from_numpy(rnd(('lndg', rows), rows, width))
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, b))
    F.layer_norm(x64, (width,), w64, b64, 1e-5).backward(go.double())
    xd, wd, bd = (t.cuda().requires_grad_(True) for t in (x, w, b))
    y = Fn.LayerNormDet.apply(xd, wd, bd, 1e-5)
    assert torch.equal(y, ops.layernorm(xd.detach(), wd.detach(), bd.detach(), 1e-5))
    y.backward(go.cuda())
    close(xd.grad, x64.grad, 2e-5, 'ln det dx'); close(wd.grad, w64.grad, 2e-5, 'ln det dw'); close(bd.grad, b64.grad, 2e-5, 'ln det db')
    gx, gw, gb = ops.layernorm_bwd(xd.detach(), wd.detach(), go.cuda(), 1e-5)
    assert torch.equal(xd.grad, gx)
    close(wd.grad, gw, 2e-5, 'ln det dw vs atomics'); close(bd.grad, gb, 2e-5, 'ln det db vs atomics')
    for _ in range(2):
        gx2, gw2, gb2 = ops.layernorm_bwd_det(xd.detach(), wd.detach(), go.cuda(), 1e-5)
        assert torch.equal(gx2, gx) and torch.equal(gw2, wd.grad) and torch.equal(gb2, bd.grad)
    ws = torch.empty(8, device='cuda')
    ptr = lambda t: C.c_void_p(t.data_ptr())
    assert ops.lib().nbm_layernorm_bwd_det(ptr(xd), ptr(wd), ptr(go.cuda()), rows, width, 1e-5, ptr(gx), ptr(gw), ptr(gb), ptr(ws), 8,
                                           None) == -1             # a workspace that is too small: nothing is launched
