"""GPU: the deterministic twins behind ops.set_deterministic, one by one.  Three properties each:
 (a) accuracy: within the bound the existing test of the DEFAULT kernel uses against its float64 reference (cited beside each use);
 (b) repeatability: five launches give identical bits, two of them after the slot workspace was filled with NaN;
 (c) scheduling independence: two of the five run while a second stream executes a long filler axpby, so that the workgroups are
     placed differently.
Shapes are the smallest at which the mechanism can go wrong: several workgroups / pixel splits, odd sizes, partial tiles."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_ref as CR                                            # noqa: E402
import detect_ref as D                                           # noqa: E402
import pointwise_ref as R                                        # noqa: E402
from birdsoundclassif_amd import _lib, ops, synth                # noqa: E402

U64 = R.U64


def rnd(key, *shape, scale=1.0, shift=0.0):
    return torch.from_numpy((synth.normal(key, int(np.prod(shape))) * scale + shift).astype(np.float32).reshape(shape))


def dev(t):
    return t.cuda().contiguous()


@pytest.fixture
def det():
    with ops.set_deterministic(True):
        yield


_FILLER = {}


@pytest.fixture(autouse=True, scope='module')
def _release_the_filler():
    yield
    _FILLER.clear()
    torch.cuda.empty_cache()


def _filler():
    if not _FILLER:
        _FILLER['s'] = torch.cuda.Stream()
        _FILLER['a'] = torch.ones(1 << 25, device='cuda')
        _FILLER['b'] = torch.ones(1 << 25, device='cuda')
        _FILLER['c'] = torch.empty(1 << 25, device='cuda')
    return _FILLER['s'], _FILLER['a'], _FILLER['b']


def five(run):
    """run() -> tensor or tuple of tensors.  Launch 1 plain, 2 and 5 after the workspaces were filled with NaN bytes, 3 and 4 while the
    filler stream is busy; all five must agree bit for bit.  -> the first result."""
    def once(busy=False):
        if busy:                                                  # ~40 x 0.1 ms of filler on the second stream, queued right before the launch
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(40):
                    _lib.check(ops.lib().nbm_axpby(ops._ptr(a), ops._ptr(b), ops._ptr(_FILLER['c']), 1.0, 1.0, a.numel(), 0, ops._stream()),
                               'nbm_axpby')
        r = run()
        r = r if isinstance(r, (tuple, list)) else (r,)
        return [t.detach().clone() for t in r if t is not None]

    def poison():
        for buf in ops._DET['ws'].values():
            if buf is not None:
                buf.fill_(255)                                    # 0xFF..: a NaN in every float and double slot

    s, a, b = _filler()
    results = [once()]
    poison()
    results.append(once())
    for _ in range(2):
        results.append(once(busy=True))
    torch.cuda.synchronize()
    poison()
    results.append(once())
    torch.cuda.synchronize()
    for k, other in enumerate(results[1:], 2):
        for i, (x, y) in enumerate(zip(results[0], other)):
            assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), f'launch {k}, output {i} differs from launch 1'
            assert bool(torch.isfinite(x).all()) if x.dtype.is_floating_point else True
    return results[0] if len(results[0]) > 1 else results[0][0]


def report(name, r):
    print(f'RATIO {name} {r:.3g}')
    assert r <= 1.0, f'{name}: error / limit = {r:.3g}'


# ================================================================================================== the ordered reduction itself
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['float', 'double'])
def test_ordered_sum_adds_the_slots_in_ascending_order(dtype):
    """out[i] (+)= sum_s part[s][i] carried in the partials' type, s ascending: equal to the same loop on the host, bit for bit."""
    slots, n = 37, 1003
    part = rnd(('os', str(dtype)), slots, n).to(dtype)
    part[:, 0] = torch.tensor([1e8, 1.0, -1e8] + [0.0] * (slots - 3), dtype=dtype)     # the order shows: (1e8 + 1) - 1e8 = 0 in fp32
    base = rnd('os.base', n)
    ref = torch.zeros(n, dtype=dtype)
    for s in range(slots):
        ref = ref + part[s]
    pd = dev(part)
    for acc in (0, 1):
        out = dev(base).clone()
        _lib.check(ops.lib().nbm_ordered_sum(ops._ptr(pd), int(dtype == torch.float64), slots, n, ops._ptr(out), acc, ops._stream()),
                   'nbm_ordered_sum')
        want = (base + ref.float()) if acc else ref.float()
        assert torch.equal(out.cpu(), want), acc


# ================================================================================================== nbm_conv_wgrad
# Precision bound of tests/test_gpu_train_geometry.py:376-387 (`_prec_bound`): K fp32 additions of products, each rounding <= 2^-24 of the
# running |sum| <= abs_ref, as independent errors at 6.5 sigma, doubled: 8 sqrt(K) 2^-24 abs_ref.  The twin adds the same K products (the
# splits' partial sums, then `splits` more additions, which sqrt(K) covers as it covers the atomics' there).
def prec_bound(K, absref):
    return 8.0 * math.sqrt(K) * 2.0 ** -24 * absref + 1e-30


WGRAD = {
    '1x1': dict(B=2, H=47, W=128, Cin=64, N=64),
    '3x3-s2-odd': dict(B=2, H=23, W=31, Cin=32, N=32, k=3, stride=2, pad=1),
    'generic-cin3': dict(B=2, H=47, W=128, Cin=3, N=32, k=3, pad=1),
    'n17-bias-rowscale': dict(B=2, H=47, W=128, Cin=64, N=17, bias=True, row_scale=True),
    'groups2': dict(B=1, H=2 * 47 * 128, W=1, Cin=32, N=32, groups=2),
    'accumulate': dict(B=2, H=47, W=128, Cin=64, N=64, accumulate=True),
    'halves-cin192': dict(B=2, H=47, W=128, Cin=192, N=64),
}


@pytest.mark.parametrize('name', list(WGRAD))
def test_wgrad_twin(det, name):
    c = dict(WGRAD[name])
    B, H, W, Cin, N = c['B'], c['H'], c['W'], c['Cin'], c['N']
    k, stride, pad, G = c.get('k', 1), c.get('stride', 1), c.get('pad', 0), c.get('groups', 1)
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    g_ld = (N + 3) // 4 * 4
    g = dev(rnd(('wg.g', name), G, B, Ho, Wo, g_ld))
    x = dev(rnd(('wg.x', name), G, B, H, W, Cin))
    KC = k * k * Cin
    base = dev(rnd(('wg.base', name), G, N, KC)) if c.get('accumulate') else torch.zeros((G, N, KC), device='cuda')
    row_scale = dev(rnd(('wg.rs', name), N)) if c.get('row_scale') else None
    bias0 = dev(rnd(('wg.b', name), N)) if c.get('bias') else None
    kw = dict(B=B, H=H, W=W, Cin=Cin, N=N, kh=k, kw=k, stride=stride, pad=pad, g_ld=g_ld, groups=G, g_gs=B * Ho * Wo * g_ld,
              x_gs=B * H * W * Cin, out_gs=N * KC, row_scale=row_scale, alpha=0.5)
    # the slices are really exercised: the plan the twin runs has >= 2 pixel splits
    d = ops._bwd_desc(g, B=B, H=H, W=W, Cin=Cin, N=N, kh=k, kw=k, stride=stride, pad=pad, g_ld=g_ld, groups=G, alpha=0.5)
    d.x, d.out, d.x_ld, d.out_ld = x.data_ptr(), base.data_ptr(), Cin, KC
    d.g_gs, d.x_gs, d.out_gs = kw['g_gs'], kw['x_gs'], kw['out_gs']
    plan = ops.gemm_plan(2, d)
    assert plan.rc == 0 and plan.splits >= 2, plan
    assert plan.halves == (1 if name.startswith('halves') else 0)

    def run():
        out = base.clone()
        bg = None if bias0 is None else bias0.clone()
        ops.conv_wgrad(g, x, out, bias_grad=bg, **kw)
        return out, bg
    got = five(run)
    out, bg = (got[0], got[1]) if bias0 is not None else (got, None)
    gv = g[..., :N]
    rk = dict(kh=k, kw=k, stride=stride, pad=pad, row_scale=row_scale, alpha=0.5)
    ref, gb_ref = CR.wgrad(gv, x, out=base, bias_grad=bias0, **rk)
    absr, absb = CR.wgrad(gv.abs(), x.abs(), out=base.abs(), bias_grad=None if bias0 is None else bias0.abs(),
                          **dict(rk, row_scale=None if row_scale is None else row_scale.abs()))
    K = B * Ho * Wo
    report(f'wgrad {name}', float(((out.double() - ref).abs() / prec_bound(K, absr)).max()))
    if bias0 is not None:
        report(f'wgrad {name} bias', float(((bg.double() - gb_ref.reshape(-1)).abs() / prec_bound(K, absb.reshape(-1))).max()))


def test_wgrad_twin_refuses_a_workspace_that_is_too_small(det):
    c = WGRAD['1x1']
    g, x = dev(rnd('wr.g', 2, 47, 128, 64)), dev(rnd('wr.x', 2, 47, 128, 64))
    out = torch.zeros((64, 64), device='cuda')
    d = ops._bwd_desc(g, B=2, H=47, W=128, Cin=64, N=64, kh=1, kw=1, stride=1, pad=0, g_ld=64)
    d.x, d.out, d.x_ld, d.out_ld = x.data_ptr(), out.data_ptr(), 64, 64
    nbytes, stride = ops.wgrad_workspace(d)
    ws = torch.zeros((nbytes,), device='cuda', dtype=torch.uint8)
    for bad_stride, bad_bytes in ((stride - 4, nbytes), (stride, nbytes - 4), (stride + 2, nbytes * 2)):
        d.workspace, d.ws_split_stride, d.workspace_bytes = ws.data_ptr(), bad_stride, bad_bytes
        assert ops.lib().nbm_conv_wgrad(C.byref(d), ops._stream()) == -1
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0 and c['N'] == 64


# ================================================================================================== bias gradients that ride along
def test_winograd_bias_gradients(det):
    """F(2x2) and F(4x4) output-gradient transforms, B = 2, 24 x 64, C = N = 32: gb = sum of g over the pixels, rtol = atol = 1e-4 as in
    tests/test_gpu_lazy.py:290."""
    x, g = dev(rnd('wb.x', 2, 24, 64, 32)), dev(rnd('wb.g', 2, 24, 64, 32))
    ref = g.double().sum((0, 1, 2))
    for m in (2, 4):
        dU, gb = five(lambda m=m: ops.conv3x3_winograd_wgrad(x, g, want_bias=True, m=m))
        assert torch.allclose(gb.double(), ref, rtol=1e-4, atol=1e-4), m
        dU0, _ = ops.conv3x3_winograd_wgrad(x, g, want_bias=False, m=m)
        assert torch.equal(dU, dU0)


def test_cell_bias_gradients(det):
    """nbm_cell_outgrad (sum of the 3 x 3 pattern blocks) and nbm_cell_dgrad_output (sum of the patches written), B = 2, 24 x 64,
    C = N = 32, stride 8: rtol = atol = 1e-4 as in tests/test_gpu_lazy.py:290."""
    B, H, W, N, S = 2, 24, 64, 32, 8
    g = dev(rnd('cb.g', B, H, W, N))
    OH, OW = (H + 2 - 3) // S + 1, (W + 2 - 3) // S + 1
    T = B * OH * OW
    mask = torch.zeros(H, W, dtype=torch.bool)
    for oy in range(OH):
        for ox in range(OW):
            mask[max(S * oy - 1, 0):S * oy + 2, max(S * ox - 1, 0):S * ox + 2] = True
    ref = (g.double() * mask.cuda()[None, :, :, None]).sum((0, 1, 2))

    def outgrad():
        vg = torch.empty((25, T, N), device='cuda')
        gb = torch.zeros((N,), device='cuda')
        ops._reduction('nbm_cell_outgrad', (ops._ptr(g), B, H, W, N, S, ops._ptr(vg), ops._ptr(gb)), lambda: ops._bias_ws_bytes(N))
        return gb, vg
    gb, vg = five(outgrad)
    assert torch.allclose(gb.double(), ref, rtol=1e-4, atol=1e-4)
    vg0 = torch.empty_like(vg)
    _lib.check(ops.lib().nbm_cell_outgrad(ops._ptr(g), B, H, W, N, S, ops._ptr(vg0), None, ops._stream()), 'nbm_cell_outgrad')
    assert torch.equal(vg, vg0)                                   # the transform itself is the default kernel's

    M = dev(rnd('cb.m', 25, T, N))

    def dgrad_output():
        gx = torch.zeros((B, H, W, N), device='cuda')
        gb = torch.zeros((N,), device='cuda')
        ops._reduction('nbm_cell_dgrad_output', (ops._ptr(M), B, H, W, N, S, ops._ptr(gx), -1, N, 0, ops._ptr(gb)), lambda: ops._bias_ws_bytes(N))
        return gb, gx
    gb, gx = five(dgrad_output)
    assert torch.allclose(gb.double(), gx.double().sum((0, 1, 2)), rtol=1e-4, atol=1e-4)


# ================================================================================================== stem
def test_stem_wgrad_twin(det):
    """The (2, 64, 96, 1) image of the stem tests; bound of tests/test_gpu_train_geometry.py:949-953 (`_prec_bound` on the two sums)."""
    B, H, W = 2, 64, 96
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    img, g = dev(rnd('st.img', B, H, W, 1)), dev(rnd('st.g', B, Ho, Wo, 64))
    U, V = five(lambda: ops.stem7x7_wgrad(img, g))
    K = B * Ho * Wo
    for name, got, x in (('U', U, img), ('V', V, torch.ones_like(img))):
        ref, _ = CR.wgrad(g, x, kh=7, kw=7, stride=2, pad=3)
        absr, _ = CR.wgrad(g.abs(), x.abs(), kh=7, kw=7, stride=2, pad=3)
        report(f'stem {name}', float(((got.reshape(64, 49).double() - ref).abs() / prec_bound(K, absr)).max()))


# ================================================================================================== RoI pooling backward
FMAP_HW = [(64, 128), (32, 64), (16, 32), (8, 16), (4, 8)]      # a 128 x 256 image
ROI_C = 8


def roi_bwd_ref(rois, level, gpool, ph, pw):
    """Float64 restatement of the pooling's transpose (layers.py:424-465 windows, bins floor / ceil): every pixel of a bin receives
    g / bin area."""
    B, Rn = rois.shape[:2]
    out = [torch.zeros(B, h, w, ROI_C, dtype=torch.float64) for h, w in FMAP_HW]
    gp = gpool.double().view(B, Rn, ph, pw, ROI_C)
    for b in range(B):
        for r in range(Rn):
            lvl = int(level[b, r])
            H, W = FMAP_HW[lvl]
            s = float(2 << lvl)
            x1, y1, x2, y2 = (int(np.rint(np.float32(v) / np.float32(s))) for v in rois[b, r].tolist())
            y2 = min(y2, H - 1)
            for _ in range(max(ph, pw)):
                if y2 - y1 + 1 >= ph:
                    break
                y1, y2 = max(0, y1 - 1), min(H - 1, y2 + 1)
            for _ in range(max(ph, pw)):
                if x2 - x1 + 1 >= pw:
                    break
                x1, x2 = max(0, x1 - 1), min(W - 1, x2 + 1)
            h, w = y2 - y1 + 1, min(x2, W - 1) - x1 + 1
            assert h >= 1 and w >= 1
            for i in range(ph):
                ya, yb = (i * h) // ph, -((-(i + 1) * h) // ph)
                for j in range(pw):
                    xa, xb = (j * w) // pw, -((-(j + 1) * w) // pw)
                    out[lvl][b, y1 + ya:y1 + yb, x1 + xa:x1 + xb] += gp[b, r, i, j] / ((yb - ya) * (xb - xa))
    return out


def mixed_rois(B, n, key):
    """Boxes of every size class of the 128 x 256 image, so that they cross all level boundaries."""
    u = synth.uniform(key, B * n * 4).reshape(B, n, 4)
    size = 6.0 * 2.0 ** (u[..., 2] * 5.2)                         # 6 .. 220 pixels
    w = np.minimum(size * (0.6 + 0.8 * u[..., 3]), 250.0)
    h = np.minimum(size / (0.6 + 0.8 * u[..., 3]), 124.0)
    x1, y1 = np.floor(u[..., 0] * (255.0 - w)), np.floor(u[..., 1] * (127.0 - h))
    return torch.from_numpy(np.stack([x1, y1, x1 + np.floor(w), y1 + np.floor(h)], -1).astype(np.float32))


def run_roi_bwd(rois, ph, pw, key):
    B, Rn = rois.shape[:2]
    rd = dev(rois)
    fm = [torch.zeros(B, h, w, ROI_C, device='cuda') for h, w in FMAP_HW]
    pe_f, pe_t = torch.zeros(128, ROI_C // 2, device='cuda'), torch.zeros(256, ROI_C // 2, device='cuda')
    _, _, level = ops.roi_pool(fm, rd, torch.full((B,), Rn, dtype=torch.int32, device='cuda'), pe_f, pe_t, 128, 256, pool_hw=(ph, pw))
    gpool = dev(rnd(key, B * Rn, ph, pw, ROI_C))
    shapes = [tuple(f.shape) for f in fm]
    gf = five(lambda: ops.roi_pool_bwd(gpool, rd, level, shapes))
    return gf, level.cpu(), gpool.cpu()


@pytest.mark.parametrize('ph,pw', [(2, 2), (3, 3)])
@pytest.mark.parametrize('kind', ['same-box', 'mixed'])
def test_roi_pool_backward_twin(det, kind, ph, pw):
    """B = 2, 16 RoIs per image -- all the same box (every pixel of the window receives 16 shares: where the scatter order matters most) or a
    mixed set across the level boundaries; 1e-5 of the largest gradient of the level as in tests/test_gpu_roi_pool_sizes.py:208-212."""
    B, Rn = 2, 16
    rois = torch.tensor([37.0, 21.0, 75.0, 64.0]).expand(B, Rn, 4).contiguous() if kind == 'same-box' else mixed_rois(B, Rn, ('roi', ph))
    gf, level, gpool = run_roi_bwd(rois, ph, pw, ('roi.g', kind, ph))
    if kind == 'mixed':
        assert len(set(level.reshape(-1).tolist())) >= 4
    ref = roi_bwd_ref(rois, level, gpool, ph, pw)
    for i, (got, want) in enumerate(zip(gf, ref)):
        err, scale = float((got.cpu().double() - want).abs().max()), float(want.abs().max())
        assert err <= 1e-5 * scale, f'level {i}: max err {err:.3e} vs scale {scale:.3e}'


def test_roi_pool_backward_twin_with_1000_rois(det):
    """The evaluation geometry's count: four chunks of the 256-record window pass, B = 1."""
    rois = mixed_rois(1, 1000, 'roi1000')
    gf, level, gpool = run_roi_bwd(rois, 2, 2, 'roi1000.g')
    ref = roi_bwd_ref(rois, level, gpool, 2, 2)
    for i, (got, want) in enumerate(zip(gf, ref)):
        err, scale = float((got.cpu().double() - want).abs().max()), float(want.abs().max())
        assert err <= 1e-5 * scale, f'level {i}: max err {err:.3e} vs scale {scale:.3e}'


def test_roi_pool_backward_twin_adds_to_a_base_and_leaves_other_pixels_alone(det):
    """The twin reads and writes only pixels inside a RoI window (the footprint nbm_zero_roi_windows restores): NaN everywhere else in the map
    stays NaN and never reaches a window pixel."""
    rois = torch.tensor([37.0, 21.0, 75.0, 64.0]).expand(1, 16, 4).contiguous()
    rd = dev(rois)
    level = torch.full((1, 16), 2, dtype=torch.int32, device='cuda')             # sqrt(38 * 43) * 0.1 = 4.04 -> level 2
    gpool = dev(rnd('roi.base.g', 16, 2, 2, ROI_C))
    gf = [torch.full((1, h, w, ROI_C), float('nan'), device='cuda') for h, w in FMAP_HW]
    gf[2][0, 3:9, 5:10] = 1.0                                                      # rows 21/8 -> 3 .. 8, columns 37/8 -> 5 .. 9
    n = len(gf)
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in gf])
    fh, fw = (C.c_int * n)(*[h for h, _ in FMAP_HW]), (C.c_int * n)(*[w for _, w in FMAP_HW])
    ops._reduction('nbm_roi_pool_hw_bwd', (ptrs, fh, fw, n, ROI_C, ops._ptr(rd), ops._ptr(level), 1, 16, 2, 2, ops._ptr(gpool)))
    torch.cuda.synchronize()
    ref = roi_bwd_ref(rois, level.cpu(), gpool.cpu(), 2, 2)[2]
    win = gf[2][0, 3:9, 5:10].cpu().double()
    assert bool(torch.isfinite(win).all()) and float((win - 1.0 - ref[0, 3:9, 5:10]).abs().max()) <= 1e-5 * float(ref.abs().max())
    gf[2][0, 3:9, 5:10] = float('nan')
    assert all(bool(torch.isnan(t).all()) for t in gf)


# ================================================================================================== tile lists
def test_tile_list_is_ascending_in_image_and_tile_id(det):
    """B = 3 on the finest (64 x 128) map: image 0 a few tiles, image 1 more than 128 (at least two blocks), image 2 none.  The list equals
    the host restatement as a SEQUENCE: image by image, ids ascending, every image's run padded to whole 128-entry blocks."""
    level = 0
    H, W = FMAP_HW[level]
    TH, TW = (H + 1) // 2, (W + 1) // 2
    thw = TH * TW
    R_ = 40
    rois = torch.zeros(3, R_, 4)
    small = torch.tensor([[4.0 + 6 * i, 6.0 + 3 * (i % 7), 4.0 + 6 * i + 14, 6.0 + 3 * (i % 7) + 12] for i in range(R_)])   # level 0: size < 20
    rois[0, :5], rois[1], rois[2, :3] = small[:5], small, small[:3]
    n_roi = [5, R_, 0]
    ref_set = D.tiles_ref(rois, n_roi, level, 0, None, fmap_hw=FMAP_HW)
    per_img = [sorted(t for t in ref_set if t // thw == b) for b in range(3)]
    assert 0 < len(per_img[0]) <= 128 < len(per_img[1]) and not per_img[2]
    want = []
    for ids in per_img:
        want += ids + [-1] * (-len(ids) % 128)
    nl = len(FMAP_HW)
    fh, fw = (C.c_int * nl)(*[h for h, _ in FMAP_HW]), (C.c_int * nl)(*[w for _, w in FMAP_HW])
    rd, nd = dev(rois), torch.tensor(n_roi, dtype=torch.int32, device='cuda')
    n_cap = 3 * (-(-thw // 128)) * 128

    def run():
        tiles = torch.full((n_cap,), -5, device='cuda', dtype=torch.int32)
        n_blocks = torch.full((1,), -5, device='cuda', dtype=torch.int32)
        ops.roi_tiles(ops._ptr(rd), ops._ptr(nd), 3, R_, nl, level, fh, fw, None, 0, ops._ptr(tiles), ops._ptr(n_blocks))
        return tiles[:len(want)], n_blocks
    tiles, n_blocks = five(run)
    assert int(n_blocks) == len(want) // 128 >= 3
    assert tiles.cpu().tolist() == want


# ================================================================================================== point-wise reductions
@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('Cin,mult', [(8, 2), (5, 3)], ids=['vec-C8-m2', 'scalar-C5-m3'])
def test_dwconv_weight_gradient_twin(det, Cin, mult, stride):
    """2 x 13 x 17: 2e-5 of the largest value as in tests/test_gpu_pointwise_edges.py:465-466 (both forms of the kernel)."""
    cfg = (2, 13, 17, Cin, mult, stride)
    Cout = Cin * mult
    x, w = rnd(('dw.x', cfg), 2, 13, 17, Cin), rnd(('dw.w', cfg), Cout, 1, 3, 3, scale=0.3)
    Ho, Wo = (13 - 1) // stride + 1, (17 - 1) // stride + 1
    g = rnd(('dw.g', cfg), 2, Ho, Wo, Cout)
    xd, gd, wd = dev(x), dev(g), dev(w)
    gw, gb = five(lambda: ops.dwconv3x3_bwd(xd, gd, wd, mult, stride, need_gx=False))     # (gx is None: `five` drops it)
    _, rgw, rgb = R.dwconv_bwd(x, g, w, mult, stride)
    for name, got, ref in (('gw', gw, rgw), ('gb', gb, rgb)):
        err = float((R.t64(got) - R.t64(ref)).abs().max())
        report(f'dwconv {name} {cfg}', err / (2e-5 * (float(R.t64(ref).abs().max()) + 1e-12)))


def test_colsum_twin(det):
    """M = 100 003 rows, N = 18: the default kernel's bound is one fp32 rounding per workgroup of the column, k = min(ceil(M / 4), 1024)
    (tests/test_gpu_pointwise_edges.py:357-363); the twin carries the sum in double and rounds once, far inside it."""
    M, N, ld = 100003, 18, 20
    g = rnd('cs.g', M, ld)
    out = five(lambda: ops.colsum(dev(g), N))
    report('colsum', R.ratio(out, *R.colsum(g, N), min((M + 3) // 4, 1024)))
    big = rnd('cs.big', M, ld, scale=1e-2, shift=1e4)
    report('colsum mean 1e4', R.ratio(five(lambda: ops.colsum(dev(big), N)), *R.colsum(big, N), min((M + 3) // 4, 1024)))


@pytest.mark.parametrize('raw', [(0.7, -0.2, 1.3), (0.5, 0.9)], ids=str)
def test_weighted_sum_bwd_twin(det, raw):
    """One ReLU'd weight at zero, n = 4 * 100 003 (no multiple of the grid's sweep): the bounds of
    tests/test_gpu_pointwise_edges.py:334-345 (gx: k = 5; gw: k = 4 sweeps + 8 + workgroups + 15)."""
    n = 4 * 100003
    xs = [rnd(('ws.x', raw, i), n) for i in range(len(raw))]
    g, wt = rnd(('ws.g', raw), n), torch.tensor(raw, dtype=torch.float32)
    xd, gd, wd = [dev(t) for t in xs], dev(g), dev(wt)

    def run():
        gxs, gw = ops.weighted_sum_bwd(xd, wd, gd, [True] * len(raw))
        return (*gxs, gw)
    got = five(run)
    rgx, (rgw, rgw_a) = R.weighted_sum_bwd(xs, wt, g)
    for i in range(len(raw)):
        report(f'weighted_sum gx{i} {raw}', R.ratio(got[i], rgx[i][0], rgx[i][1], 5))
    blocks = min(max((n // 4 + 255) // 256, 1), 2048)
    sweeps = -(-(n // 4) // (blocks * 256))
    report(f'weighted_sum gw {raw}', R.ratio(got[-1], rgw, rgw_a, 4 * sweeps + 8 + blocks + 15))
    for i, r in enumerate(raw):
        if r <= 0:
            assert float(got[-1][i]) == 0.0


def test_batchnorm_twins(det):
    """M = 4 099, C = 12: the bounds of tests/test_gpu_pointwise_edges.py:385-397 (the sums run in double: the final fp32 rounding, plus
    (M + 8) 2^-53 of the magnitudes)."""
    M, Cc, eps, mom = 4099, 12, 1e-5, 0.1
    x, g = rnd('bn.x', M, Cc, scale=2.0), rnd('bn.g', M, Cc)
    w, b = 1 + 0.1 * rnd('bn.w', Cc), 0.1 * rnd('bn.b', Cc)
    rm, rv = 0.05 * rnd('bn.rm', Cc), 1 + 0.1 * rnd('bn.rv', Cc).abs()
    xd, gd, wd, bd = dev(x), dev(g), dev(w), dev(b)
    y, mean, invstd = five(lambda: ops.bn_train_fwd(xd, wd, bd, eps, mom, dev(rm), dev(rv)))
    r = R.bn_train_fwd(x, w, b, eps, mom, rm, rv)
    dvar = (M + 8) * U64 * r['var_cancel']
    rel = 0.5 * dvar / (r['var'][0] + float(np.float32(eps)))
    report('bn mean', R.ratio(mean, *r['mean'], 1, (M + 8) * U64 * r['mean'][1]))
    report('bn invstd', R.ratio(invstd, *r['invstd'], 1, rel * r['invstd'][0]))
    xm = (x.double() - r['mean'][0]).abs() * r['invstd'][0] * w.double().abs()
    report('bn y', R.ratio(y, *r['y'], 6, rel * xm))
    gx, gw, gb = five(lambda: ops.bn_train_bwd(gd, xd, mean, invstd, wd))
    (rgx, rgx_a), (rgw, rgw_a), (rgb, rgb_a) = R.bn_train_bwd(g, x, mean, invstd, w)
    report('bn gx', R.ratio(gx, rgx, rgx_a, 12, (M + 8) * U64 * rgx_a))
    report('bn gw', R.ratio(gw, rgw, rgw_a, 3, (M + 8) * U64 * rgw_a))
    report('bn gb', R.ratio(gb, rgb, rgb_a, 1, (M + 8) * U64 * rgb_a))


def test_sqnorm_twin(det):
    """n = 1 000 003 onto a non-zero start: k = sweeps + 11 + workgroups roundings of 2^-53 (tests/test_gpu_pointwise_edges.py:493-501)."""
    n, init = 1000003, 3.25
    g = rnd('sq.g', n)
    gd = dev(g)

    def run():
        out = torch.tensor([init], dtype=torch.float64).cuda()
        ops.sqnorm_accum(gd, out)
        return out
    out = float(five(run))
    ref = init + R.sqnorm(g)
    blocks = min((n + 255) // 256, 2048)
    k = -(-n // (blocks * 256)) + 11 + blocks
    report('sqnorm', abs(out - ref) / (k * U64 * ref))


def test_film_backward_has_nothing_to_order(det):
    """`film_bwd_kernel` holds no atomic (every output element is written once): it runs unchanged in deterministic mode and repeats."""
    gy, z, film = dev(rnd('fm.g', 1037, 12)), dev(rnd('fm.z', 1037, 12)), dev(rnd('fm.f', 1037, 24))
    gz, gf = five(lambda: ops.film_bwd(gy, z, film))
    assert torch.equal(gz, gy * film[:, :12]) and torch.equal(gf, torch.cat([gy * z, gy], 1))


def test_layernorm_backward_routes_to_its_twin(det):
    x, w, g = dev(rnd('ln.x', 1037, 96)), dev(rnd('ln.w', 96)), dev(rnd('ln.g', 1037, 96))
    a = five(lambda: ops.layernorm_bwd(x, w, g))
    b = ops.layernorm_bwd_det(x, w, g)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_tilewise_bilinear_backward_is_refused_and_the_dense_route_is_repeatable(det):
    """nbm_tiles_upsample_bilinear_bwd_add has no twin: deterministic mode switches ondemand.UPBWD_SPLIT off, so the RoI share stays in the
    map and goes through the dense gather-form kernel, and a tile share that still arrives is refused."""
    from birdsoundclassif_amd import ondemand
    assert ondemand.UPBWD_SPLIT is False
    gy = dev(rnd('ub.g', 2, 47, 66, 8))
    five(lambda: ops.upsample_bilinear_bwd(gy, 24, 33))
    tiles = torch.full((128,), -1, device='cuda', dtype=torch.int32)
    with pytest.raises(RuntimeError, match='nbm_tiles_upsample_bilinear_bwd_add is not reproducible under --deterministic'):
        ops.upsample_bilinear_bwd(gy, 24, 33, tiles_share=[(torch.zeros((512, 8), device='cuda'), tiles, 0, 2)])
