"""GPU: the RoI-pooling kernels (csrc/roipool.hip: nbm_roi_pool_hw / nbm_roi_pool_hw_bwd) at pool sizes other than
2 x 2, on the level-boundary and edge RoIs of tests/detect_ref.py and the real map sizes, against the CPU oracle
(`oracle.nets_ref.roi_pooling` with `roi_pool_h` / `roi_pool_w` set).

Criteria are those of the 2 x 2 tests in test_gpu_detect_edges.py: `level` equal, `pool` bit-equal on the integer maps and
within 2e-7 relative on the modular maps, `pe` within 2e-6 + 2e-6 |ref|, gradients within 1e-5 of the largest per level."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from birdsoundclassif_amd import _lib, ops                           # noqa: E402
from birdsoundclassif_amd.nets import functional as Fn               # noqa: E402
import detect_ref as D                                               # noqa: E402
from helpers import load_golden                                      # noqa: E402
from oracle import nets_ref as O                                     # noqa: E402

IMG_W, IMG_H = D.IMG_W, D.IMG_H
SIZES = [(3, 4), (7, 7), (12, 32), (2, 5)]
B, C_ROI = 3, 16


def i32(v):
    return torch.tensor(list(v), dtype=torch.int32).cuda()


def _pe_tables(C=C_ROI):
    from birdsoundclassif_amd.nets.position_encoding import one_dimension_positional_encoding as pe1d
    return pe1d(IMG_H, C // 2).cuda().contiguous(), pe1d(IMG_W, C // 2).cuda().contiguous()


_ROIS = []


def all_rois():
    """[3, 271, 4]: the level-boundary RoIs (one placement per image) followed by the edge RoIs (in every image)."""
    if not _ROIS:
        _ROIS.append(torch.cat([D.boundary_rois(), D.edge_rois().expand(B, -1, -1)], 1).contiguous())
    return _ROIS[0]


_REF = {}


def oracle(ph, pw, kind, C=C_ROI):
    """(pool, pe, level) of the oracle, computed once per (size, map kind, channel count) and never modified."""
    key = (ph, pw, kind, C)
    if key not in _REF:
        fmaps = {'integer': D.integer_fmaps, 'modular': D.modular_fmaps}[kind](B, C)
        with torch.no_grad():
            _REF[key] = O.roi_pooling(O.make_cfg(roi_pool_h=ph, roi_pool_w=pw), all_rois(), fmaps)
    return _REF[key]


def nhwc(fmaps):
    return [f.permute(0, 2, 3, 1).contiguous().cuda() for f in fmaps]


def device_pool(ph, pw, fmaps_d, n_roi, C=C_ROI):
    rois = all_rois()
    R = rois.shape[1]
    pe_f, pe_t = _pe_tables(C)
    pool, pe, lvl = ops.roi_pool(fmaps_d, rois.cuda(), i32(n_roi), pe_f, pe_t, IMG_H, IMG_W, pool_hw=(ph, pw))
    assert pool.shape == (B * R, ph, pw, C) and pe.shape == pool.shape
    return (pool.view(B, R, ph, pw, C).permute(0, 1, 4, 2, 3).cpu(), pe.view(B, R, ph, pw, C).permute(0, 1, 4, 2, 3).cpu(),
            lvl.cpu())


def assert_pe_close(pe, ref_pe):
    err = (pe - ref_pe).abs()
    assert bool((err <= 2e-6 + 2e-6 * ref_pe.abs()).all()), float(err.max())


@pytest.mark.parametrize('ph,pw', SIZES)
def test_forward_on_the_boundary_and_edge_rois(ph, pw):
    R = all_rois().shape[1]
    ref_pool, ref_pe, ref_lvl = oracle(ph, pw, 'integer')
    pool, pe, lvl = device_pool(ph, pw, nhwc(D.integer_fmaps(B, C_ROI)), [R] * B)
    bad = (lvl.long() != ref_lvl).nonzero().tolist()
    assert not bad, f'{len(bad)} RoIs on another pyramid level, first: {all_rois()[bad[0][0], bad[0][1]].tolist()}'
    assert torch.equal(pool, ref_pool), f'{int((pool != ref_pool).any(-1).any(-1).any(-1).sum())} RoIs pooled another window'
    assert_pe_close(pe, ref_pe)
    ref_pool = oracle(ph, pw, 'modular')[0]
    pool = device_pool(ph, pw, nhwc(D.modular_fmaps(B, C_ROI)), [R] * B)[0]
    err = (pool - ref_pool).abs()
    print(f'{ph}x{pw}: modular pool max relative error {float((err / ref_pool.abs().clamp(min=1e-30)).max()):.3e}')
    assert bool((err <= 2e-7 * ref_pool.abs()).all()), float(err.max())


@pytest.mark.parametrize('ph,pw', SIZES)
def test_rows_beyond_the_count_stay_zero(ph, pw):
    R = all_rois().shape[1]
    n_roi = [R, 0, 77]
    ref_pool, ref_pe, ref_lvl = oracle(ph, pw, 'integer')
    pool, pe, lvl = device_pool(ph, pw, nhwc(D.integer_fmaps(B, C_ROI)), n_roi)
    for b, n in enumerate(n_roi):
        assert torch.equal(pool[b, :n], ref_pool[b, :n]) and torch.equal(lvl[b, :n].long(), ref_lvl[b, :n]), b
        assert_pe_close(pe[b, :n], ref_pe[b, :n])
        assert not pool[b, n:].any() and not pe[b, n:].any() and not lvl[b, n:].any(), b


def _oracle_with_tables(cfg, rois, fmaps, pe_f, pe_t):
    """`O.roi_pooling` with the encoding tables handed in: the reference's sine / cosine table exists for C % 4 == 0 only
    (position_encoding.py:10-15 interleaves the two halves of C / 2 columns), the kernel's 4-byte path is the one for every
    other even C.  Geometry, pooling and the float64 bin means are the oracle's own (nets_ref.py:387-417)."""
    import torch.nn.functional as F
    Bn, R = rois.shape[:2]
    C = fmaps[0].shape[1]
    lvl, x1, y1, x2, y2 = O.roi_geometry(cfg, rois, [f.shape[-2] for f in fmaps], [f.shape[-1] for f in fmaps])
    ph, pw = cfg.roi_pool_h, cfg.roi_pool_w
    pool, pe = torch.zeros(Bn, R, C, ph, pw), torch.zeros(Bn, R, C, ph, pw)
    for b in range(Bn):
        for r in range(R):
            l, a, c, d, e = (int(t[b, r]) for t in (lvl, y1, y2, x1, x2))
            pool[b, r] = F.adaptive_avg_pool2d(fmaps[l][b, :, a:c + 1, d:e + 1], (ph, pw))
            s = 2 ** (l + 1)
            fr, tm = pe_f[s * a:s * c], pe_t[:s * (e - d)]
            for i in range(ph):
                pe[b, r, :C // 2, i, :] = fr[(i * len(fr)) // ph:-((-(i + 1) * len(fr)) // ph)].mean(0).float()[:, None]
            for j in range(pw):
                pe[b, r, C // 2:, :, j] = tm[(j * len(tm)) // pw:-((-(j + 1) * len(tm)) // pw)].mean(0).float()[:, None]
    return pool, pe, lvl


def test_scalar_path_with_six_channels():
    """C = 6 is no multiple of 4: 4-byte accesses.  Seeded encoding tables of 3 columns (see _oracle_with_tables)."""
    rois = all_rois()
    R = rois.shape[1]
    fmaps = D.integer_fmaps(B, 6)
    pe_f, pe_t = D.rnd('pe_f6', IMG_H, 3), D.rnd('pe_t6', IMG_W, 3)
    ref_pool, ref_pe, ref_lvl = _oracle_with_tables(O.make_cfg(roi_pool_h=3, roi_pool_w=4), rois, fmaps, pe_f.double(), pe_t.double())
    pool, pe, lvl = ops.roi_pool(nhwc(fmaps), rois.cuda(), i32([R] * B), pe_f.cuda(), pe_t.cuda(), IMG_H, IMG_W, pool_hw=(3, 4))
    pool, pe = (t.view(B, R, 3, 4, 6).permute(0, 1, 4, 2, 3).cpu() for t in (pool, pe))
    assert torch.equal(lvl.cpu().long(), ref_lvl) and torch.equal(pool, ref_pool)
    assert_pe_close(pe, ref_pe)


def test_scalar_path_with_maps_that_are_not_16_byte_aligned():
    """C = 16, every map 4 bytes past a 16-byte boundary: the 16-byte path must not be taken."""
    R = all_rois().shape[1]
    ref_pool, ref_pe, ref_lvl = oracle(3, 4, 'integer')
    shifted = []
    for f in nhwc(D.integer_fmaps(B, C_ROI)):
        buf = torch.empty(f.numel() + 1, device='cuda', dtype=torch.float32)
        m = buf[1:].view(f.shape)
        m.copy_(f)
        assert m.data_ptr() % 16 == 4 and m.is_contiguous()
        shifted.append(m)
    pool, pe, lvl = device_pool(3, 4, shifted, [R] * B)
    assert torch.equal(lvl.long(), ref_lvl) and torch.equal(pool, ref_pool)
    assert_pe_close(pe, ref_pe)


def test_2x2_gives_the_bits_of_the_retired_fixed_kernel():
    """tests/golden/roi_pool_2x2_fixed.npz holds what the retired 2 x 2-only kernel wrote on an MI355X (nbm_roi_pool of the
    library built from the commit before its removal, loaded beside the new one: profiles/roi_pool_unify.md) for
    D.modular_fmaps(3, 16), all_rois() and the counts [R, 0, 77]: `pool`, `pe` [348, 2, 2, 16] and `level` [348], the rows of
    the valid slots in slot order.  The one kernel that is left gives those bits."""
    g = load_golden('roi_pool_2x2_fixed.npz')
    rois = all_rois()
    R = rois.shape[1]
    n_roi = [R, 0, 77]
    pe_f, pe_t = _pe_tables()
    pool, pe, lvl = ops.roi_pool(nhwc(D.modular_fmaps(B, C_ROI)), rois.cuda(), i32(n_roi), pe_f, pe_t, IMG_H, IMG_W, pool_hw=(2, 2))
    valid = torch.cat([torch.arange(b * R, b * R + n) for b, n in enumerate(n_roi)])
    assert len(valid) == 348
    for got, what in ((pool, 'pool'), (pe, 'pe'), (lvl.view(-1), 'level')):
        want = torch.from_numpy(g[what])
        got = got.cpu()[valid].contiguous()
        assert got.shape == want.shape, what
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), what


def _backward_pair(ph, pw, bases=False):
    """-> list per level of (device gradient NCHW on the host, reference gradient).  `bases`: every level's gradient map is a
    non-zero share parked by another consumer; the reference is then that share + the scatter."""
    rois = all_rois()
    R = rois.shape[1]
    fm = [D.rnd(('edge_fm', i), B, C_ROI, h, w).requires_grad_(True) for i, (h, w) in enumerate(D.FMAP_HW)]
    pool, _, _ = O.roi_pooling(O.make_cfg(roi_pool_h=ph, roi_pool_w=pw), rois, fm)
    gp = D.rnd(('edge_gp', ph, pw), *pool.shape)
    pool.backward(gp)
    fmd = [f.detach().permute(0, 2, 3, 1).contiguous().cuda().requires_grad_(True) for f in fm]
    pe_f, pe_t = _pe_tables()
    pd, _, _ = Fn.RoiPool.apply(ph, pw, rois.cuda(), i32([R] * B), pe_f, pe_t, IMG_H, IMG_W, *fmd)
    share = []
    if bases:
        share = [D.rnd(('edge_base', i), *f.shape) for i, f in enumerate(fmd)]
        for f, s in zip(fmd, share):
            Fn._PARKED[f.data_ptr()] = (s.cuda(), f, None)
    try:
        pd.backward(gp.permute(0, 1, 3, 4, 2).reshape(B * R, ph, pw, C_ROI).contiguous().cuda())
    finally:
        left = len(Fn._PARKED)
        Fn._PARKED.clear()
        Fn._GRAD_ACC.clear()
    assert left == 0, 'a parked share was not taken'
    out = []
    for i in range(len(fm)):
        ref = fm[i].grad + (share[i].permute(0, 3, 1, 2) if bases else 0)
        out.append((fmd[i].grad.cpu().permute(0, 3, 1, 2), ref))
    return out


@pytest.mark.parametrize('ph,pw', SIZES)
def test_backward_against_autograd_of_the_oracle(ph, pw):
    for i, (got, ref) in enumerate(_backward_pair(ph, pw)):
        err, scale = float((got - ref).abs().max()), float(ref.abs().max())
        print(f'{ph}x{pw} level {i}: max err {err:.3e} vs scale {scale:.3e}')
        assert err <= 1e-5 * scale, f'level {i}: max err {err:.3e} vs scale {scale:.3e}'


def test_backward_scatters_into_a_parked_share():
    """A non-zero base map handed in as a parked share (the early RPN backward's): the result is base + scatter.  The same
    bound on the same scale: adding the base costs one fp32 rounding (6e-8 relative) per element."""
    for i, (got, ref) in enumerate(_backward_pair(3, 4, bases=True)):
        err, scale = float((got - ref).abs().max()), float(ref.abs().max())
        assert err <= 1e-5 * scale, f'level {i}: max err {err:.3e} vs scale {scale:.3e}'


# ----------------------------------------------------------------------------------------------- refusals
def _raw_forward(ph, pw, C):
    """nbm_roi_pool_hw called directly on -777-filled outputs -> (rc, outputs)."""
    rois = all_rois().cuda()
    R = rois.shape[1]
    fm = [torch.zeros(B, h, w, C, device='cuda') for h, w in D.FMAP_HW]
    pe_f = torch.zeros(IMG_H, max(C // 2, 1), device='cuda')
    pe_t = torch.zeros(IMG_W, max(C // 2, 1), device='cuda')
    n = i32([R] * B)
    outs = [torch.full((B * R, ph, pw, C), -777.0, device='cuda'), torch.full((B * R, ph, pw, C), -777.0, device='cuda'),
            torch.full((B, R), -777, device='cuda', dtype=torch.int32)]
    d = _lib.RoiHwDesc()
    for i, f in enumerate(fm):
        d.fmap[i], d.fh[i], d.fw[i] = f.data_ptr(), f.shape[1], f.shape[2]
    d.n_levels, d.C, d.rois, d.n_roi, d.B, d.roi_cap = len(fm), C, rois.data_ptr(), n.data_ptr(), B, R
    d.pe_f, d.pe_t, d.img_h, d.img_w = pe_f.data_ptr(), pe_t.data_ptr(), IMG_H, IMG_W
    d.pool, d.pe, d.level = (t.data_ptr() for t in outs)
    d.pool_h, d.pool_w = ph, pw
    rc = ops.lib().nbm_roi_pool_hw(ctypes.byref(d), ops._stream())
    torch.cuda.synchronize()
    return rc, outs


def _raw_backward(ph, pw, C):
    rois = all_rois().cuda()
    R = rois.shape[1]
    gf = [torch.full((B, h, w, C), -777.0, device='cuda') for h, w in D.FMAP_HW]
    level = torch.zeros(B, R, device='cuda', dtype=torch.int32)
    gpool = torch.ones(B * R, ph, pw, C, device='cuda')
    n = len(gf)
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in gf])
    fh = (ctypes.c_int * n)(*[h for h, _ in D.FMAP_HW])
    fw = (ctypes.c_int * n)(*[w for _, w in D.FMAP_HW])
    rc = ops.lib().nbm_roi_pool_hw_bwd(ptrs, fh, fw, n, C, rois.data_ptr(), level.data_ptr(), B, R, ph, pw, gpool.data_ptr(),
                                       ops._stream())
    torch.cuda.synchronize()
    return rc, gf


@pytest.mark.parametrize('ph,pw,C', [(1, 2, 16), (13, 2, 16), (3, 4, 15)], ids=['pool1x2', 'pool13x2_on_12_rows', 'odd_C'])
def test_refused_calls_write_nothing(ph, pw, C):
    rc, outs = _raw_forward(ph, pw, C)
    assert rc in (-1, -3), rc                                          # NBM_EINVAL / NBM_EUNSUPPORTED
    assert all(bool((t == -777).all()) for t in outs)
    rc, gf = _raw_backward(ph, pw, C)
    assert rc in (-1, -3), rc
    assert all(bool((t == -777).all()) for t in gf)
    # the op layer: a ValueError from the plan for the two pool sizes, the kernel's code for the odd channel count
    rois = all_rois().cuda()
    fm = [torch.zeros(B, h, w, C, device='cuda') for h, w in D.FMAP_HW]
    pe_f, pe_t = torch.zeros(IMG_H, C // 2, device='cuda'), torch.zeros(IMG_W, C // 2, device='cuda')
    with pytest.raises(ValueError if C % 2 == 0 else _lib.NbmHipError):
        ops.roi_pool(fm, rois, i32([rois.shape[1]] * B), pe_f, pe_t, IMG_H, IMG_W, pool_hw=(ph, pw))
    with pytest.raises(ValueError if C % 2 == 0 else _lib.NbmHipError):
        ops.roi_pool_bwd(torch.ones(B * rois.shape[1], ph, pw, C, device='cuda'), rois,
                         torch.zeros(B, rois.shape[1], device='cuda', dtype=torch.int32), [tuple(f.shape) for f in fm])
