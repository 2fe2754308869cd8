"""GPU: the proposal / RoI / detection kernels of csrc/detect.hip at their edges -- counts on 64-bit word and power-of-two
boundaries, score ties, IoUs exactly on the threshold, RoI sizes exactly on a pyramid-level boundary, stale workspaces, empty
and failed images -- each against the CPU oracle (`oracle.nets_ref`) and the small references of tests/detect_ref.py.

Every comparison is exact (`torch.equal` / `np.array_equal`) except the RoI positional encoding (2e-6), the RoI-pool
gradients (1e-5) and box corners of `nbm_rpn_decode` whose pre-round value, recomputed in float64 from the same deltas, lies
within 1e-4 of x.5 (`expf` differs by an ulp between device and host)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from birdsoundclassif_amd import _lib, ops, synth    # noqa: E402
import detect_ref as D                               # noqa: E402
from helpers import filler_state_dict                # noqa: E402
from oracle import nets_ref as O                     # noqa: E402

IMG_W, IMG_H = D.IMG_W, D.IMG_H
FAIL_BELOW = 16                                      # rcnn_batch_size: fewer candidates -> "RPN failed"


def i32(v):
    return torch.tensor(list(v), dtype=torch.int32).cuda()


def key_of(scores):
    """The order-preserving u32 key of an fp32 score (include/nbm_hip.h): sign bit set for >= +0, all bits flipped for negatives."""
    u = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


# =============================================================================================== nbm_rpn_decode
def _check_decode(cls, reg, anchors, n_anchor, what):
    """Device decode against decode_ref.  -> number of explained half-pixel flips."""
    boxes, keys, cnt = ops.rpn_decode(cls.cuda().contiguous(), reg.cuda().contiguous(), anchors.cuda().contiguous(), n_anchor,
                                      IMG_W, IMG_H, 5)
    boxes, keys, cnt = boxes.cpu(), keys.cpu().numpy().view(np.uint32), cnt.cpu().numpy()
    ref_boxes, scores, ref_keep = D.decode_ref(cls, reg, anchors, n_anchor, 5)
    diff = boxes != ref_boxes
    n_flip = int(diff.sum())
    if n_flip:
        pre = D.preround_f64(reg, anchors)
        dist = ((pre - pre.floor()) - 0.5).abs()[diff]
        assert float((boxes - ref_boxes).abs().max()) == 1.0, what
        assert float(dist.max()) < 1e-4, f'{what}: a corner {float(dist.max()):.3e} away from x.5 came out on the other side'
    print(f'{what}: {n_flip} half-pixel flip(s) in {boxes.numel()} corners')
    # the size rule and the keys follow from the device's own boxes exactly (integer arithmetic); they are the reference's
    # wherever the boxes are
    keep = ((boxes[..., 2] - boxes[..., 0] + 1 >= 5) & (boxes[..., 3] - boxes[..., 1] + 1 >= 5)).numpy()
    same = ~diff.any(-1).numpy()
    assert np.array_equal(keep[same], ref_keep.numpy()[same]), what
    assert np.array_equal(keys, np.where(keep, key_of(scores.numpy()), np.uint32(0))), what
    assert np.array_equal(cnt, keep.sum(1)), what
    return n_flip, ref_keep


def test_decode_ragged_map_borders_and_the_size_rule():
    """5 x 7 positions x 15 anchors (KA = 525: neither a multiple of 256 nor of 64), B = 3; image 0 carries the border cases:
    boxes across each border, wholly outside, clipped width / height exactly min_threshold and one below."""
    cfg = O.make_cfg()
    B, h, w, A = 3, 5, 7, 15
    anchors = torch.from_numpy(O.all_anchors(cfg, h, w)).float()
    KA = anchors.shape[0]
    assert KA == 525 and KA % 64 and KA % 256
    cls = D.rnd('de_cls', B, h * w, A, 2, scale=1.5).softmax(-1).reshape(B, h * w, 2 * A)
    reg = D.rnd('de_reg', B, KA, 4, scale=0.25)
    rows = []
    for i, j in enumerate(np.linspace(0, KA - 1, 16).astype(int)):
        d, names = D.border_deltas(anchors[j].numpy())
        reg[0, j] = torch.from_numpy(d[i])
        rows.append((j, names[i]))
    reg = reg.reshape(B, h * w, 4 * A)
    n_flip, ref_keep = _check_decode(cls, reg, anchors, A, 'decode 5x7')
    assert n_flip == 0              # no corner of this small map is near a tie (the planted ones sit on x.25): nothing to explain
    # the planted cases did what they were built for, in the reference the kernel was just compared with
    ref_boxes = D.decode_ref(cls, reg, anchors, A, 5)[0]
    for j, name in rows:
        bx, k = ref_boxes[0, j].tolist(), bool(ref_keep[0, j])
        if name.startswith('out_'):
            assert not k and (bx[0] == bx[2] or bx[1] == bx[3]), (name, bx)
        elif 'minus_1' in name:
            assert not k and min(bx[2] - bx[0], bx[3] - bx[1]) + 1 == 4, (name, bx)
        elif '_eq_t' in name:
            assert k and min(bx[2] - bx[0], bx[3] - bx[1]) + 1 == 5, (name, bx)
        else:
            assert k and (bx[0] == 0 or bx[1] == 0 or bx[2] == IMG_W - 1 or bx[3] == IMG_H - 1), (name, bx)


def test_decode_full_map_flips_are_half_pixel_ties():
    """The 24 x 64 map (KA = 23 040), B = 3, seeded deltas: every corner that differs from the reference is explained."""
    cfg = O.make_cfg()
    anchors = torch.from_numpy(O.all_anchors(cfg, 24, 64)).float()
    _, cls, reg = D.rpn_inputs(3, 11)
    _check_decode(cls.permute(0, 2, 3, 1).contiguous().reshape(3, -1, 30), reg.permute(0, 2, 3, 1).contiguous().reshape(3, -1, 60),
                  anchors, 15, 'decode 24x64')


def test_decode_nan_deltas_keep_nothing():
    """NaN deltas and NaN scores (what a NaN feature map gives): no comparison with NaN is true, so no anchor is kept."""
    cfg = O.make_cfg()
    anchors = torch.from_numpy(O.all_anchors(cfg, 5, 7)).float()
    cls = torch.full((2, 35, 30), float('nan'))
    reg = torch.full((2, 35, 60), float('nan'))
    reg[1] = 0.0
    assert D.decode_ref(cls, reg, anchors, 15)[2].sum(1).tolist()[0] == 0
    _, keys, cnt = ops.rpn_decode(cls.cuda(), reg.cuda(), anchors.cuda(), 15, IMG_W, IMG_H, 5)
    assert cnt.tolist()[0] == 0 and cnt.tolist()[1] > 0 and not keys[0].any()


# =============================================================================================== nbm_rpn_select
def _run_select(scores, keep, top_n, cap, segments):
    """scores / keep [B, KA] through nbm_rpn_decode (which forms the keys and counts) and nbm_rpn_select, against select_ref."""
    B, KA = scores.shape
    cls, reg, anchors = D.decode_inputs_for(scores, keep)
    boxes, keys, cnt = ops.rpn_decode(cls.cuda(), reg.cuda(), anchors.cuda(), 15, IMG_W, IMG_H, 5)
    assert np.array_equal(cnt.cpu().numpy(), keep.sum(1))
    assert np.array_equal(keys.cpu().numpy().view(np.uint32), np.where(keep, key_of(scores), np.uint32(0)))
    sb, ss, n_sel = ops.rpn_select(boxes, keys, cnt, top_n, FAIL_BELOW, cap, segments=ops.segment_table(segments))
    idx, n_ref = D.select_ref(scores, keep, top_n, FAIL_BELOW, segments)
    assert np.array_equal(n_sel.cpu().numpy(), n_ref), (n_sel.tolist(), n_ref.tolist())
    boxes, sb, ss = boxes.cpu(), sb.cpu(), ss.cpu()
    for b in range(B):
        n = int(n_ref[b])
        assert torch.equal(sb[b, :n], boxes[b, idx[b]]), b
        assert np.array_equal(ss[b, :n].numpy().view(np.uint32), scores[b, idx[b]].view(np.uint32)), b      # bits: -0.0, denormals
        assert not sb[b, n:].any() and not ss[b, n:].numpy().view(np.uint32).any(), b
    return n_ref


@pytest.mark.parametrize('ka', [23040, 4995, 450])
@pytest.mark.parametrize('top_n,cap', [(500, 512), (512, 512), (3000, 4096), (4096, 4096)])
def test_select_counts_and_score_layouts(top_n, cap, ka):
    """Every score layout with the kept count of an image on top_n - 1, top_n, top_n + 1, fail_below and fail_below - 1 (five
    images, each a segment of its own).  KA = 23 040 (the model's), 4 995 (no multiple of 1024), 450 (below every top_n)."""
    assert ka % 15 == 0 and (ka == 23040 or ka % 1024)
    counts = [min(c, ka) for c in (top_n - 1, top_n, top_n + 1, FAIL_BELOW, FAIL_BELOW - 1)]
    for layout in D.SCORE_LAYOUTS:
        scores = np.stack([D.score_layout(layout, (ka, top_n, b), ka) for b in range(5)])
        keep = np.stack([D.keep_mask((layout, ka, top_n, b), ka, m) for b, m in enumerate(counts)])
        n = _run_select(scores, keep, top_n, cap, [1] * 5)
        assert n.tolist() == [min(counts[0], top_n), min(counts[1], top_n), min(counts[2], top_n), FAIL_BELOW, 0], (layout, n)
        # one model call on the first three images: the smallest count rules
        n = _run_select(scores[:3], keep[:3], top_n, cap, [3])
        assert n.tolist() == [min(counts[0], top_n)] * 3, (layout, n)


def test_select_every_anchor_kept_and_dropped_zero_scores():
    """All anchors kept with N == cap == 4096 of 4 995 equal scores (pure index order); and kept anchors of score exactly +0.0
    (key 0x80000000) beside dropped ones (key 0) with N == the kept count: the last kept zero is in, no dropped anchor is."""
    ka = 4995
    scores = np.full((1, ka), 0.5, np.float32)
    _run_select(scores, np.ones((1, ka), bool), 4096, 4096, [1])
    scores = np.zeros((2, ka), np.float32)
    keep = np.stack([D.keep_mask(('zeros', b), ka, m) for b, m in enumerate((300, 512))])
    assert _run_select(scores, keep, 512, 512, [1, 1]).tolist() == [300, 512]


def test_select_segment_tables_on_the_same_six_images():
    """Segments [1, 3, 2] and [6] on the same six images, image 2 below fail_below: only its own segment fails."""
    ka = 23040
    counts = [700, 650, FAIL_BELOW - 1, 600, 450, 480]
    scores = np.stack([D.score_layout('quant4', ('seg', b), ka) for b in range(6)])
    keep = np.stack([D.keep_mask(('seg', b), ka, m) for b, m in enumerate(counts)])
    assert _run_select(scores, keep, 500, 512, [1, 3, 2]).tolist() == [500, 0, 0, 0, 450, 450]
    assert _run_select(scores, keep, 500, 512, [6]).tolist() == [0] * 6
    assert _run_select(scores, keep, 500, 512, [2, 1, 1, 2]).tolist() == [500, 500, 0, 500, 450, 450]


# =============================================================================================== nbm_nms_batched
def _nms_stale(boxes, scores, n_in, thresh, post_n, segments):
    """nbm_nms_batched through the C entry with workspaces that hold all-ones bits from "an earlier launch".
    What this can show: a word inside the triangle [row block <= column block < ceil(n / 64)] that the mask kernel does not write
    (the scan then ORs ones into `removed`), and a result row or count that is not written.  What it cannot show: reads of
    words below the diagonal or at and beyond ceil(n / 64) -- those would only set bits of boxes already visited or of j >= n,
    which the walk never looks at."""
    B, cap = scores.shape
    mask_ws = torch.full((B * cap * (cap // 64),), -1, device='cuda', dtype=torch.int64)
    keep_ws = torch.full((B * (cap + 1),), -1, device='cuda', dtype=torch.int32)
    rois = torch.full((B, post_n, 4), -7.0, device='cuda')
    rs = torch.full((B, post_n), -7.0, device='cuda')
    n_out = torch.full((B,), -7, device='cuda', dtype=torch.int32)
    rc = ops.lib().nbm_nms_batched(ops._ptr(boxes), ops._ptr(scores), ops._ptr(n_in), B, cap, ctypes.c_float(thresh), post_n,
                                   ops._ptr(mask_ws), ops._ptr(keep_ws), ops._ptr(rois), ops._ptr(rs), ops._ptr(n_out),
                                   ops._ptr(segments), ops._stream())
    assert rc == 0
    return rois, rs, n_out


def _check_nms(boxes, n_in, thresh, post_n, segments, what):
    """boxes [B, cap, 4] (rows beyond n_in hold a box that would suppress everything if it were read)."""
    B, cap = boxes.shape[:2]
    scores = torch.from_numpy(synth.uniform(('nms_scores', what), B * cap).astype(np.float32).reshape(B, cap))
    ref_rois, keeps, ref_n = D.nms_ref(boxes, n_in, thresh, post_n, segments)
    bd, sd, nd, seg = boxes.cuda(), scores.cuda(), i32(n_in), ops.segment_table(segments)
    for name, (rois, rs, n_out) in (('fresh', ops.nms_batched(bd, sd, nd, thresh, post_n, segments=seg)),
                                    ('stale', _nms_stale(bd, sd, nd, thresh, post_n, seg))):
        assert np.array_equal(n_out.cpu().numpy(), ref_n), (what, name, n_out.tolist(), ref_n.tolist())
        assert torch.equal(rois.cpu(), ref_rois), (what, name)
        rs = rs.cpu()
        for b in range(B):
            assert torch.equal(rs[b, :len(keeps[b])], scores[b, keeps[b]]) and not rs[b, len(keeps[b]):].any(), (what, name, b)
    return ref_n


NMS_LAYOUTS = ('realistic', 'dense', 'scattered', 'identical', 'disjoint', 'chain64')


def _nms_layout(layout, n):
    from merge_cpu_ref import make_boxes
    if layout in ('realistic', 'dense', 'scattered'):
        seed = int(synth.uniform(('nms_seed', layout, n), 1)[0] * 2 ** 31)
        return make_boxes(layout, n, seed=seed).astype(np.float32).reshape(-1, 4)
    return {'identical': D.nms_identical, 'disjoint': D.nms_disjoint, 'chain64': D.nms_chain64}[layout](n)


@pytest.mark.parametrize('cap,post_n,n', [(512, 50, n) for n in (0, 1, 63, 64, 65, 127, 128, 129, 500, 512)] +
                         [(4096, 1000, n) for n in (2999, 3000, 4095, 4096)])
def test_nms_word_boundaries_layouts_and_stale_workspace(cap, post_n, n):
    """n_in around the 64-bit word boundaries, six box layouts as six independent images of one launch, at the merge tests'
    threshold 0.3 (their planted pairs sit one ulp around it) and the model's 0.7 -- with a fresh workspace and with one full of
    stale bits.  Rows beyond n_in hold the image's first box: read by mistake, they would change the walk."""
    boxes = torch.zeros(len(NMS_LAYOUTS), cap, 4)
    for b, layout in enumerate(NMS_LAYOUTS):
        bx = torch.from_numpy(_nms_layout(layout, n))
        boxes[b, :n] = bx
        boxes[b, n:] = bx[0] if n else torch.tensor([0., 0., 2000., 2000.])
    if cap == 512:
        for thresh in (0.3, 0.7):
            n_out = _check_nms(boxes, [n] * 6, thresh, post_n, [1] * 6, (cap, n, thresh))
            assert n_out[3] == min(n, 1) and n_out[4] == min(n, post_n), n_out
        n_chain = n_out[5]
    else:       # (the 4096 x 4096 IoU matrices of the CPU reference cost time: each layout at the threshold it was built for)
        _check_nms(boxes[:3], [n] * 3, 0.3, post_n, [1] * 3, (cap, n, 0.3))
        n_out = _check_nms(boxes[3:], [n] * 3, 0.7, post_n, [1] * 3, (cap, n, 0.7))
        assert n_out[0] == 1 and n_out[1] == min(n, post_n), n_out
        n_chain = n_out[2]
    assert n_chain == min(post_n, sum(1 for i in range(n) if (i // 64) % 2 == 0))          # 0.7: the even steps of the chain


def test_nms_iou_exactly_on_the_threshold_suppresses():
    for thresh, a, b in D.THRESHOLD_PAIRS:
        boxes = torch.zeros(1, 64, 4)
        boxes[0, 0], boxes[0, 1] = torch.tensor(a), torch.tensor(b)
        assert _check_nms(boxes, [2], thresh, 50, [1], ('pair', thresh)).tolist() == [1]
        # the same pair across a word boundary
        boxes = torch.zeros(1, 128, 4)
        boxes[0, :64] = torch.from_numpy(D.nms_disjoint(64)) + 5000
        boxes[0, 63], boxes[0, 64] = torch.tensor(a), torch.tensor(b)
        assert _check_nms(boxes, [65], thresh, 64, [1], ('pair64', thresh)).tolist() == [64]


def test_nms_counts_differ_per_image_in_segments():
    """Six images with different n_in in segments [2, 1, 3]: n_out is the minimum over the segment, rows beyond it are zero."""
    n_in = [129, 64, 0, 500, 65, 512]
    layouts = ['disjoint', 'chain64', 'identical', 'realistic', 'disjoint', 'chain64']
    boxes = torch.zeros(6, 512, 4)
    for b, (layout, n) in enumerate(zip(layouts, n_in)):
        boxes[b, :n] = torch.from_numpy(_nms_layout(layout, n))
    n_out = _check_nms(boxes, n_in, 0.7, 100, [2, 1, 3], 'segments')
    assert n_out.tolist() == [64, 64, 0, 65, 65, 65]
    assert _check_nms(boxes, n_in, 0.7, 100, [6], 'one segment').tolist() == [0] * 6


# =============================================================================================== nbm_roi_pool / nbm_roi_tiles
C_ROI = 16


def _pe_tables():
    from birdsoundclassif_amd.nets.position_encoding import one_dimension_positional_encoding as pe1d
    return pe1d(IMG_H, C_ROI // 2).cuda().contiguous(), pe1d(IMG_W, C_ROI // 2).cuda().contiguous()


def _all_rois():
    """[3, n, 4]: the level-boundary RoIs (one placement per image) followed by the edge RoIs (in every image)."""
    return torch.cat([D.boundary_rois(), D.edge_rois().expand(3, -1, -1)], 1).contiguous()


def _roi_pool_device(rois, n_roi, fmaps):
    pe_f, pe_t = _pe_tables()
    pool, pe, lvl = ops.roi_pool([f.permute(0, 2, 3, 1).contiguous().cuda() for f in fmaps], rois.cuda(), i32(n_roi), pe_f, pe_t,
                                 IMG_H, IMG_W)
    B, R = rois.shape[:2]
    return (pool.view(B, R, 2, 2, C_ROI).permute(0, 1, 4, 2, 3).cpu(), pe.view(B, R, 2, 2, C_ROI).permute(0, 1, 4, 2, 3).cpu(),
            lvl.cpu())


def test_roi_level_on_every_boundary_size_and_exact_pool():
    """Every RoI size that sits exactly on a pyramid-level boundary (+- 1 in width), three placements; x.5 quotients, RoIs on
    x = 1023 / y = 374, zero-area and one-pixel RoIs in the corners.  `level` equal for every RoI; on the integer maps `pool`
    is bit-equal (an off-by-one window is another integer); `pe` within 2e-6."""
    cfg = O.make_cfg()
    rois = _all_rois()
    B, R = rois.shape[:2]
    fmaps = D.integer_fmaps(B, C_ROI)
    ref_pool, ref_pe, ref_lvl = O.roi_pooling(cfg, rois, fmaps)
    pool, pe, lvl = _roi_pool_device(rois, [R] * B, fmaps)
    bad = (lvl.long() != ref_lvl).nonzero().tolist()
    assert not bad, f'{len(bad)} RoIs on another pyramid level, first: {rois[bad[0][0], bad[0][1]].tolist()} -> ' \
                    f'{int(lvl[bad[0][0], bad[0][1]])} (reference {int(ref_lvl[bad[0][0], bad[0][1]])})'
    assert torch.equal(pool, ref_pool), f'{int((pool != ref_pool).any(-1).any(-1).any(-1).sum())} RoIs pooled another window'
    err = (pe - ref_pe).abs()
    assert bool((err <= 2e-6 + 2e-6 * ref_pe.abs()).all()), float(err.max())
    # a pseudo-random integer map as well: errors that cancel inside a bin of the linear map do not cancel here.  torch's
    # adaptive pooling divides the (exact) bin sum by the bin's height and then its width, the kernel by the area at once, so
    # this comparison is to an ulp (2e-7 relative) and not to the bit; a wrong pixel moves a bin mean by 1 / 400 at the least
    fmaps = D.modular_fmaps(B, C_ROI)
    ref_pool = O.roi_pooling(cfg, rois, fmaps)[0]
    pool = _roi_pool_device(rois, [R] * B, fmaps)[0]
    assert bool(((pool - ref_pool).abs() <= 2e-7 * ref_pool.abs()).all()), float((pool - ref_pool).abs().max())


def test_roi_counts_differ_per_image_and_rows_beyond_stay_zero():
    cfg = O.make_cfg()
    rois = _all_rois()
    B, R = rois.shape[:2]
    fmaps = D.integer_fmaps(B, C_ROI)
    n_roi = [R, 0, 77]
    pool, pe, lvl = _roi_pool_device(rois, n_roi, fmaps)
    ref_pool, _, ref_lvl = O.roi_pooling(cfg, rois, fmaps)
    for b, n in enumerate(n_roi):
        assert torch.equal(pool[b, :n], ref_pool[b, :n]) and torch.equal(lvl[b, :n].long(), ref_lvl[b, :n]), b
        assert not pool[b, n:].any() and not pe[b, n:].any() and not lvl[b, n:].any(), b


@pytest.mark.parametrize('dilate', [0, 1, 2])
@pytest.mark.parametrize('with_skip', [False, True])
def test_roi_tiles_equal_the_set_under_the_oracle_windows(dilate, with_skip):
    """nbm_roi_tiles on the same RoIs, levels 0 and 1: the listed 2 x 2 tiles are exactly the set under the oracle's windows
    (each once; a 128-entry block holds one image, ascending, -1 padded)."""
    rois = _all_rois()
    B, R = rois.shape[:2]
    n_roi = [R, 0, 150]
    rois_d, n_roi_d = rois.cuda(), i32(n_roi)
    nl = len(D.FMAP_HW)
    fh = (ctypes.c_int * nl)(*[h for h, _ in D.FMAP_HW])
    fw = (ctypes.c_int * nl)(*[w for _, w in D.FMAP_HW])
    for level in (0, 1):
        H, W = D.FMAP_HW[level]
        thw = ((H + 1) // 2) * ((W + 1) // 2)
        skip = (synth.uniform(('skip', level), thw) < 0.3) if with_skip else None
        skip_d = torch.from_numpy(skip.astype(np.uint8)).cuda() if with_skip else None
        n_cap = B * (-(-thw // 128)) * 128
        tiles = torch.full((n_cap,), -5, device='cuda', dtype=torch.int32)
        n_blocks = torch.full((1,), -5, device='cuda', dtype=torch.int32)
        rc = ops.lib().nbm_roi_tiles(ops._ptr(rois_d), ops._ptr(n_roi_d), B, R, nl, level, fh, fw,
                                     ops._ptr(skip_d) if with_skip else None, dilate, ops._ptr(tiles), ops._ptr(n_blocks), ops._stream())
        assert rc == 0
        ref = D.tiles_ref(rois, n_roi, level, dilate, skip)
        nb = int(n_blocks.item())
        got = tiles[:nb * 128].cpu().numpy().reshape(nb, 128)
        listed = got[got >= 0]
        assert len(listed) == len(set(listed.tolist())) and set(listed.tolist()) == ref, (level, len(listed), len(ref))
        assert len(ref) > 100
        for blk in got:
            v = blk[blk >= 0]
            assert len(v) and (blk[:len(v)] >= 0).all() and (blk[len(v):] == -1).all() and (np.diff(v) > 0).all()
            assert len(set((v // thw).tolist())) == 1


def test_roi_pool_backward_on_the_edge_rois():
    """Fn.RoiPool's backward pass on the same RoIs against autograd of the oracle's pooling (1e-5 of the largest gradient,
    the tolerance of test_roi_pool_backward)."""
    from birdsoundclassif_amd.nets import functional as Fn
    cfg = O.make_cfg()
    rois = _all_rois()
    B, R = rois.shape[:2]
    fm = [D.rnd(('edge_fm', i), B, C_ROI, h, w).requires_grad_(True) for i, (h, w) in enumerate(D.FMAP_HW)]
    pool, _, _ = O.roi_pooling(cfg, rois, fm)
    gp = D.rnd('edge_gp', *pool.shape)
    pool.backward(gp)
    fmd = [f.detach().permute(0, 2, 3, 1).contiguous().cuda().requires_grad_(True) for f in fm]
    pe_f, pe_t = _pe_tables()
    pd, _, _ = Fn.RoiPool.apply(2, 2, rois.cuda(), i32([R] * B), pe_f, pe_t, IMG_H, IMG_W, *fmd)
    pd.backward(gp.permute(0, 1, 3, 4, 2).reshape(B * R, 2, 2, C_ROI).contiguous().cuda())
    for i in range(len(fm)):
        assert fm[i].grad is not None
        got, ref = fmd[i].grad.cpu().permute(0, 3, 1, 2), fm[i].grad
        err, scale = float((got - ref).abs().max()), float(ref.abs().max())
        assert err <= 1e-5 * scale, f'level {i}: max err {err:.3e} vs scale {scale:.3e}'


def test_the_2x2_abi_entries_forward_to_the_general_ones():
    """nbm_roi_pool through a nbm_roi_desc gives the bits of ops.roi_pool(..., pool_hw=(2, 2)) (nbm_roi_pool_hw); nbm_roi_pool_bwd
    equals nbm_roi_pool_hw_bwd(..., 2, 2, ...) within 1e-5 of the largest gradient (the atomic scatter's order is not fixed)."""
    rois = _all_rois().cuda()
    B, R = rois.shape[:2]
    fm = [D.rnd(('edge_fm', i), B, C_ROI, h, w).permute(0, 2, 3, 1).contiguous().cuda() for i, (h, w) in enumerate(D.FMAP_HW)]
    pe_f, pe_t = _pe_tables()
    n_roi = i32([R, 0, 77])
    ref = ops.roi_pool(fm, rois, n_roi, pe_f, pe_t, IMG_H, IMG_W, pool_hw=(2, 2))
    outs = [torch.zeros_like(t) for t in ref]
    d = _lib.RoiDesc()
    for i, f in enumerate(fm):
        d.fmap[i], d.fh[i], d.fw[i] = f.data_ptr(), f.shape[1], f.shape[2]
    d.n_levels, d.C, d.rois, d.n_roi, d.B, d.roi_cap = len(fm), C_ROI, rois.data_ptr(), n_roi.data_ptr(), B, R
    d.pe_f, d.pe_t, d.img_h, d.img_w = pe_f.data_ptr(), pe_t.data_ptr(), IMG_H, IMG_W
    d.pool, d.pe, d.level = (t.data_ptr() for t in outs)
    assert ops.lib().nbm_roi_pool(ctypes.byref(d), ops._stream()) == 0
    for got, want, what in zip(outs, ref, ('pool', 'pe', 'level')):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), what
    assert bool(ref[0].any()) and bool(ref[2].any())

    level = ops.roi_pool(fm, rois, i32([R] * B), pe_f, pe_t, IMG_H, IMG_W)[2]
    gpool = D.rnd('edge_gp', B * R, 2, 2, C_ROI).cuda()
    n = len(fm)
    fh = (ctypes.c_int * n)(*[h for h, _ in D.FMAP_HW])
    fw = (ctypes.c_int * n)(*[w for _, w in D.FMAP_HW])
    maps = []
    for hw in (False, True):
        gf = [torch.zeros_like(f) for f in fm]
        ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in gf])
        head = (ptrs, fh, fw, n, C_ROI, rois.data_ptr(), level.data_ptr(), B, R)
        if hw:
            rc = ops.lib().nbm_roi_pool_hw_bwd(*head, 2, 2, gpool.data_ptr(), ops._stream())
        else:
            rc = ops.lib().nbm_roi_pool_bwd(*head, gpool.data_ptr(), ops._stream())
        assert rc == 0
        maps.append(gf)
    for i, (got, want) in enumerate(zip(*maps)):
        err, scale = float((got - want).abs().max()), float(want.abs().max())
        assert scale > 0 and err <= 1e-5 * scale, f'level {i}: max err {err:.3e} vs scale {scale:.3e}'


def test_zero_roi_windows_zeroes_exactly_the_oracle_windows():
    """nbm_zero_roi_windows on maps filled with -777, levels 0 and 1: the pixels under the oracle's 2 x 2 windows of that level
    (O.roi_geometry, the windows of D.tiles_ref) are zero, every other value is still -777; slots on another level touch nothing."""
    rois = _all_rois()
    B, R = rois.shape[:2]
    lvl, x1, y1, x2, y2 = O.roi_geometry(O.make_cfg(), rois, [h for h, _ in D.FMAP_HW], [w for _, w in D.FMAP_HW])
    rois_d, lvl_d = rois.cuda(), lvl.int().cuda()
    for level in (0, 1):
        H, W = D.FMAP_HW[level]
        want = torch.full((B, H, W), -777.0)
        for b in range(B):
            for r in range(R):
                if int(lvl[b, r]) == level:
                    want[b, int(y1[b, r]):int(y2[b, r]) + 1, int(x1[b, r]):min(int(x2[b, r]), W - 1) + 1] = 0.0
        assert 100 < int((want == 0).sum()) < want.numel() // 2
        for levels, expect in ((lvl_d, want), (torch.full_like(lvl_d, 2), torch.full_like(want, -777.0))):
            g = torch.full((B, H, W, C_ROI), -777.0, device='cuda')
            rc = ops.lib().nbm_zero_roi_windows(ops._ptr(g), H, W, C_ROI, ops._ptr(rois_d), ops._ptr(levels), B, R, level,
                                                ops._stream())
            assert rc == 0
            assert torch.equal(g.cpu(), expect[..., None].expand(-1, -1, -1, C_ROI)), level


# =============================================================================================== nbm_rcnn_post
def _check_post(rois, n_roi, reg, cls, nms_thresh, min_score, what, proposal_number=50):
    B, cap = rois.shape[:2]
    ref = D.post_ref(rois, n_roi, reg, cls, nms_thresh, min_score, proposal_number)
    det, n_det = ops.rcnn_post(rois.cuda(), i32(n_roi), reg.reshape(B * cap, -1).cuda(), cls.reshape(B * cap, -1).cuda(), IMG_W, IMG_H,
                               nms_thresh, min_score, proposal_number)
    det, n_det = det.cpu(), n_det.cpu().tolist()
    assert n_det == [len(r) for r in ref], (what, n_det, [len(r) for r in ref])
    for b in range(B):
        assert torch.equal(det[b, :n_det[b]], ref[b]), (what, b)
        assert not det[b, n_det[b]:].any(), (what, b)
    return n_det


def test_post_roi_counts_around_the_powers_of_two():
    """R in {0, 1, 2, 3, 50, 63, 64, 65, 1023, 1024}, all in one launch (roi_cap = POST_MAX = 1024), random head outputs."""
    counts = [0, 1, 2, 3, 50, 63, 64, 65, 1023, 1024]
    rois, reg, cls = D.post_random('counts', len(counts), 1024)
    for ms in (0.05, 0.3):
        n_det = _check_post(rois, counts, reg, cls, 0.3, ms, ('counts', ms))
        assert n_det[0] == 0 and sum(n_det) > 100
    rois, reg, cls = D.post_random('cap64', 3, 64)
    _check_post(rois, [64, 63, 1], reg, cls, 0.3, 0.05, 'cap 64')


def test_post_background_ties_and_identical_rows():
    rois, reg, cls = D.post_random('bg', 4, 64)
    cls[0, :, 0] = 1.0                                             # image 0: every RoI background
    cls[1, :, 0] = cls[1, :, 1:].max(-1)[0]                        # image 1: background tied with the best class -> background wins
    cls[2, :] = cls[2, :1]                                         # image 2: identical class rows -> order by RoI index
    cls[2, :, 0] = 0.0
    cls[3, :, 0] = 0.0                                             # image 3: no background anywhere
    n_det = _check_post(rois, [64] * 4, reg, cls, 0.3, 0.05, 'background')
    assert n_det[0] == 0 and n_det[1] == 0 and n_det[2] > 1 and n_det[3] > 1


def test_post_truncation_to_proposal_number_and_strict_min_score():
    """200 disjoint boxes of one class, descending scores: exactly proposal_number = 50 rows; min_score between the 30th and
    the 31st score: 30 rows; min_score equal to the 30th score: 29 rows (strict >)."""
    rois, reg, cls, scores = D.post_disjoint_200()
    assert _check_post(rois, [200], reg, cls, 0.3, 0.05, 'truncate') == [50]
    assert _check_post(rois, [200], reg, cls, 0.3, 0.5 * (float(scores[29]) + float(scores[30])), 'truncate then filter') == [30]
    assert _check_post(rois, [200], reg, cls, 0.3, float(scores[29]), 'score == min_score') == [29]
    assert _check_post(rois, [200], reg, cls, 0.3, 0.05, 'proposal_number 7', proposal_number=7) == [7]


def test_post_decoded_boxes_clip_on_every_border():
    """Deltas that push the decoded boxes across each border of the image (and far outside)."""
    rois, reg, cls = D.post_random('clip', 2, 64)
    reg = reg * 4.0
    cls[..., 0] = 0.0
    ref = D.post_ref(rois, [64, 64], reg, cls, 0.3, 0.05)
    rows = torch.cat(ref)
    assert bool((rows[:, 1] == 0).any() and (rows[:, 2] == 0).any() and (rows[:, 3] == IMG_W - 1).any() and (rows[:, 4] == IMG_H - 1).any())
    _check_post(rois, [64, 64], reg, cls, 0.3, 0.05, 'clip')


# =============================================================================================== a NaN image through the detector
@pytest.fixture(scope='module')
def model():
    from birdsoundclassif_amd.nets import build_model
    from birdsoundclassif_amd.train import default_args
    m, _ = build_model(default_args(device='cuda'))
    m.load_state_dict(filler_state_dict())
    return m.cuda().eval()


def test_nan_image_fails_the_rpn_like_the_reference(model):
    """A silent file gives an all-NaN image (test_silent_file_is_nan_like_reference).  The reference's first stage keeps no
    anchor for it (every comparison with NaN is false): "RPN failed".  The device must take the same path: no RoIs, no
    detections."""
    x = torch.full((1, 1, IMG_H, IMG_W), float('nan'))
    with torch.no_grad():
        ref = O.forward_first_stage(filler_state_dict(), O.make_cfg(), x)
    assert ref['rois'].numel() == 0
    with torch.no_grad():
        out = model.forward_first_stage(x.cuda())
        assert out['rois'].numel() == 0
        det, n_det = model.detect(x.cuda(), min_score=0.05)
    assert n_det.tolist() == [0] and not det.any()
    assert all(len(v['bbox_coord']) == 0 for v in model(x.cuda(), min_score=0.05)[0].values())


def test_one_nan_pixel_fails_the_rpn_like_the_reference(model):
    """A single NaN pixel in an otherwise ordinary image: in the reference it reaches every RPN output (the attention levels
    and the top-down path spread it), so the first stage fails just the same.  The device decides from the image."""
    x = torch.from_numpy(synth.image_batch(0, 1))[:, None].clone()
    with torch.no_grad():
        assert int(model.detect(x.cuda(), min_score=0.05)[1][0]) > 0          # the clean image has detections
    x[0, 0, IMG_H // 2, IMG_W // 2] = float('nan')
    with torch.no_grad():
        ref = O.forward_first_stage(filler_state_dict(), O.make_cfg(), x)
    assert ref['rois'].numel() == 0 and bool(torch.isnan(ref['rpn_cls_scores']).all())
    with torch.no_grad():
        assert model.forward_first_stage(x.cuda())['rois'].numel() == 0
        det, n_det = model.detect(x.cuda(), min_score=0.05)
    assert n_det.tolist() == [0] and not det.any()


def test_nan_image_does_not_touch_its_launch_mates(model):
    """B = 4, every image a model call of its own, image 2 all-NaN: it fails alone; images 0, 1, 3 give the bits they give
    without it."""
    x = torch.from_numpy(synth.image_batch(0, 4))[:, None].cuda()
    with torch.no_grad():
        clean_det, clean_n = model.detect(x[[0, 1, 3]].contiguous(), min_score=0.05, independent=True)
        x[2] = float('nan')
        det, n = model.detect(x, min_score=0.05, independent=True)
    assert int(n[2]) == 0 and not det[2].any()
    assert torch.equal(n[[0, 1, 3]], clean_n) and torch.equal(det[[0, 1, 3]], clean_det) and int(clean_n.sum()) > 0
    with torch.no_grad():                            # one model call on the four: the NaN image fails everybody (reference semantics)
        _, n = model.detect(x, min_score=0.05)
    assert n.tolist() == [0] * 4
