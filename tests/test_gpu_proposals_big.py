"""GPU: proposals beyond 4 096 boxes per image (--pre_nms_topN / --pre_nms_topN_eval above 4 096) -- nbm_rpn_select_big and
nbm_nms_big against the references of tests/detect_ref.py (`select_ref`) and tests/merge_cpu_ref.py (`greedy_keep`, tied to
`oracle.nets_ref.greedy_nms_keep` below), against the kernels of the small route on the sizes both take, and through the
layer and the public routes.  Every comparison is exact (`torch.equal` / `np.array_equal`, scores by bit pattern)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from birdsoundclassif_amd import ops, synth          # noqa: E402
import detect_ref as D                               # noqa: E402
from helpers import filler_state_dict                # noqa: E402
from merge_cpu_ref import greedy_keep, make_boxes    # noqa: E402
from oracle import nets_ref as O                     # noqa: E402

IMG_W, IMG_H = D.IMG_W, D.IMG_H
FAIL_BELOW = 16                                      # rcnn_batch_size: fewer candidates -> "RPN failed"


def i32(v):
    return torch.tensor(list(v), dtype=torch.int32).cuda()


def key_of(scores):
    u = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def _workspace_ff(query, B, cap):
    """A workspace of the queried size full of 0xFF bytes; the size is linear in B * cap."""
    nbytes = ctypes.c_int64()
    assert query(B, cap, ctypes.byref(nbytes)) == 0
    assert 0 < nbytes.value <= 64 * B * cap + 4096
    return torch.full((nbytes.value,), 0xFF, device='cuda', dtype=torch.uint8), nbytes.value


# =============================================================================================== nbm_rpn_select_big
def _select_stale(boxes, keys, cnt, top_n, cap, seg):
    """nbm_rpn_select_big through the C entry: the workspace full of 0xFF bytes, the outputs prefilled with -7."""
    B, KA = keys.shape
    ws, ws_bytes = _workspace_ff(ops.lib().nbm_rpn_select_big_workspace, B, cap)
    sb = torch.full((B, cap, 4), -7.0, device='cuda')
    ss = torch.full((B, cap), -7.0, device='cuda')
    n_sel = torch.full((B,), -7, device='cuda', dtype=torch.int32)
    rc = ops.lib().nbm_rpn_select_big(ops._ptr(boxes), ops._ptr(keys), ops._ptr(cnt), B, KA, top_n, FAIL_BELOW, cap, ops._ptr(ws),
                                      ws_bytes, ops._ptr(sb), ops._ptr(ss), ops._ptr(n_sel), ops._ptr(seg), ops._stream())
    assert rc == 0
    return sb, ss, n_sel


def _run_select(scores, keep, top_n, cap, segments, stale=False):
    """scores / keep [B, KA] through nbm_rpn_decode (which forms the keys and counts) and the big selection, against select_ref."""
    B, KA = scores.shape
    cls, reg, anchors = D.decode_inputs_for(scores, keep)
    boxes, keys, cnt = ops.rpn_decode(cls.cuda(), reg.cuda(), anchors.cuda(), 15, IMG_W, IMG_H, 5)
    assert np.array_equal(cnt.cpu().numpy(), keep.sum(1))
    assert np.array_equal(keys.cpu().numpy().view(np.uint32), np.where(keep, key_of(scores), np.uint32(0)))
    seg = ops.segment_table(segments)
    idx, n_ref = D.select_ref(scores, keep, top_n, FAIL_BELOW, segments)
    runs = [('fresh', ops.rpn_select(boxes, keys, cnt, top_n, FAIL_BELOW, cap, segments=seg, force_big=True))]
    if stale:
        runs.append(('stale', _select_stale(boxes, keys, cnt, top_n, cap, seg)))
    boxes = boxes.cpu()
    for name, (sb, ss, n_sel) in runs:
        assert np.array_equal(n_sel.cpu().numpy(), n_ref), (name, n_sel.tolist(), n_ref.tolist())
        sb, ss = sb.cpu(), ss.cpu()
        for b in range(B):
            n = int(n_ref[b])
            assert torch.equal(sb[b, :n], boxes[b, idx[b]]), (name, b)
            assert np.array_equal(ss[b, :n].numpy().view(np.uint32), scores[b, idx[b]].view(np.uint32)), (name, b)   # bits
            assert not sb[b, n:].any() and not ss[b, n:].numpy().view(np.uint32).any(), (name, b)
    return n_ref


@pytest.mark.parametrize('ka,top_n,cap', [(23040, 4097, 8192), (23040, 6000, 8192), (23040, 8192, 8192), (23040, 12000, 16384),
                                          (23040, 23040, 32768), (38400, 38400, 65536)])
def test_select_counts_and_score_layouts(ka, top_n, cap):
    """Every score layout with the kept count of an image on top_n - 1, top_n, top_n + 1, fail_below and fail_below - 1 (capped
    at KA), five images each a segment of its own, then the first three as one model call.  The ties of `quant4` straddle the
    rank; `denormal` and `zero_one` check the bits.  On the parent the first case returns NBM_EINVAL."""
    assert ops.proposal_plan(top_n, ka) == (top_n, cap, 'big')
    counts = [min(c, ka) for c in (top_n - 1, top_n, top_n + 1, FAIL_BELOW, FAIL_BELOW - 1)]
    for layout in D.SCORE_LAYOUTS:
        scores = np.stack([D.score_layout(layout, (ka, top_n, b), ka) for b in range(5)])
        keep = np.stack([D.keep_mask((layout, ka, top_n, b), ka, m) for b, m in enumerate(counts)])
        n = _run_select(scores, keep, top_n, cap, [1] * 5, stale=True)
        assert n.tolist() == [min(counts[0], top_n), min(counts[1], top_n), min(counts[2], top_n), FAIL_BELOW, 0], (layout, n)
        n = _run_select(scores[:3], keep[:3], top_n, cap, [3])
        assert n.tolist() == [min(counts[0], top_n)] * 3, (layout, n)


def test_select_budget_above_a_small_map_keeps_every_anchor():
    """--pre_nms_topN 6000 on a map of 4 995 anchors: the plan cuts the budget to the map, every anchor is kept and comes out."""
    ka = 4995
    top_n, cap, route = ops.proposal_plan(6000, ka)
    assert (top_n, cap, route) == (4995, 8192, 'big')
    keep = np.ones((2, ka), bool)
    for layout in D.SCORE_LAYOUTS:
        scores = np.stack([D.score_layout(layout, ('all', b), ka) for b in range(2)])
        assert _run_select(scores, keep, top_n, cap, [1, 1], stale=True).tolist() == [ka, ka]
        assert _run_select(scores, keep, top_n, cap, [2]).tolist() == [ka, ka]


# =============================================================================================== nbm_nms_big
NMS_LAYOUTS = ('realistic', 'dense', 'scattered', 'identical', 'disjoint', 'chain64')
PAIR_A, PAIR_B = (np.array(p, np.float32) for p in D.THRESHOLD_PAIRS[1][1:])      # IoU exactly 0.7


SENTINEL = torch.tensor([0., 9000., 9., 9009.])      # the layouts stay below y = 5 300, the planted pairs sit at y = 5 000


def _pair_positions(n):
    """Where the pairs with IoU exactly 0.7 go (index of the first box): across 4 095 | 4 096, across a 64-box block boundary
    of the walk, and on the last two valid rows."""
    return sorted({p for p in (127, 4095, n - 2) if p >= 1 and p + 1 < n})


@functools.lru_cache(maxsize=None)
def _layout_boxes(layout, n):
    if layout in ('realistic', 'dense', 'scattered'):
        seed = int(synth.uniform(('nms_seed', layout, n), 1)[0] * 2 ** 31)
        return make_boxes(layout, n, seed=seed).astype(np.float32).reshape(-1, 4)
    b = {'identical': D.nms_identical, 'disjoint': D.nms_disjoint, 'chain64': D.nms_chain64}[layout](n).copy()
    if layout != 'chain64':
        # away from every other box (y = 5000), each pair in a column of its own: the first is kept, the second goes at 0.7
        for q, p in enumerate(_pair_positions(n)):
            off = np.array([100.0 * q, 5000.0, 100.0 * q, 5000.0], np.float32)
            b[p], b[p + 1] = PAIR_A + off, PAIR_B + off
    return b


@functools.lru_cache(maxsize=None)
def _keep(layout, n, thresh):
    return greedy_keep(_layout_boxes(layout, n), thresh)


@functools.lru_cache(maxsize=4)
def _nms_inputs(cap, n, layouts):
    """boxes [B, cap, 4] and seeded scores.  Rows beyond n hold SENTINEL, a box apart from every box of every layout: a walk
    that read one as a candidate would keep it, which adds a row and a count wherever fewer than post_n boxes survive."""
    boxes = torch.zeros(len(layouts), cap, 4)
    for b, layout in enumerate(layouts):
        bx = torch.from_numpy(_layout_boxes(layout, n))
        boxes[b, :n] = bx
        boxes[b, n:] = SENTINEL
    scores = torch.from_numpy(synth.uniform(('nms_big_scores', cap, n), len(layouts) * cap).astype(np.float32).reshape(-1, cap))
    return boxes, scores, boxes.cuda(), scores.cuda()


def _nms_stale(boxes, scores, n_in, thresh, post_n, seg):
    B, cap = scores.shape
    ws, ws_bytes = _workspace_ff(ops.lib().nbm_nms_big_workspace, B, cap)
    rois = torch.full((B, post_n, 4), -7.0, device='cuda')
    rs = torch.full((B, post_n), -7.0, device='cuda')
    n_out = torch.full((B,), -7, device='cuda', dtype=torch.int32)
    rc = ops.lib().nbm_nms_big(ops._ptr(boxes), ops._ptr(scores), ops._ptr(n_in), B, cap, ctypes.c_float(thresh), post_n,
                               ops._ptr(ws), ws_bytes, ops._ptr(rois), ops._ptr(rs), ops._ptr(n_out), ops._ptr(seg), ops._stream())
    assert rc == 0
    return rois, rs, n_out


def _check_nms(cap, n, thresh, post_n, segments, layouts=NMS_LAYOUTS):
    """One launch over the images of `layouts`, fresh and stale, against greedy_keep and the coupling rule of detect_ref.nms_ref."""
    boxes, scores, bd, sd = _nms_inputs(cap, n, layouts)
    B = len(layouts)
    keeps = [_keep(layout, n, thresh) for layout in layouts]
    n_ref = np.zeros(B, dtype=np.int64)
    b = 0
    for size in segments:
        n_ref[b:b + size] = min(post_n, min(len(k) for k in keeps[b:b + size]))
        b += size
    nd, seg = i32([n] * B), ops.segment_table(segments)
    for name, (rois, rs, n_out) in (('fresh', ops.nms_batched(bd, sd, nd, thresh, post_n, segments=seg)),
                                    ('stale', _nms_stale(bd, sd, nd, thresh, post_n, seg))):
        what = (cap, n, thresh, post_n, name)
        assert np.array_equal(n_out.cpu().numpy(), n_ref), (what, n_out.tolist(), n_ref.tolist())
        rois, rs = rois.cpu(), rs.cpu()
        for b in range(B):
            k = keeps[b][:n_ref[b]]
            assert torch.equal(rois[b, :len(k)], boxes[b, k]) and not rois[b, len(k):].any(), (what, layouts[b])
            assert torch.equal(rs[b, :len(k)], scores[b, k]) and not rs[b, len(k):].any(), (what, layouts[b])
    return n_ref, keeps


def _assert_pairs(n, keeps):
    """The planted pairs did what they were built for in the reference the kernel was compared with (threshold 0.7)."""
    for layout in ('identical', 'disjoint'):
        k = set(keeps[NMS_LAYOUTS.index(layout)])
        for p in _pair_positions(n):
            assert p in k and p + 1 not in k, (layout, n, p)


def test_greedy_keep_is_the_oracles_walk():
    """The reference of this file against `oracle.nets_ref.greedy_nms_keep` (a full IoU matrix) at n = 4 097, planted pairs included."""
    for layout in NMS_LAYOUTS:
        for thresh in (0.3, 0.7):
            assert _keep(layout, 4097, thresh) == O.greedy_nms_keep(torch.from_numpy(_layout_boxes(layout, 4097)), thresh), (layout, thresh)


@pytest.mark.parametrize('cap,n', [(8192, n) for n in (4095, 4096, 4097, 8191, 8192)] + [(32768, n) for n in (23040, 32767, 32768)])
def test_nms_sizes_layouts_and_stale_workspace(cap, n):
    """n_in around 4 096 and around cap, six box layouts as six images of one launch, thresholds 0.3 and 0.7, post_n 50 and
    1 000, a fresh workspace and one full of 0xFF bytes.  `identical` and `dense` walk every box; `disjoint` stops at post_n."""
    for thresh in (0.3, 0.7):
        for post_n in (50, 1000):
            n_out, keeps = _check_nms(cap, n, thresh, post_n, [1] * 6)
            assert n_out[4] == post_n and n_out[3] == 1 + len(_pair_positions(n)), n_out
    _assert_pairs(n, keeps)
    assert n_out[5] == min(1000, sum(1 for i in range(n) if (i // 64) % 2 == 0))           # 0.7: the even steps of the chain


@pytest.mark.parametrize('cap,thresholds', [(8192, (0.3, 0.7)), (32768, (0.7,))])
def test_nms_without_an_early_stop(cap, thresholds):
    """post_n = cap = n: the walk cannot stop early, and kept boxes beyond those held in LDS are read back from the output."""
    for thresh in thresholds:
        n_out, keeps = _check_nms(cap, cap, thresh, cap, [1] * 6)
        assert n_out[4] == cap - len(_pair_positions(cap)), n_out
    _assert_pairs(cap, keeps)


def test_nms_coupled_segment_takes_the_smallest_survivor_count():
    """One model call on `disjoint`, `dense` and `chain64` at 23 040 boxes and post_n 1 000: all three come out with `dense`'s
    survivor count, which is below post_n."""
    layouts = ('disjoint', 'dense', 'chain64')
    n_out, keeps = _check_nms(32768, 23040, 0.7, 1000, [3], layouts)
    assert len(keeps[0]) > 1000 and len(keeps[2]) > 1000 and 0 < len(keeps[1]) < 1000
    assert n_out.tolist() == [len(keeps[1])] * 3


def test_nms_counts_out_of_range_are_clamped():
    """n_in below 0 and above cap: clamped into [0, cap]."""
    cap = 8192
    boxes, scores, bd, sd = _nms_inputs(cap, cap, ('disjoint', 'disjoint'))
    rois, rs, n_out = ops.nms_batched(bd, sd, i32([-5, cap + 1000]), 0.7, 50, segments=ops.segment_table([1, 1]))
    assert n_out.tolist() == [0, 50] and not rois[0].any()
    assert torch.equal(rois[1].cpu(), boxes[1, _keep('disjoint', cap, 0.7)[:50]])


# =============================================================================================== both routes agree
def _both(fn, *args, **kw):
    small, big = fn(*args, **kw), fn(*args, force_big=True, **kw)
    for x, y in zip(small, big):
        assert torch.equal(x, y)
    return small


@pytest.mark.parametrize('top_n,cap', [(3000, 4096), (4096, 4096)])
def test_small_and_forced_big_route_give_the_same_bits(top_n, cap):
    """The sizes both routes take: selection and NMS on seeded RPN outputs, on tied scores, and on the NMS layouts."""
    cfg, cls, reg = D.rpn_inputs(2, 11)
    anchors = torch.from_numpy(O.all_anchors(cfg, 24, 64)).float().cuda()
    boxes, keys, cnt = ops.rpn_decode(cls.permute(0, 2, 3, 1).contiguous().cuda(), reg.permute(0, 2, 3, 1).contiguous().cuda(),
                                      anchors, 15, IMG_W, IMG_H, 5)
    sb, ss, n_sel = _both(ops.rpn_select, boxes, keys, cnt, top_n, FAIL_BELOW, cap)
    assert n_sel.tolist() == [top_n] * 2
    for thresh, post_n in ((0.7, 1000), (0.3, 50), (0.7, cap)):
        n_out = _both(ops.nms_batched, sb, ss, n_sel, thresh, post_n)[2]
        assert 0 < int(n_out[0]) <= post_n
    ka = 23040
    counts = (top_n - 1, top_n + 1, FAIL_BELOW - 1)
    scores = np.stack([D.score_layout('quant4', ('both', top_n, b), ka) for b in range(3)])
    keep = np.stack([D.keep_mask(('both', top_n, b), ka, m) for b, m in enumerate(counts)])
    c, r, a = D.decode_inputs_for(scores, keep)
    boxes, keys, cnt = ops.rpn_decode(c.cuda(), r.cuda(), a.cuda(), 15, IMG_W, IMG_H, 5)
    assert _both(ops.rpn_select, boxes, keys, cnt, top_n, FAIL_BELOW, cap, segments=ops.segment_table([1] * 3))[2].tolist() == \
        [top_n - 1, top_n, 0]
    for n in (top_n - 1, top_n):
        _, _, bd, sd = _nms_inputs(cap, n, NMS_LAYOUTS)
        for thresh in (0.3, 0.7):
            _both(ops.nms_batched, bd, sd, i32([n] * 6), thresh, 1000, segments=ops.segment_table([1, 2, 3]))


# =============================================================================================== the layer
@pytest.mark.parametrize('pre,training', [(6000, False), (12000, False), (6000, True)])
def test_proposal_layer_above_4096(pre, training):
    """ProposalLayer.forward_device on the seeded RPN outputs, against select_ref + greedy_keep on the device's own decode
    (which keeps the known half-pixel decode ties out of this test); and against the oracle's whole layer at 6 000 when the
    decode shows no flip."""
    from birdsoundclassif_amd.nets.layers import ProposalLayer
    from birdsoundclassif_amd.train import default_args
    post = 1000
    args = default_args(pre_nms_topN=pre, post_nms_topN=post) if training else default_args(pre_nms_topN_eval=pre, post_nms_topN_eval=post)
    pl = ProposalLayer(args, 5)
    pl.train(training)
    cfg, cls, reg = D.rpn_inputs(2, 11)
    cn, rn = cls.permute(0, 2, 3, 1).contiguous().cuda(), reg.permute(0, 2, 3, 1).contiguous().cuda()
    assert ops.proposal_plan(pre, 23040)[2] == 'big'
    rois, rs, n_roi = pl.forward_device(cn, rn)
    boxes, keys, cnt = ops.rpn_decode(cn, rn, pl.anchors(24, 64, cn.device), 15, args.img_width, args.img_height, args.min_threshold)
    boxes, keep = boxes.cpu(), keys.cpu().numpy().view(np.uint32) != 0
    assert np.array_equal(cnt.cpu().numpy(), keep.sum(1)) and int(cnt.min()) >= 12000
    scores = np.ascontiguousarray(cn.cpu().reshape(2, -1, 2)[..., 1].numpy())
    idx, n_sel = D.select_ref(scores, keep, pre, args.rcnn_batch_size, [2])
    assert n_sel.tolist() == [pre] * 2
    keeps = [greedy_keep(boxes[b, idx[b]].numpy(), args.nms_thresh) for b in range(2)]
    R = min(post, min(len(k) for k in keeps))
    assert n_roi.tolist() == [R] * 2 and R > args.rcnn_batch_size
    rois, rs = rois.cpu(), rs.cpu()
    for b in range(2):
        sel = idx[b][keeps[b][:R]]
        assert torch.equal(rois[b, :R], boxes[b, sel]) and not rois[b, R:].any(), b
        assert np.array_equal(rs[b, :R].numpy().view(np.uint32), scores[b, sel].view(np.uint32)) and not rs[b, R:].any(), b
    if pre == 6000 and not training:
        flips = int((boxes != D.decode_ref(cn.cpu().reshape(2, -1, 30), rn.cpu().reshape(2, -1, 60), pl.anchors(24, 64, cn.device).cpu(),
                                           15)[0]).sum())
        print(f'decode flips on these inputs: {flips}')
        if flips == 0:
            ref_rois, ref_rs = O.proposal_layer(O.make_cfg(pre_nms_topN_eval=pre, post_nms_topN_eval=post), cls, reg)
            assert torch.equal(rois[:, :R], ref_rois) and torch.equal(rs[:, :R], ref_rs)


# =============================================================================================== public routes
def _model(**overrides):
    from birdsoundclassif_amd.nets import build_model
    from birdsoundclassif_amd.train import default_args
    args = default_args(device='cuda', **overrides)
    model, crit = build_model(args)
    model.load_state_dict(filler_state_dict())
    return model.cuda(), crit, args


def test_detect_and_the_captured_route_give_the_same_bits_at_6000():
    from birdsoundclassif_amd import bulk
    model, _, args = _model(pre_nms_topN_eval=6000)
    model.eval()
    assert ops.proposal_plan(args.pre_nms_topN_eval, 23040) == (6000, 8192, 'big')
    pcm = torch.from_numpy(synth.clip_batch_pcm16(500, 2)).cuda()
    det = bulk.GraphedDetector(model, 2, 66150, 22050, min_score=0.05)
    try:
        c = det.census
        assert c['memset'] == c['memcpy'] == c['host'] == c['other'] == 0 and c['kernel'] > 100, c
        with torch.no_grad():
            imgs, _ = det.fe(pcm, 22050)
            imgs = imgs[:, 0][:, None].contiguous()
            d, n = model.detect(imgs, 0.3, 0.05)
        d, n = d.clone(), n.clone()
        det.pcm.copy_(pcm)
        det.replay()
        torch.cuda.synchronize()
        assert torch.equal(det.n_det, n) and torch.equal(det.det, d)
    finally:
        det.close()


def test_nms_helper_takes_5000_boxes():
    """nets_utils.nms raised NotImplementedError above 4 096 boxes."""
    from birdsoundclassif_amd.nets.util.nets_utils import nms
    n = 5000
    boxes = np.stack([_layout_boxes('realistic', n), _layout_boxes('chain64', n)])
    scores = synth.uniform('nms_helper', 2 * n).astype(np.float32).reshape(2, n)
    keeps = [greedy_keep(boxes[b], 0.7) for b in range(2)]
    R = min(300, min(len(k) for k in keeps))
    rois, rs = nms(torch.from_numpy(boxes), torch.from_numpy(scores), 0.7, 300)
    assert rois.shape == (2, R, 4)
    for b in range(2):
        assert torch.equal(rois[b], torch.from_numpy(boxes[b, keeps[b][:R]])) and torch.equal(rs[b], torch.from_numpy(scores[b, keeps[b][:R]]))


def test_one_training_step_at_6000():
    from birdsoundclassif_amd.train import build_optimizer, train_one_step
    model, crit, args = _model(pre_nms_topN=6000)
    assert ops.proposal_plan(args.pre_nms_topN, 23040)[2] == 'big'
    model.train()
    crit.train()
    opt, _ = build_optimizer(model, args)
    fpn_before = model.fpn.out_convs['0'].weight.detach().clone()
    head_before = model.head.fast_rcnn.rcnn.bbox_reg_layer.weight.detach().clone()
    img = torch.from_numpy(synth.image_batch(0, 2))
    bb, ids, lengths = synth.label_batch(0, 2)
    np.random.seed(7)
    loss = train_one_step(model, crit, opt, [img, img, bb, ids, lengths], args.clip_max_norm, 'cuda', negative_sample=False)
    torch.cuda.synchronize()
    vals = {k: float(v.detach() if torch.is_tensor(v) else v) for k, v in loss.items()}
    print(vals)
    assert vals and all(np.isfinite(v) for v in vals.values())
    assert not torch.equal(fpn_before, model.fpn.out_convs['0'].weight) and \
        not torch.equal(head_before, model.head.fast_rcnn.rcnn.bbox_reg_layer.weight)
