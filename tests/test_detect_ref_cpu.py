"""CPU: the references and input builders of tests/detect_ref.py, checked against `oracle.nets_ref` -- the references must say
what the oracle says, and every builder must meet on the CPU the condition its GPU test relies on."""
import numpy as np
import torch

import detect_ref as D
from oracle import nets_ref as O


def test_select_ref_equals_the_selection_inside_the_proposal_layer():
    for training in (False, True):
        cfg, cls, reg = D.rpn_inputs(2, 3)
        ref_rois, ref_scores = O.proposal_layer(cfg, cls, reg, training=training)
        anchors = torch.from_numpy(O.all_anchors(cfg, 24, 64)).float()
        boxes, scores, keep = D.decode_ref(cls.permute(0, 2, 3, 1).reshape(2, -1, 30), reg.permute(0, 2, 3, 1).reshape(2, -1, 60),
                                           anchors, 15, cfg.min_threshold)
        pre, post = (cfg.pre_nms_topN, cfg.post_nms_topN) if training else (cfg.pre_nms_topN_eval, cfg.post_nms_topN_eval)
        idx, n_sel = D.select_ref(scores.numpy(), keep.numpy(), pre, cfg.rcnn_batch_size, [2])
        assert n_sel.tolist() == [pre, pre]
        sel = torch.from_numpy(np.stack(idx))
        bx = torch.gather(boxes, 1, sel[..., None].expand(-1, -1, 4))
        rois, rs, _ = O.batched_nms(bx, torch.gather(scores, 1, sel), cfg.nms_thresh, post)
        assert torch.equal(rois, ref_rois) and torch.equal(rs, ref_scores)


def test_select_ref_ties_segments_and_failure():
    s = np.array([[0.5, 0.5, 0.25, 0.5, 0.75, 0.5], [0.1, 0.2, 0.3, 0.4, 0.5, 0.6], [0.9, 0.8, 0.7, 0.6, 0.5, 0.4]], np.float32)
    k = np.array([[1, 1, 1, 0, 1, 1], [1, 1, 1, 1, 1, 1], [0, 1, 0, 0, 0, 0]], bool)
    idx, n = D.select_ref(s, k, 3, 2, [1, 1, 1])
    assert n.tolist() == [3, 3, 0] and idx[0].tolist() == [4, 0, 1] and idx[1].tolist() == [5, 4, 3] and len(idx[2]) == 0
    idx, n = D.select_ref(s, k, 3, 2, [2, 1])
    assert n.tolist() == [3, 3, 0]
    idx, n = D.select_ref(s, k, 3, 2, [1, 2])                        # image 2 fails its launch-mate of the same segment only
    assert n.tolist() == [3, 0, 0]
    idx, n = D.select_ref(s, k, 3, 1, [3])
    assert n.tolist() == [1, 1, 1] and [i.tolist() for i in idx] == [[4], [5], [1]]


def test_score_layouts_meet_their_conditions():
    n = 23040
    for name in D.SCORE_LAYOUTS:
        s = D.score_layout(name, 0, n)
        assert s.dtype == np.float32 and s.shape == (n,) and (s >= 0).all() and np.isfinite(s).all()
    assert len(np.unique(D.score_layout('quant4', 0, n))) == 4
    bits = D.score_layout('low_byte', 0, n).view(np.uint32)
    assert len(np.unique(bits >> 8)) == 1 and len(np.unique(bits & 255)) == 256
    z = D.score_layout('zero_one', 0, n)
    assert (z == 0).sum() > 1000 and (z == 1).sum() > 1000 and ((z > 0) & (z < 1)).sum() > 1000
    d = D.score_layout('denormal', 0, n)
    assert d.max() < np.finfo(np.float32).tiny and (d > 0).sum() > n // 2 and len(np.unique(d)) > 1000
    # a run of equal scores straddles rank 500 and rank 3000 of the four-valued layout
    q = np.sort(D.score_layout('quant4', 0, n))[::-1]
    assert q[499] == q[500] and q[2999] == q[3000]
    for m in (0, 15, 16, 499, 500, 501, 23040):
        assert int(D.keep_mask(m, n, m).sum()) == m


def test_decode_inputs_keep_exactly_the_requested_anchors():
    s = np.stack([D.score_layout('zero_one', b, 525) for b in range(2)])
    k = np.stack([D.keep_mask(b, 525, m) for b, m in enumerate((17, 300))])
    cls, reg, anchors = D.decode_inputs_for(s, k)
    boxes, scores, keep = D.decode_ref(cls, reg, anchors, 15)
    assert np.array_equal(keep.numpy(), k) and np.array_equal(scores.numpy(), s)
    assert len(np.unique(boxes[1].numpy()[k[1]], axis=0)) == 7


def test_border_deltas_cross_clip_and_hit_the_size_rule():
    anchor = torch.tensor([[184., 120., 215., 151.]])
    d, names = D.border_deltas(anchor[0].numpy())
    reg = torch.from_numpy(d).reshape(1, len(d), 4)
    pre = D.preround_f64(reg, anchor.expand(len(d), 4))[0]
    assert float((pre - pre.floor() - 0.5).abs().min()) > 0.2              # no corner of these is a rounding tie
    boxes, _, keep = D.decode_ref(torch.zeros(1, len(d), 2), reg, anchor.expand(len(d), 4), 1)
    b = dict(zip(names, boxes[0].tolist()))
    k = dict(zip(names, keep[0].tolist()))
    assert b['cross_left'][0] == 0 and b['cross_top'][1] == 0 and b['cross_right'][2] == 1023 and b['cross_bottom'][3] == 374
    assert b['out_left'][0] == b['out_left'][2] == 0 and b['out_right'][0] == b['out_right'][2] == 1023
    assert b['out_top'][1] == b['out_top'][3] == 0 and b['out_bottom'][1] == b['out_bottom'][3] == 374
    assert not (k['out_left'] or k['out_right'] or k['out_top'] or k['out_bottom'])
    for axis, (lo, hi) in (('w', (0, 2)), ('h', (1, 3))):
        for suffix in ('', '_clipped'):
            assert b[f'{axis}_eq_t{suffix}'][hi] - b[f'{axis}_eq_t{suffix}'][lo] + 1 == 5 and k[f'{axis}_eq_t{suffix}']
            assert b[f'{axis}_eq_t_minus_1{suffix}'][hi] - b[f'{axis}_eq_t_minus_1{suffix}'][lo] + 1 == 4
            assert not k[f'{axis}_eq_t_minus_1{suffix}']


def test_level_boundary_sizes_and_the_oracle_level():
    sizes = D.level_boundary_sizes(1024, 375)
    assert len(sizes) == 75
    want = [int(np.rint(np.log2(np.sqrt(float(w) * h) / 10.0))) for w, h in sizes]
    assert [want.count(l) for l in range(-1, 6)] == [3, 9, 14, 17, 16, 11, 5]
    assert (20, 20) in sizes and (16, 25) in sizes and (80, 80) in sizes and (160, 160) in sizes
    rois = torch.tensor([[0., 0., w, h] for w, h in sizes])[None]
    cfg = O.make_cfg()
    lvl = O.roi_geometry(cfg, rois, [h for h, _ in D.FMAP_HW], [w for _, w in D.FMAP_HW])[0][0]
    assert lvl.tolist() == [min(max(l, 0), cfg.n_layers - 1) for l in want]
    # the unclamped fp32 expression of the oracle gives exactly the integer
    size = ((rois[..., 2] - rois[..., 0]) * (rois[..., 3] - rois[..., 1])) ** 0.5
    lf = torch.log(size * 0.1) / np.log(2)
    assert lf[0].tolist() == [float(l) for l in want]
    br = D.boundary_rois()
    assert br.shape == (3, 225, 4)
    assert bool((br[..., 0] >= 0).all() and (br[..., 1] >= 0).all() and (br[..., 2] <= 1023).all() and (br[..., 3] <= 374).all())
    assert bool((br[..., 2] >= br[..., 0]).all() and (br[..., 3] >= br[..., 1]).all())
    assert bool((br[2, :, 2] == 1023).all() and (br[2, :, 3] == 374).all() and (br[0, :, :2] == 0).all())
    # the placements do not change the size, so the three images agree on every level
    l3 = O.roi_geometry(cfg, br, [h for h, _ in D.FMAP_HW], [w for _, w in D.FMAP_HW])[0]
    assert torch.equal(l3[0], l3[1]) and torch.equal(l3[0], l3[2]) and sorted(set(l3.flatten().tolist())) == [0, 1, 2, 3, 4]


def test_edge_rois_hold_the_ties_borders_and_degenerate_boxes():
    rois = D.edge_rois()
    assert rois.shape[0] == 1
    r = rois[0]
    assert bool((r[:, 0] >= 0).all() and (r[:, 1] >= 0).all() and (r[:, 2] <= 1023).all() and (r[:, 3] <= 374).all())
    assert bool((r[:, 2] >= r[:, 0]).all() and (r[:, 3] >= r[:, 1]).all())
    cfg = O.make_cfg()
    lvl = O.roi_geometry(cfg, rois, [h for h, _ in D.FMAP_HW], [w for _, w in D.FMAP_HW])[0][0]
    q = r / (2.0 ** (lvl + 1).float())[:, None]
    ties = (q - q.floor() == 0.5)
    assert int(ties.all(1).sum()) >= 15                                    # RoIs with all four quotients on x.5
    assert set(lvl[ties.all(1)].tolist()) == {0, 1, 2, 3, 4}
    assert int((r[:, 2] == 1023).sum()) >= 10 and int((r[:, 3] == 374).sum()) >= 10
    area = (r[:, 2] - r[:, 0]) * (r[:, 3] - r[:, 1])
    assert int((area == 0).sum()) >= 12 and int((area == 1).sum()) == 4


def test_nms_layouts_meet_their_conditions():
    for n in (129, 500, 4096):
        b = torch.from_numpy(D.nms_chain64(n))
        keep = O.greedy_nms_keep(b, 0.7)
        assert keep == [i for i in range(n) if (i // 64) % 2 == 0]         # a removed box does not remove
        iou = O.pair_iou(b, b)
        hit = (iou >= 0.7).nonzero().tolist()
        assert all(abs(i - j) in (0, 64) for i, j in hit)                  # every suppression crosses a word boundary
        assert len(hit) == n + 2 * (n - 64)
        assert O.greedy_nms_keep(torch.from_numpy(D.nms_identical(n)), 0.7) == [0]
        assert O.greedy_nms_keep(torch.from_numpy(D.nms_disjoint(n)), 0.7) == list(range(n))
    for thresh, a, b in D.THRESHOLD_PAIRS:
        pair = torch.tensor([a, b])
        iou = O.pair_iou(pair, pair)[0, 1]
        assert float(iou) == float(np.float32(thresh))                     # exactly the fp32 threshold
        assert bool(iou >= thresh) and O.greedy_nms_keep(pair, thresh) == [0]
        assert O.greedy_nms_keep(pair, float(np.nextafter(np.float32(thresh), np.float32(1)))) == [0, 1]
    boxes = torch.zeros(3, 64, 4)
    boxes[0, :5] = torch.from_numpy(D.nms_disjoint(5))
    boxes[1, :9] = torch.from_numpy(D.nms_identical(9))
    boxes[2, :7] = torch.from_numpy(D.nms_disjoint(7))
    rois, keeps, n_out = D.nms_ref(boxes, [5, 9, 7], 0.7, 4, [1, 2])
    assert n_out.tolist() == [4, 1, 1] and keeps == [[0, 1, 2, 3], [0], [0]] and not rois[1, 1:].any()


def test_integer_maps_make_the_oracle_pool_one_rounded_division():
    fm = D.integer_fmaps(3, 8)
    assert all(float(f.max()) < 2600 and torch.equal(f, f.round()) for f in fm)
    cfg = O.make_cfg()
    br = D.boundary_rois()
    rois = torch.cat([br[:, ::9], D.edge_rois().expand(3, -1, -1)], 1)
    pool, _, _ = O.roi_pooling(cfg, rois, fm)
    assert torch.equal(pool, D.pool_f64(rois, fm))
    # the largest window still sums exactly in fp32, and the bins hold different integers (a shifted window would show)
    _, x1, y1, x2, y2 = O.roi_geometry(cfg, rois, [h for h, _ in D.FMAP_HW], [w for _, w in D.FMAP_HW])
    assert 2600 * int(((x2 - x1 + 1) * (y2 - y1 + 1)).max()) < 2 ** 24
    assert bool((pool[..., 0, 0] < pool[..., 1, 0]).all() and (pool[..., 0, 0] <= pool[..., 0, 1]).all())   # (== : one-column window at x = W - 1)
    assert torch.equal(pool, pool.round())


def test_tiles_ref_counts_a_hand_made_case():
    rois = torch.tensor([[[0., 0., 12., 12.], [100., 100., 112., 112.]]])
    s = D.tiles_ref(rois, [2], 0, 0)
    TW = 256
    # 12 / 2 = 6 -> window 0..6 and 50..56: tiles 0..3 and 25..28 in both directions
    assert s == {ty * TW + tx for ty in range(4) for tx in range(4)} | {ty * TW + tx for ty in range(25, 29) for tx in range(25, 29)}
    assert len(D.tiles_ref(rois, [1], 0, 0)) == 16 and len(D.tiles_ref(rois, [2], 1, 0)) == 0
    assert len(D.tiles_ref(rois, [1], 0, 1)) == 16 and len(D.tiles_ref(rois, [1], 0, 2)) == 25
    skip = np.zeros(94 * 256, bool)
    skip[0] = True
    assert len(D.tiles_ref(rois, [1], 0, 0, skip)) == 15


def test_post_inputs_give_50_and_30_rows():
    rois, reg, cls, scores = D.post_disjoint_200()
    assert bool((scores[:-1] > scores[1:]).all())
    rows = D.post_ref(rois, [200], reg, cls, 0.3, 0.05)[0]
    assert rows.shape == (50, 6) and torch.equal(rows[:, 5], scores[:50]) and bool((rows[:, 0] == 7).all())
    ms = 0.5 * (float(scores[29]) + float(scores[30]))
    rows = D.post_ref(rois, [200], reg, cls, 0.3, ms)[0]
    assert rows.shape == (30, 6) and torch.equal(rows[:, 5], scores[:30])
    # a score exactly equal to min_score is dropped (strict >)
    rows = D.post_ref(rois, [200], reg, cls, 0.3, float(scores[29]))[0]
    assert rows.shape == (29, 6)
    # background tied with a class for the maximum: background wins, the RoI is dropped
    cls2 = cls.clone()
    cls2[0, 3, 0] = cls2[0, 3, 7]
    rows = D.post_ref(rois, [200], reg, cls2, 0.3, 0.05)[0]
    assert rows.shape == (50, 6) and float(scores[3]) not in rows[:, 5].tolist() and float(scores[50]) in rows[:, 5].tolist()
    r, g, c = D.post_random(0, 2, 64)
    assert sum(len(x) for x in D.post_ref(r, [64, 3], g, c, 0.3, 0.05)) > 0
