"""CPU references and input builders for the edge tests of the proposal / RoI / detection kernels (csrc/detect.hip):
tests/test_detect_ref_cpu.py checks them against `oracle.nets_ref`, tests/test_gpu_detect_edges.py feeds them to the kernels.

Everything is seeded through `birdsoundclassif_amd.synth`; nothing here touches the GPU."""
import numpy as np
import torch

from birdsoundclassif_amd import synth
from oracle import nets_ref as O

IMG_W, IMG_H = 1024, 375
FMAP_HW = [(188, 512), (94, 256), (47, 128), (24, 64), (12, 32)]


def rnd(key, *shape, scale=1.0):
    return torch.from_numpy((synth.normal(key, int(np.prod(shape))) * scale).astype(np.float32).reshape(shape))


def rpn_inputs(B, seed):
    """The seeded RPN outputs of tests/test_gpu_ops.py (`_rpn_inputs`): softmaxed class pairs and deltas on the 24 x 64 map."""
    cfg = O.make_cfg()
    cls_raw = rnd(('pc', seed), B, 30, 24, 64, scale=1.5)
    cls = cls_raw.view(B, 15, 2, 24, 64).softmax(2).view(B, 30, 24, 64)
    reg = rnd(('pr', seed), B, 60, 24, 64, scale=0.25)
    return cfg, cls, reg


# ----------------------------------------------------------------------------------------------- top-N selection
def select_ref(scores, keep, top_n, fail_below, segments):
    """Selection of ProposalLayer.forward (reference layers.py:284-293): per image the kept anchors in stable descending score
    order (ties by ascending anchor index), cut to N = min(top_n, min over the image's segment of the kept counts), N = 0 for
    the whole segment when N < fail_below ("RPN failed").  scores [B, KA] float32, keep [B, KA] bool, segments: sizes of the
    contiguous segments.  -> (list of B index arrays, n_sel int [B])."""
    scores = np.asarray(scores, dtype=np.float32)
    keep = np.asarray(keep, dtype=bool)
    B = scores.shape[0]
    assert sum(segments) == B
    counts = keep.sum(1)
    n_sel = np.zeros(B, dtype=np.int64)
    b = 0
    for size in segments:
        n = min(int(top_n), int(counts[b:b + size].min()))
        n_sel[b:b + size] = 0 if n < fail_below else n
        b += size
    idx = []
    for b in range(B):
        order = np.argsort(-scores[b], kind='stable')
        idx.append(order[keep[b][order]][:n_sel[b]])
    return idx, n_sel


SCORE_LAYOUTS = ('distinct', 'quant4', 'low_byte', 'zero_one', 'denormal')


def score_layout(name, key, n):
    """n float32 scores >= 0: 'distinct' (all different), 'quant4' (four values: the index tie-break decides and a run of
    equal scores straddles any rank), 'low_byte' (equal in the upper three bytes of the bit pattern), 'zero_one' (exactly 0.0
    and 1.0 mixed with others), 'denormal' (fp32 denormals and 0)."""
    u = synth.uniform(('score', name, key), n)
    if name == 'distinct':
        rank = np.argsort(np.argsort(u, kind='stable'), kind='stable')
        s = ((rank + 1.0) / (n + 1.0)).astype(np.float32)
        assert len(np.unique(s)) == n
        return s
    if name == 'quant4':
        return (np.floor(u * 4) / 4 + 0.125).astype(np.float32)
    if name == 'low_byte':
        return (np.uint32(0x3F000000) + np.floor(u * 256).astype(np.uint32)).view(np.float32)
    if name == 'zero_one':
        return np.where(u < 0.3, 0.0, np.where(u < 0.6, 1.0, u)).astype(np.float32)
    if name == 'denormal':
        return np.floor(u * 2000).astype(np.uint32).view(np.float32)
    raise KeyError(name)


def keep_mask(key, n, m):
    """Boolean [n] with exactly m True at seeded positions."""
    order = np.argsort(synth.uniform(('keep', key), n), kind='stable')
    k = np.zeros(n, dtype=bool)
    k[order[:max(0, min(m, n))]] = True
    return k


SEL_ANCHOR = (96.0, 96.0, 127.0, 127.0)


def decode_inputs_for(scores, keep, n_anchor=15):
    """(cls [B, K, 2A], reg [B, K, 4A], anchors [KA, 4]) that make nbm_rpn_decode emit `scores` as the objectness and keep
    exactly the anchors of `keep`: kept anchors get zero deltas on a 32 x 32 anchor, dropped ones a width delta of -20 (the box
    collapses to one pixel, below min_threshold)."""
    scores = np.asarray(scores, dtype=np.float32)
    B, KA = scores.shape
    assert KA % n_anchor == 0
    K = KA // n_anchor
    cls = np.zeros((B, K, n_anchor, 2), np.float32)
    cls[..., 1] = scores.reshape(B, K, n_anchor)
    cls[..., 0] = 0.25
    reg = np.zeros((B, K, n_anchor, 4), np.float32)
    reg[..., 2] = np.where(np.asarray(keep).reshape(B, K, n_anchor), 0.0, -20.0)
    anchors = np.tile(np.array(SEL_ANCHOR, np.float32), (KA, 1))
    anchors[:, 0] += np.arange(KA) % 7                    # boxes differ, so a wrong index shows in the box too
    anchors[:, 2] += np.arange(KA) % 7
    return (torch.from_numpy(cls.reshape(B, K, 2 * n_anchor)), torch.from_numpy(reg.reshape(B, K, 4 * n_anchor)),
            torch.from_numpy(anchors))


# ----------------------------------------------------------------------------------------------- RPN decode
def decode_ref(cls, reg, anchors, n_anchor, min_threshold=5, img_w=IMG_W, img_h=IMG_H):
    """decode_boxes + clip + the min_threshold rule (reference layers.py:258-283) on K-major / anchor-minor inputs:
    cls [B, K, 2A], reg [B, K, 4A], anchors [KA, 4] -> boxes [B, KA, 4], scores [B, KA], keep bool [B, KA]."""
    B = cls.shape[0]
    scores = cls.reshape(B, -1, 2)[..., 1]
    boxes = O.decode_boxes(reg.reshape(B, -1, 4), anchors)
    boxes = torch.stack([boxes[..., 0].clamp(0, img_w - 1), boxes[..., 1].clamp(0, img_h - 1),
                         boxes[..., 2].clamp(0, img_w - 1), boxes[..., 3].clamp(0, img_h - 1)], -1)
    keep = ((boxes[..., 2] - boxes[..., 0] + 1 >= min_threshold) & (boxes[..., 3] - boxes[..., 1] + 1 >= min_threshold))
    return boxes, scores, keep


def preround_f64(reg, anchors):
    """Box corners before the rounding, float64, from the same (fp32) deltas: [B, KA, 4]."""
    d = reg.reshape(reg.shape[0], -1, 4).double()
    a = anchors.double()
    wa, ha = a[:, 2] - a[:, 0] + 1, a[:, 3] - a[:, 1] + 1
    xa, ya = a[:, 0] + 0.5 * wa, a[:, 1] + 0.5 * ha
    x, y = d[..., 0] * wa + xa, d[..., 1] * ha + ya
    w, h = torch.exp(d[..., 2]) * wa, torch.exp(d[..., 3]) * ha
    return torch.stack([x - 0.5 * w, y - 0.5 * h, x + 0.5 * w, y + 0.5 * h], -1)


def border_deltas(anchors, min_threshold=5, img_w=IMG_W, img_h=IMG_H):
    """One row of deltas per case, all against anchor 0 of `anchors` (anchor [4] -> deltas [n, 4] float32, names): boxes that
    cross each of the four borders, lie wholly outside on each side, and have a clipped width / height of exactly
    min_threshold and min_threshold - 1."""
    a = np.asarray(anchors, dtype=np.float64)
    wa, ha = a[2] - a[0] + 1, a[3] - a[1] + 1
    xa, ya = a[0] + 0.5 * wa, a[1] + 0.5 * ha

    def to(x1, y1, x2, y2):
        # deltas whose decoded (pre-round) corners are x1 .. x2 + 0, i.e. centre / size of the requested corners
        w, h = x2 - x1, y2 - y1
        return [((x1 + x2) / 2 - xa) / wa, ((y1 + y2) / 2 - ya) / ha, np.log(w / wa), np.log(h / ha)]

    t = min_threshold
    cases = {
        'cross_left': to(-30.25, 100.25, 40.25, 160.25), 'cross_top': to(300.25, -20.25, 380.25, 50.25),
        'cross_right': to(990.25, 100.25, 1060.25, 160.25), 'cross_bottom': to(300.25, 340.25, 380.25, 400.25),
        'out_left': to(-90.25, 100.25, -20.25, 160.25), 'out_top': to(300.25, -90.25, 380.25, -20.25),
        'out_right': to(1040.25, 100.25, 1100.25, 160.25), 'out_bottom': to(300.25, 400.25, 380.25, 460.25),
        # clipped sizes: x2 - x1 + 1 == t (kept) and t - 1 (dropped), inside and against a border
        'w_eq_t': to(200.25, 100.25, 200.25 + t - 1, 160.25), 'w_eq_t_minus_1': to(200.25, 100.25, 200.25 + t - 2, 160.25),
        'h_eq_t': to(200.25, 100.25, 260.25, 100.25 + t - 1), 'h_eq_t_minus_1': to(200.25, 100.25, 260.25, 100.25 + t - 2),
        'w_eq_t_clipped': to(-40.25, 100.25, t - 1 + 0.25, 160.25), 'w_eq_t_minus_1_clipped': to(-40.25, 100.25, t - 2 + 0.25, 160.25),
        'h_eq_t_clipped': to(300.25, 374 - (t - 1) - 0.25, 380.25, 420.25),
        'h_eq_t_minus_1_clipped': to(300.25, 374 - (t - 2) - 0.25, 380.25, 420.25),
    }
    return np.array(list(cases.values()), dtype=np.float32), list(cases)


# ----------------------------------------------------------------------------------------------- NMS
def nms_identical(n):
    return np.tile(np.array([10., 10., 50., 50.], np.float32), (n, 1))


def nms_disjoint(n):
    x = 20.0 * np.arange(n, dtype=np.float32)
    return np.stack([x, np.zeros_like(x), x + 9, np.full_like(x, 9)], 1)


def nms_chain64(n):
    """Box i overlaps only box i + 64 (and i - 64) at threshold 0.7: 64 lanes far apart in x, box i is step i // 64 of lane
    i % 64, consecutive steps are 10 rows apart (IoU 90 / 110 = 0.82), steps two apart have IoU 80 / 120 = 0.67.  So every
    suppression crosses a 64-bit word boundary, and a removed box must not remove: the even steps survive."""
    i = np.arange(n)
    x = 1000.0 * (i % 64)
    y = 10.0 * (i // 64)
    return np.stack([x, y, x + 99, y + 99], 1).astype(np.float32)


# (threshold, box a, box b): integer boxes whose IoU is exactly the threshold -- intersection 1 of union 2, 7 of 10
THRESHOLD_PAIRS = ((0.5, (0., 0., 0., 0.), (0., 0., 1., 0.)),
                   (0.7, (0., 0., 6., 0.), (0., 0., 9., 0.)))


def nms_ref(boxes, n_in, thresh, post_n, segments):
    """boxes [B, cap, 4] torch, n_in list -> (rois [B, post_n, 4], index lists, n_out [B]); rows beyond n_out zero."""
    B = boxes.shape[0]
    keeps = [O.greedy_nms_keep(boxes[b, :n_in[b]], thresh) for b in range(B)]
    n_out = np.zeros(B, dtype=np.int64)
    b = 0
    for size in segments:
        n_out[b:b + size] = min(post_n, min(len(k) for k in keeps[b:b + size]))
        b += size
    rois = torch.zeros((B, post_n, 4))
    for b in range(B):
        k = keeps[b][:n_out[b]]
        rois[b, :len(k)] = boxes[b, k]
        keeps[b] = k
    return rois, keeps, n_out


# ----------------------------------------------------------------------------------------------- RoI pooling
def level_boundary_sizes(max_w, max_h):
    """The (w, h) pairs, 1 <= w < max_w, 1 <= h < max_h, whose float64 log2(sqrt(w h) / 10) is within 1e-6 of an integer:
    RoI sizes (x2 - x1, y2 - y1) that sit exactly on a pyramid-level boundary (reference layers.py:408-417)."""
    w = np.arange(1, max_w, dtype=np.float64)[:, None]
    h = np.arange(1, max_h, dtype=np.float64)[None, :]
    lf = np.log2(np.sqrt(w * h) / 10.0)
    hit = np.argwhere(np.abs(lf - np.rint(lf)) < 1e-6)
    return [(int(a) + 1, int(b) + 1) for a, b in hit]


def boundary_rois(img_w=IMG_W, img_h=IMG_H):
    """Every level-boundary size, and each with width + 1 and width - 1, at the origin, in the middle and against the right /
    bottom border (where it fits): float32 [3, n, 4], one image per placement."""
    rows = [[], [], []]
    for (w, h) in level_boundary_sizes(img_w, img_h):
        for ww in (w, w + 1, w - 1):
            if ww < 0 or ww > img_w - 1:
                ww = w
            x_mid, y_mid = (img_w - 1 - ww) // 2, (img_h - 1 - h) // 2
            rows[0].append([0, 0, ww, h])
            rows[1].append([x_mid, y_mid, x_mid + ww, y_mid + h])
            rows[2].append([img_w - 1 - ww, img_h - 1 - h, img_w - 1, img_h - 1])
    return torch.tensor(rows, dtype=torch.float32)


def edge_rois(img_w=IMG_W, img_h=IMG_H):
    """float32 [1, n, 4]: coordinates whose quotient by the level's stride is exactly x.5 (ties to even), RoIs touching
    x = img_w - 1 and y = img_h - 1, zero-area and one-pixel RoIs at all four corners."""
    X, Y = img_w - 1, img_h - 1
    rows = []
    for lvl, side in enumerate((12, 30, 60, 120, 250)):           # sqrt(w h) / 10 in [2^lvl, 2^(lvl+1))
        s = 2 << lvl
        m = max(1, int(round(side / s)))
        for k in (0, 1, 2, 3):
            x1, y1 = s * k + s // 2, s * (k + 1) + s // 2         # quotients k + 0.5, k + 1.5: even and odd neighbours
            x2, y2 = x1 + s * m, y1 + s * m                        # (k + m).5 as well
            if x2 <= X and y2 <= Y:
                rows.append([x1, y1, x2, y2])
        rows.append([X - side, Y - min(side, Y), X, Y])            # touches the right and the bottom border
        rows.append([X - side, 0, X, min(side, Y)])
    for (cx, cy) in ((0, 0), (X, 0), (0, Y), (X, Y)):
        rows.append([cx, cy, cx, cy])                              # zero area: size 0 -> log(0)
        rows.append([min(cx, X - 1), min(cy, Y - 1), min(cx, X - 1) + 1, min(cy, Y - 1) + 1])   # one pixel
        rows.append([cx, min(cy, Y - 9), cx, min(cy, Y - 9) + 9])  # zero width
        rows.append([min(cx, X - 9), cy, min(cx, X - 9) + 9, cy])  # zero height
    rows.append([0, 0, X, Y])
    return torch.tensor([rows], dtype=torch.float32)


def integer_fmaps(B, C, fmap_hw=FMAP_HW):
    """NCHW maps of small integers, linear in the position with even slopes: 2 y + 4 x + 3 c + 7 b + 11 level.  The mean of
    any rectangular bin is then an integer and every partial sum stays far below 2^24, so the fp32 bin sum is exact in any
    order and dividing it by the bin's area -- at once, or by its height and then its width as torch's adaptive pooling
    does -- gives the same bits; a window that is off by one row or column moves the mean by at least 1."""
    out = []
    for l, (H, W) in enumerate(fmap_hw):
        y = torch.arange(H).view(1, 1, H, 1)
        x = torch.arange(W).view(1, 1, 1, W)
        c = torch.arange(C).view(1, C, 1, 1)
        b = torch.arange(B).view(B, 1, 1, 1)
        out.append((2 * y + 4 * x + 3 * c + 7 * b + 11 * l).float())
    return out


def modular_fmaps(B, C, fmap_hw=FMAP_HW):
    """NCHW maps of the pseudo-random small integers (y * W + x + 3 c + 7 b + 11 level) % 251: bin sums are exact in fp32, the
    mean is not an integer, so it compares to an ulp only (torch divides by the height, then by the width)."""
    out = []
    for l, (H, W) in enumerate(fmap_hw):
        y = torch.arange(H).view(1, 1, H, 1)
        x = torch.arange(W).view(1, 1, 1, W)
        c = torch.arange(C).view(1, C, 1, 1)
        b = torch.arange(B).view(B, 1, 1, 1)
        out.append(((y * W + x + 3 * c + 7 * b + 11 * l) % 251).float())
    return out


def pool_f64(rois, fmaps):
    """Bin means of the RoI windows in float64, rounded once to fp32: [B, R, C, 2, 2] (geometry from O.roi_geometry)."""
    cfg = O.make_cfg()
    B, R = rois.shape[:2]
    lvl, x1, y1, x2, y2 = O.roi_geometry(cfg, rois, [f.shape[-2] for f in fmaps], [f.shape[-1] for f in fmaps])
    out = torch.zeros(B, R, fmaps[0].shape[1], 2, 2)
    for b in range(B):
        for r in range(R):
            f = fmaps[int(lvl[b, r])][b, :, int(y1[b, r]):int(y2[b, r]) + 1, int(x1[b, r]):int(x2[b, r]) + 1].double()
            h, w = f.shape[-2:]
            for i in range(2):
                for j in range(2):
                    ya, yb = (i * h) // 2, -((-(i + 1) * h) // 2)
                    xa, xb = (j * w) // 2, -((-(j + 1) * w) // 2)
                    out[b, r, :, i, j] = f[:, ya:yb, xa:xb].mean((1, 2)).float()
    return out


def tiles_ref(rois, n_roi, level, dilate, skip=None, fmap_hw=FMAP_HW):
    """The set of 2 x 2 output tiles of pyramid level `level` under the RoI windows (grown by `dilate` pixels, minus the tiles
    of `skip` [TH * TW] bool), as entries b * TH * TW + ty * TW + tx."""
    cfg = O.make_cfg()
    lvl, x1, y1, x2, y2 = O.roi_geometry(cfg, rois, [h for h, _ in fmap_hw], [w for _, w in fmap_hw])
    H, W = fmap_hw[level]
    TH, TW = (H + 1) // 2, (W + 1) // 2
    out = set()
    for b in range(rois.shape[0]):
        for r in range(int(n_roi[b])):
            if int(lvl[b, r]) != level:
                continue
            ty0, ty1 = max(int(y1[b, r]) - dilate, 0) // 2, min(int(y2[b, r]) + dilate, H - 1) // 2
            tx0, tx1 = max(int(x1[b, r]) - dilate, 0) // 2, min(min(int(x2[b, r]), W - 1) + dilate, W - 1) // 2
            for ty in range(ty0, ty1 + 1):
                for tx in range(tx0, tx1 + 1):
                    if skip is None or not skip[ty * TW + tx]:
                        out.add(b * TH * TW + ty * TW + tx)
    return out


# ----------------------------------------------------------------------------------------------- FastRCNN post-processing
NC = 150


def post_rows(res):
    """fast_rcnn_post's dictionaries of ONE image -> float32 [n, 6] rows {class, x1, y1, x2, y2, score}, (class asc, score desc)."""
    rows = []
    for c in range(1, NC + 1):
        v = res[str(c)]
        bb = v['bbox_coord']
        if len(bb) == 0:
            continue
        sc = v['scores'].reshape(-1)
        for i in range(len(bb)):
            rows.append([float(c), *bb[i].tolist(), float(sc[i])])
    return torch.tensor(rows, dtype=torch.float32).reshape(-1, 6)


def post_ref(rois, n_roi, reg, cls, nms_thresh, min_score, proposal_number=50):
    """O.fast_rcnn_post per image on its first n_roi[b] RoIs: rois [B, cap, 4], reg [B, cap, 4 (NC + 1)], cls [B, cap, NC + 1]
    -> list of B row tensors [n_det, 6]."""
    cfg = O.make_cfg(proposal_number=proposal_number)
    out = []
    for b in range(rois.shape[0]):
        n = int(n_roi[b])
        if n == 0:
            out.append(torch.zeros((0, 6)))
            continue
        res = O.fast_rcnn_post(cfg, rois[b:b + 1, :n], reg[b, :n], cls[b, :n], nms_thresh, min_score)
        out.append(post_rows(res[0]))
    return out


def post_random(key, B, cap):
    """Random head outputs on random RoIs: (rois [B, cap, 4], reg, cls softmaxed with a background bias)."""
    u = synth.uniform(('post_rois', key), B * cap * 4).reshape(B, cap, 4)
    x1, y1 = np.floor(u[..., 0] * 1000), np.floor(u[..., 1] * 360)
    w, h = np.floor(2 + u[..., 2] ** 3 * 1000), np.floor(2 + u[..., 3] ** 3 * 370)
    rois = torch.tensor(np.stack([x1, y1, np.minimum(x1 + w, IMG_W - 1), np.minimum(y1 + h, IMG_H - 1)], -1), dtype=torch.float32)
    reg = rnd(('post_reg', key), B, cap, 4 * (NC + 1), scale=0.3)
    logits = rnd(('post_cls', key), B, cap, NC + 1, scale=3.0)
    logits[..., 0] += 2.0
    return rois, reg, logits.softmax(-1)


def post_disjoint_200(cls_id=7):
    """200 disjoint RoIs of one class with strictly descending scores and zero deltas (a 20 x 10 grid of 30 x 20 boxes in
    40 x 30 cells: the decoded boxes, one pixel larger, stay disjoint): rois [1, 200, 4], reg, cls, scores [200]."""
    i = np.arange(200)
    x1, y1 = 40.0 * (i % 20) + 5, 30.0 * (i // 20) + 5
    rois = torch.tensor(np.stack([x1, y1, x1 + 29, y1 + 19], -1), dtype=torch.float32)[None]
    scores = torch.from_numpy((0.99 - 0.0015 * i).astype(np.float32))
    cls = torch.zeros(1, 200, NC + 1)
    cls[0, :, cls_id] = scores
    cls[0, :, 0] = 0.005
    return rois, torch.zeros(1, 200, 4 * (NC + 1)), cls, scores
