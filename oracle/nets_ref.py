"""TEST INFRASTRUCTURE ONLY — CPU restatement (pure torch, fp32) of the NBM detector.

This is the *oracle* for the detector half of the hot path (SURVEY.md §8a rows
M1..M10, P1..P5, L1..L5).  It is a functional re-expression of the reference's
algorithm -- every function cites the reference file:line it follows -- written
batched and loop-free where the reference loops in Python.  It is pinned by
the golden fixtures in `tests/golden/` that `oracle/make_golden.py` generates
from the real reference (imported with `oracle/tv_standin.py`), among them
`reference_checks.npz` for `tests/test_oracle_vs_reference.py`.  Only tests,
`__graft_entry__.smoke()` and `bench.py`'s `cpu_baseline` leg may import it;
the product path never does.

All tensors are NCHW like the reference.  Weights come in as a plain
`state_dict` (SURVEY.md Appendix B names).
"""
import math
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F


# --------------------------------------------------------------------------- config
def make_cfg(args=None, **kw):
    """Subset of the reference `args` namespace that shapes the model (train.py:21-168,
    nets_utils.py:405-416 `setattr_others`)."""
    d = dict(img_width=1024, img_height=375, inpt_channels=1, n_ratios=3, anchor_stride=16, base_size=16,
             fpn_p_chan=384, out_fpn_chan=256, pyramid_top_n_attn=2, num_classes=150,
             roi_pool_h=2, roi_pool_w=2, depth_rcnn=3,
             pre_nms_topN=3000, pre_nms_topN_eval=500, post_nms_topN=1000, post_nms_topN_eval=50,
             min_threshold=5, nms_thresh=0.7, proposal_number=50,
             rpn_neg_label=0.3, rpn_pos_label=0.7, rpn_batchsize=16, rpn_fg_fraction=0.5,
             rcnn_batch_size=16, rcnn_fg_prop=0.4, fg_threshold=0.5, bg_threshold_lo=0.1, bg_threshold_hi=0.5,
             focal_loss=False, clip_max_norm=0.1, lr=1e-4, lr_backbone=1e-5, weight_decay=1e-4,
             top_size=(24, 64), n_layers=5,
             add_posenc=False, one_dim_posenc=True, fpn_first=False, sandwich_attn=False, fpn='fpn', n_bifpn_layers=5, dilation=False,
             tf_rcnn=False, tf_pe_qk=False, tf_model_dim=512, tf_nhead=8, tf_num_encoder_layers=6, tf_dim_feedforward=1024)
    if args is not None:
        for k in list(d):
            if hasattr(args, k):
                d[k] = getattr(args, k)
    d.update(kw)
    d['ratios'] = {3: [0.5, 1, 2], 5: [0.2, 0.5, 1, 2, 5]}[d['n_ratios']]
    d['top_size'] = tuple(d['top_size'])
    return SimpleNamespace(**d)


# --------------------------------------------------------------------------- backbone (M1, M2)
def _fbn(x, sd, p):
    """FrozenBatchNorm2d.forward, backbone.py:52-62 (eps=1e-5, scale computed first)."""
    scale = sd[p + '.weight'] * (sd[p + '.running_var'] + 1e-5).rsqrt()
    bias = sd[p + '.bias'] - sd[p + '.running_mean'] * scale
    return x * scale.reshape(1, -1, 1, 1) + bias.reshape(1, -1, 1, 1)


def _bottleneck(x, sd, p, stride, dilation=1):
    """torchvision ResNet-50 v1.5 bottleneck (stride on conv2), as instantiated at backbone.py:131."""
    out = F.relu(_fbn(F.conv2d(x, sd[p + '.conv1.weight']), sd, p + '.bn1'))
    out = F.relu(_fbn(F.conv2d(out, sd[p + '.conv2.weight'], stride=stride, padding=dilation, dilation=dilation), sd, p + '.bn2'))
    out = _fbn(F.conv2d(out, sd[p + '.conv3.weight']), sd, p + '.bn3')
    if (p + '.downsample.0.weight') in sd:
        x = _fbn(F.conv2d(x, sd[p + '.downsample.0.weight'], stride=stride), sd, p + '.downsample.1')
    return F.relu(out + x)


def backbone_forward(sd, x, dilation=False):
    """BackboneBase.forward backbone.py:110-113 + IntermediateLayerGetter taps relu,layer1..4 (:82-85).
    x [B,1,H,W] -> list of 5 maps (strides 2..32).  The sine position encodings computed by
    Joiner (:139-148) are discarded by the default config (nbm_model.py:45) and not restated.
    `dilation` (backbone.py:129-131, torchvision `replace_stride_with_dilation=[False, False, True]`): layer4 at stride 1, its first
    block with the previous dilation (1), the others with dilation 2."""
    pre = 'backbone.0.'
    if (pre + 'init_conv.weight') in sd:
        x = F.conv2d(x, sd[pre + 'init_conv.weight'], sd[pre + 'init_conv.bias'])
    b = pre + 'body.'
    x = F.relu(_fbn(F.conv2d(x, sd[b + 'conv1.weight'], stride=2, padding=3), sd, b + 'bn1'))
    taps = [x]
    x = F.max_pool2d(x, 3, stride=2, padding=1)
    for li, (nblk, stride) in enumerate(((3, 1), (4, 2), (6, 2), (3, 2)), start=1):
        dil = bool(dilation) and li == 4
        for bi in range(nblk):
            x = _bottleneck(x, sd, f'{b}layer{li}.{bi}', 1 if dil else (stride if bi == 0 else 1), 2 if (dil and bi > 0) else 1)
        taps.append(x)
    return taps


# --------------------------------------------------------------------------- attention (M4)
def self_attention(sd, p, x):
    """SelfAttention.forward self_attention.py:24-56 (downscale_factor=1, no position encoding)."""
    bs, c, h, w = x.shape
    t = x.flatten(2).transpose(1, 2)                                   # [B, L, C]
    q = F.linear(t, sd[p + '.query.weight'], sd[p + '.query.bias'])
    k = F.linear(t, sd[p + '.key.weight'], sd[p + '.key.bias'])
    v = F.linear(t, sd[p + '.value.weight'], sd[p + '.value.bias'])
    denom = float(np.round(np.sqrt(q.size(-1)), 2))                     # self_attention.py:47
    fac = torch.softmax(torch.matmul(q, k.transpose(1, 2)) / denom, dim=-1)
    ctx = torch.matmul(fac, v)
    out = F.linear(ctx, sd[p + '.final_projection.weight'], sd[p + '.final_projection.bias'])
    return out.transpose(1, 2).reshape(bs, c, h, w)


def self_attention_full(sd, p, x, downscale):
    """SelfAttention.forward self_attention.py:24-56 in the `top_n == n_levels` configuration (position_encoding=True,
    downscale_factor = max(1, 2**(3-i))): the input gets + 0.5 * frequency encoding; with a downscale factor the module
    returns the down-and-up interpolated INPUT (the attention it computed is discarded, :52-54)."""
    bs, c, h0, w0 = x.shape
    pe = pe_table(h0, c).transpose(0, 1)[None, ..., None]
    x = x + 0.5 * pe
    if downscale > 1:
        x = F.interpolate(x, size=(h0 // downscale, w0 // downscale), mode='bilinear', align_corners=True)
        return F.interpolate(x, size=(h0, w0), mode='bilinear', align_corners=True)
    return self_attention(sd, p, x)


def sa_pyramid(sd, feats, top_n=2, prefix='attn'):
    """SAPyramid.forward self_attention.py:72-76: `fm + module(fm)` for ALL levels; the lower
    levels hold nn.Identity so they come out doubled."""
    n = len(feats)
    out = []
    if top_n == n:                                  # self_attention.py:63-66
        return [fm + self_attention_full(sd, f'{prefix}.attention_modules.{i}', fm, max(1, 2 ** (3 - i)))
                for i, fm in enumerate(feats)]
    for i, fm in enumerate(feats):
        if i >= n - top_n:
            out.append(fm + self_attention(sd, f'{prefix}.attention_modules.{i}', fm))
        else:
            out.append(fm + fm)
    return out


# --------------------------------------------------------------------------- FPN (M5)
def fpn_forward(sd, feats):
    """FPN.forward fpn.py:132-146.  `pt_wise[i]` is indexed bottom-up, `out_convs[i]` from the TOP
    ('0' = coarsest) -- SURVEY Appendix C-2."""
    n = len(feats)
    lat = [F.conv2d(fm, sd[f'fpn.pt_wise.{i}.weight'], sd[f'fpn.pt_wise.{i}.bias']) for i, fm in enumerate(feats)]
    out = lat[n - 1]
    outs = [F.conv2d(out, sd['fpn.out_convs.0.weight'], sd['fpn.out_convs.0.bias'], padding=1)]
    for j in range(1, n):
        p = lat[n - 1 - j]
        out = F.interpolate(out, size=p.shape[-2:], mode='bilinear', align_corners=True) + p
        outs.insert(0, F.conv2d(out, sd[f'fpn.out_convs.{j}.weight'], sd[f'fpn.out_convs.{j}.bias'], padding=1))
    return outs


# --------------------------------------------------------------------------- RPN (M6)
def bifpn_forward(sd, feats, n_layers, training=False, new_buffers=None):
    """BiFPN.forward fpn.py:9-115 (`--fpn bifpn`): per layer a top-down then a bottom-up pass of weighted fusions
    (ReLU'd learnable weights, `num / (sum + 1e-4)`, then DepthwiseSepConv2d); neighbours are brought to the level's
    size with bilinear align_corners resizing followed by a 1x1 convolution; the last layer ends with 1x1 convolutions to
    out_fpn_chan.  Channels stay the backbone's own per level until then."""
    def rescale(p, x, size):
        out = F.interpolate(x, size=size, mode='bilinear', align_corners=True)
        if (p + '.pt_wise.weight') in sd:
            out = F.conv2d(out, sd[p + '.pt_wise.weight'], sd[p + '.pt_wise.bias'])
        return out

    def fuse(p, inputs):
        w = F.relu(sd[p + '.weights'])
        num = 0
        for wi, xi in zip(w, inputs):
            num = num + wi * xi
        return dw_sep_conv(sd, p + '.conv', num / (w.sum() + 1e-4), 1, training, new_buffers)

    x = list(feats)
    n = len(x)
    for l in range(n_layers):
        p = f'fpn.layers.{l}'
        sizes = [tuple(e.shape[-2:]) for e in x]
        td_out = x[-1]
        td = [td_out]
        for i in range(n - 2, 0, -1):
            td_out = fuse(f'{p}.fusions_td.{i}', [x[i], rescale(f'{p}.rescalings_td.{i + 1}', td_out, sizes[i])])
            td.insert(0, td_out)
        td.insert(0, rescale(f'{p}.rescalings_td.1', td_out, sizes[0]))
        bu_out = fuse(f'{p}.fusions_bu.0', [x[0], td[0]])
        bu = [bu_out]
        for i in range(1, n - 1):
            bu_out = fuse(f'{p}.fusions_bu.{i}', [x[i], td[i], rescale(f'{p}.rescalings_bu.{i - 1}', bu_out, sizes[i])])
            bu.append(bu_out)
        bu.append(fuse(f'{p}.fusions_bu.{n - 1}', [x[-1], rescale(f'{p}.rescalings_bu.{n - 2}', bu_out, sizes[-1])]))
        if (f'{p}.out_pt_wise_convs.0.weight') in sd:
            bu = [F.conv2d(b, sd[f'{p}.out_pt_wise_convs.{i}.weight'], sd[f'{p}.out_pt_wise_convs.{i}.bias']) for i, b in enumerate(bu)]
        x = bu
    return x


def _bn(x, sd, p, training, new_buffers, momentum=0.1, eps=1e-5):
    """nn.BatchNorm2d: batch statistics in training (running stats updated with the unbiased
    variance, momentum 0.1), running statistics in eval.  Updated buffers are returned through
    `new_buffers` instead of being written in place."""
    rm, rv = sd[p + '.running_mean'], sd[p + '.running_var']
    if training:
        rm, rv = rm.clone(), rv.clone()
        y = F.batch_norm(x, rm, rv, sd[p + '.weight'], sd[p + '.bias'], True, momentum, eps)
        if new_buffers is not None:
            new_buffers[p + '.running_mean'], new_buffers[p + '.running_var'] = rm, rv
            if (p + '.num_batches_tracked') in sd:
                new_buffers[p + '.num_batches_tracked'] = sd[p + '.num_batches_tracked'] + 1
        return y
    return F.batch_norm(x, rm, rv, sd[p + '.weight'], sd[p + '.bias'], False, momentum, eps)


def dw_sep_conv(sd, p, x, stride, training, new_buffers, pe=None):
    """DepthwiseSepConv2d.forward layers.py:33-46 (stride<1 => bilinear upsample first :35-37)."""
    if stride < 1:
        size = ((1 / stride) * np.array(x.shape[-2:])).astype(np.int64).tolist()
        x = F.interpolate(x, size=size, mode='bilinear', align_corners=True)
    cin = x.shape[1]
    out = F.conv2d(x, sd[p + '.depth_wise.weight'], sd[p + '.depth_wise.bias'],
                   stride=int(max(1, stride)), padding=1, groups=cin)
    if pe is not None:
        pe = F.conv2d(F.silu(pe), sd[p + '.pe_proj.weight'], sd[p + '.pe_proj.bias'])
        half = pe.shape[1] // 2
        out = out * pe[:, :half] + pe[:, half:]
    out = F.conv2d(out, sd[p + '.pt_wise.weight'], sd[p + '.pt_wise.bias'])
    return F.silu(_bn(out, sd, p + '.norm', training, new_buffers))


def rpn_forward(sd, cfg, fpn_out, training=False, new_buffers=None):
    """RegionProposalNetwork.forward layers.py:79-99.  Returns softmaxed objectness
    [B, 5*A*2, h, w] and regression [B, 5*A*4, h, w] (anchor index = level*A + ratio)."""
    A = cfg.n_ratios
    feats = []
    for i, fm in enumerate(fpn_out):
        y = dw_sep_conv(sd, f'head.rpn.convs.{i}', fm, cfg.anchor_stride / (2 ** (i + 1)), training, new_buffers)
        feats.append(F.adaptive_avg_pool2d(y, cfg.top_size))
    bs, _, h, w = feats[0].shape
    cls = [F.conv2d(f, sd[f'head.rpn.cls_score.{i}.weight'], sd[f'head.rpn.cls_score.{i}.bias'])
           .view(bs, A, 2, h, w).softmax(2) for i, f in enumerate(feats)]
    reg = [F.conv2d(f, sd[f'head.rpn.bbox_reg.{i}.weight'], sd[f'head.rpn.bbox_reg.{i}.bias'])
           for i, f in enumerate(feats)]
    return torch.cat(cls, 1).view(bs, -1, h, w), torch.cat(reg, 1)


# --------------------------------------------------------------------------- anchors / boxes (P1, P2, P4)
def base_anchors(cfg):
    """generate_anchors_frcnn nets_utils.py:35-49 (float math then C-style int truncation)."""
    ratios = np.asarray(cfg.ratios, dtype=np.float64)
    scales = 2 ** np.arange(cfg.n_layers)
    wh = np.stack([np.sqrt(ratios), 1 / np.sqrt(ratios)], 1) * float(cfg.base_size)   # [R,2]
    wh = (wh[None] * scales[:, None, None]).reshape(-1, 2)                                # scale-major
    return (np.concatenate([-wh / 2, wh / 2], 1) + int(cfg.base_size / 2)).astype(int)


def all_anchors(cfg, height=None, width=None):
    """get_anchor_shifts_frcnn nets_utils.py:52-59 + broadcast at layers.py:258 -> [K*A,4], K-major."""
    h, w = (height, width) if height is not None else cfg.top_size
    sx = np.arange(w) * cfg.anchor_stride
    sy = np.arange(h) * cfg.anchor_stride
    shifts = np.stack([np.tile(sx, h), np.repeat(sy, w)], 1)
    shifts = np.concatenate([shifts, shifts], 1)[:, None, :]
    return (base_anchors(cfg)[None] + shifts).reshape(-1, 4)


def decode_boxes(deltas, anchors):
    """bbox_reg_to_coord nets_utils.py:169-186 (inclusive-pixel widths, torch.round = half-to-even)."""
    wa = anchors[..., 2] - anchors[..., 0] + 1
    ha = anchors[..., 3] - anchors[..., 1] + 1
    xa = anchors[..., 0] + 0.5 * wa
    ya = anchors[..., 1] + 0.5 * ha
    x = deltas[..., 0] * wa + xa
    y = deltas[..., 1] * ha + ya
    w = torch.exp(deltas[..., 2]) * wa
    h = torch.exp(deltas[..., 3]) * ha
    return torch.stack([(x - 0.5 * w).round(), (y - 0.5 * h).round(),
                        (x + 0.5 * w).round(), (y + 0.5 * h).round()], -1)


def encode_boxes(anchors, bbox):
    """bbox_transform nets_utils.py:129-146."""
    wa = anchors[:, 2] - anchors[:, 0] + 1
    ha = anchors[:, 3] - anchors[:, 1] + 1
    xa = anchors[:, 0] + 0.5 * wa
    ya = anchors[:, 1] + 0.5 * ha
    w = bbox[:, 2] - bbox[:, 0] + 1
    h = bbox[:, 3] - bbox[:, 1] + 1
    x = bbox[:, 0] + 0.5 * w
    y = bbox[:, 1] + 0.5 * h
    return torch.stack([(x - xa) / wa, (y - ya) / ha, torch.log(w / wa), torch.log(h / ha)], 1)


def pair_iou(a, b):
    """bbox_overlap nets_utils.py:103-126 / batch_self_overlap :189-207 as one broadcast:
    a [...,N,4], b [...,M,4] -> [...,N,M]; +1 pixel convention; union = area_a + area_b - inter
    in that association order."""
    a, b = a[..., :, None, :], b[..., None, :, :]
    xi = (torch.minimum(a[..., 2], b[..., 2]) - torch.maximum(a[..., 0], b[..., 0]) + 1).clamp(min=0)
    yi = (torch.minimum(a[..., 3], b[..., 3]) - torch.maximum(a[..., 1], b[..., 1]) + 1).clamp(min=0)
    inter = xi * yi
    aa = (a[..., 2] - a[..., 0] + 1) * (a[..., 3] - a[..., 1] + 1)
    ab = (b[..., 2] - b[..., 0] + 1) * (b[..., 3] - b[..., 1] + 1)
    return inter / ((aa + ab) - inter)


def greedy_nms_keep(boxes, thresh):
    """Keep list of `nms` nets_utils.py:221-233 for ONE image: walk in the given order, a kept box
    suppresses every later box with IoU >= thresh.  boxes [N,4] -> python list of kept indices."""
    n = boxes.shape[0]
    if n == 0:
        return []
    hit = (pair_iou(boxes, boxes) >= thresh).numpy()
    dead = np.zeros(n, dtype=bool)
    keep = []
    for i in range(n):
        if dead[i]:
            continue
        keep.append(i)
        dead[i + 1:] |= hit[i, i + 1:]
    return keep


def batched_nms(boxes, scores, thresh, topn):
    """`nms` nets_utils.py:210-245 incl. the batch-coupled truncation :236 (every image is cut to
    the smallest keep count in the batch).  boxes [B,N,4], scores [B,N]."""
    keeps = [greedy_nms_keep(boxes[b], thresh) for b in range(boxes.shape[0])]
    n = min(min(len(k) for k in keeps), topn)
    idx = torch.tensor([k[:n] for k in keeps], dtype=torch.long).reshape(boxes.shape[0], n)
    return (torch.gather(boxes, 1, idx[..., None].expand(-1, -1, 4)), torch.gather(scores, 1, idx), keeps)


# --------------------------------------------------------------------------- proposal layer (P3)
def proposal_layer(cfg, cls_scores, bbox_reg, training=False):
    """ProposalLayer.forward layers.py:226-303.  Returns (rois [B,R,4], scores [B,R]) or two empty
    tensors when fewer than rcnn_batch_size candidates survive ("RPN failed", :288-290).
    Score ties are ordered by ascending anchor index (stable descending sort)."""
    B = cls_scores.shape[0]
    h, w = cls_scores.shape[-2:]
    anchors = torch.from_numpy(all_anchors(cfg, h, w)).float()
    scores = cls_scores.permute(0, 2, 3, 1).reshape(B, -1, 2)[..., 1]
    deltas = bbox_reg.permute(0, 2, 3, 1).reshape(B, -1, 4)
    boxes = decode_boxes(deltas, anchors)
    boxes = torch.stack([boxes[..., 0].clamp(0, cfg.img_width - 1), boxes[..., 1].clamp(0, cfg.img_height - 1),
                         boxes[..., 2].clamp(0, cfg.img_width - 1), boxes[..., 3].clamp(0, cfg.img_height - 1)], -1)
    keep = ((boxes[..., 2] - boxes[..., 0] + 1 >= cfg.min_threshold) &
            (boxes[..., 3] - boxes[..., 1] + 1 >= cfg.min_threshold))
    pre = cfg.pre_nms_topN if training else cfg.pre_nms_topN_eval
    post = cfg.post_nms_topN if training else cfg.post_nms_topN_eval
    pre = min(pre, int(keep.sum(1).min()))
    if pre < cfg.rcnn_batch_size:
        return torch.tensor([]), torch.tensor([])
    order = torch.sort(scores, dim=1, descending=True, stable=True)[1]
    sel = []
    for b in range(B):
        ob = order[b]
        sel.append(ob[keep[b, ob]][:pre])
    sel = torch.stack(sel)
    s = torch.gather(scores, 1, sel)
    bx = torch.gather(boxes, 1, sel[..., None].expand(-1, -1, 4))
    rois, rs, _ = batched_nms(bx, s, cfg.nms_thresh, post)
    return rois, rs


# --------------------------------------------------------------------------- RoI pooling (M7)
def pe_table(length, cn, temp=10000):
    """one_dimension_positional_encoding position_encoding.py:10-15."""
    pos = torch.arange(1, length + 1, dtype=torch.float32)
    dt = temp ** (2 * torch.div(torch.arange(cn, dtype=torch.float32), 2, rounding_mode='trunc') / cn)
    pe = pos[:, None] / dt[None, :]
    return torch.stack([pe[:, 0::2].sin(), pe[:, 1::2].cos()], 2).flatten(1)


def roi_geometry(cfg, rois, heights, widths):
    """Level assignment + feature-map window of every RoI, layers.py:408-428,453-465.
    rois [B,R,4] -> int64 arrays lvl, x1, y1, x2, y2 of shape [B,R] (window inclusive)."""
    size = ((rois[..., 2] - rois[..., 0]) * (rois[..., 3] - rois[..., 1])) ** 0.5
    lvl = (torch.log(size * 0.1) / np.log(2)).int().clamp(min=0, max=cfg.n_layers - 1).long()
    stride = (2.0 ** (lvl + 1).float())
    x1 = (rois[..., 0] / stride).round().int().long()
    y1 = (rois[..., 1] / stride).round().int().long()
    x2 = (rois[..., 2] / stride).round().int().long()
    y2 = (rois[..., 3] / stride).round().int().long()
    H = torch.tensor(heights)[lvl]
    W = torch.tensor(widths)[lvl]
    y2 = torch.minimum(y2, H - 1)
    for _ in range(max(cfg.roi_pool_h, cfg.roi_pool_w)):            # the `while` loops :459-465
        grow = (y2 - y1 + 1) < cfg.roi_pool_h
        y1 = torch.where(grow, (y1 - 1).clamp(min=0), y1)
        y2 = torch.where(grow, torch.minimum(y2 + 1, H - 1), y2)
        grow = (x2 - x1 + 1) < cfg.roi_pool_w
        x1 = torch.where(grow, (x1 - 1).clamp(min=0), x1)
        x2 = torch.where(grow, torch.minimum(x2 + 1, W - 1), x2)
    return lvl, x1, y1, x2, y2


def roi_pooling(cfg, rois, fpn_out):
    """ROIPooling.forward layers.py:406-497 -> (pool [B,R,C,2,2], pe [B,R,C,2,2], lvl [B,R]).
    The RoI positional encoding is separable: channels [0,C/2) depend on rows only
    (pe_frequency[s*y1 : s*y2]) and [C/2,C) on columns only (pe_time[: s*(x2-x1)]) :484-489, so the
    2-D adaptive average is evaluated as 1-D bin means (in float64, rounded once)."""
    B, R = rois.shape[:2]
    C = fpn_out[0].shape[1]
    heights = [f.shape[-2] for f in fpn_out]
    widths = [f.shape[-1] for f in fpn_out]
    lvl, x1, y1, x2, y2 = roi_geometry(cfg, rois, heights, widths)
    ph, pw = cfg.roi_pool_h, cfg.roi_pool_w
    pe_f = pe_table(cfg.img_height, C // 2).double()
    pe_t = pe_table(cfg.img_width, C // 2).double()
    pool = torch.zeros(B, R, C, ph, pw)
    pe = torch.zeros(B, R, C, ph, pw)
    for b in range(B):
        for r in range(R):
            l = int(lvl[b, r])
            a, c, d, e = int(y1[b, r]), int(y2[b, r]), int(x1[b, r]), int(x2[b, r])
            pool[b, r] = F.adaptive_avg_pool2d(fpn_out[l][b, :, a:c + 1, d:e + 1], (ph, pw))
            s = 2 ** (l + 1)
            fr = pe_f[s * a:s * c]                       # [Hf, C/2]
            tm = pe_t[:s * (e - d)]                      # [Wt, C/2]
            hf, wt = fr.shape[0], tm.shape[0]
            for i in range(ph):
                lo, hi = (i * hf) // ph, -((-(i + 1) * hf) // ph)
                pe[b, r, :C // 2, i, :] = fr[lo:hi].mean(0).float()[:, None]
            for j in range(pw):
                lo, hi = (j * wt) // pw, -((-(j + 1) * wt) // pw)
                pe[b, r, C // 2:, :, j] = tm[lo:hi].mean(0).float()[:, None]
    return pool, pe, lvl


# --------------------------------------------------------------------------- RCNN head (M8)
def rcnn_forward(sd, cfg, pool, pe, training=False, new_buffers=None):
    """RCNN.forward layers.py:560-586 -> (bbox_reg [B*R, 4*(1+nc)], bbox_classes [B*R, 1+nc] softmaxed)."""
    p = 'head.fast_rcnn.rcnn.'
    roi_pe = F.conv2d(pe.flatten(end_dim=1), sd[p + 'pe_proj.weight'], sd[p + 'pe_proj.bias'])
    out = pool.flatten(end_dim=1)
    for j in range(cfg.depth_rcnn):
        out = dw_sep_conv(sd, f'{p}rcnn.{j}', out, 1, training, new_buffers, pe=roi_pe)
    feat = out.flatten(1)
    reg = F.linear(feat, sd[p + 'bbox_reg_layer.weight'], sd[p + 'bbox_reg_layer.bias'])
    cls = F.linear(feat, sd[p + 'bbox_classif_layer.weight'], sd[p + 'bbox_classif_layer.bias']).softmax(-1)
    return reg, cls


# --------------------------------------------------------------------------- Transformer_RCNN head
def _mha(x, qk_in, sd, p, nhead):
    """nn.MultiheadAttention on sequence-major tokens x [S, N, E]: q = k = qk_in, v = x (reference
    self_attention.py:124-126 / torch's TransformerEncoderLayer self-attention block)."""
    S, N, E = x.shape
    hd = E // nhead
    w, b = sd[p + '.in_proj_weight'], sd[p + '.in_proj_bias']
    q = F.linear(qk_in, w[:E], b[:E]).reshape(S, N * nhead, hd).transpose(0, 1)
    k = F.linear(qk_in, w[E:2 * E], b[E:2 * E]).reshape(S, N * nhead, hd).transpose(0, 1)
    v = F.linear(x, w[2 * E:], b[2 * E:]).reshape(S, N * nhead, hd).transpose(0, 1)
    att = torch.softmax(torch.bmm(q, k.transpose(1, 2)) / math.sqrt(hd), dim=-1)
    out = torch.bmm(att, v).transpose(0, 1).reshape(S, N, E)
    return F.linear(out, sd[p + '.out_proj.weight'], sd[p + '.out_proj.bias'])


def transformer_rcnn_forward(sd, cfg, pool, pe):
    """Transformer_RCNN.forward layers.py:636-651 (dropout 0).  Default branch: nn.TransformerEncoder with
    batch_first=False fed a [bs, rcnn_bs, 512] tensor, i.e. the SEQUENCE axis is the batch of images and the RoI slot
    is the transformer's batch axis (the reference's behaviour; post-norm, ReLU feed-forward).  `tf_pe_qk`: the DETR-style
    layer of self_attention.py:110-139 (batch_first=True, q = k = src + pos, LeakyReLU)."""
    p = 'head.fast_rcnn.rcnn.'
    B, R = pool.shape[:2]
    pos = F.leaky_relu(F.linear(pe.flatten(-3), sd[p + 'pos_embedding.0.weight'], sd[p + 'pos_embedding.0.bias']))
    roi = F.leaky_relu(F.linear(pool.flatten(-3), sd[p + 'rois_embedding.0.weight'], sd[p + 'rois_embedding.0.bias']))
    E = roi.shape[-1]
    if cfg.tf_pe_qk:
        x, posq = roi.transpose(0, 1), pos.transpose(0, 1)              # sequence-major [R, B, E]
    else:
        x, posq = roi + pos, None                                       # [S = B, N = R, E]
    for i in range(cfg.tf_num_encoder_layers):
        lp = f'{p}encoder.layers.{i}'
        a = _mha(x, x + posq if posq is not None else x, sd, lp + '.self_attn', cfg.tf_nhead)
        x = F.layer_norm(x + a, (E,), sd[lp + '.norm1.weight'], sd[lp + '.norm1.bias'], 1e-5)
        h = F.linear(x, sd[lp + '.linear1.weight'], sd[lp + '.linear1.bias'])
        h = F.leaky_relu(h) if cfg.tf_pe_qk else F.relu(h)
        h = F.linear(h, sd[lp + '.linear2.weight'], sd[lp + '.linear2.bias'])
        x = F.layer_norm(x + h, (E,), sd[lp + '.norm2.weight'], sd[lp + '.norm2.bias'], 1e-5)
    if cfg.tf_pe_qk:
        x = x.transpose(0, 1)
    reg = F.linear(x, sd[p + 'bbox_reg_layer.weight'], sd[p + 'bbox_reg_layer.bias']).flatten(end_dim=1)
    cls = F.linear(x, sd[p + 'bbox_classif_layer.weight'], sd[p + 'bbox_classif_layer.bias']).softmax(-1).flatten(end_dim=1)
    return reg, cls


# --------------------------------------------------------------------------- detection post-processing (M9)
def fast_rcnn_post(cfg, rois, bbox_reg, bbox_classes, nms_thresh=0.3, min_score=0.5):
    """FastRCNN.forward eval branch layers.py:688-776.  Output: list[B] of
    {'1'..'nc': {'bbox_coord': f32[n,4], 'scores': f32[1,n]}} with `torch.Tensor()` for empty classes.
    Score ties ordered by ascending RoI index (stable sort)."""
    B, R = rois.shape[:2]
    nc = cfg.num_classes
    scores, cls = bbox_classes.max(1)
    deltas = bbox_reg.view(B * R, nc + 1, 4)[torch.arange(B * R), cls].view(B, R, 4)
    scores, cls = scores.view(B, R), cls.view(B, R)
    out = []
    for b in range(B):
        bx = decode_boxes(deltas[b], rois[b])
        bx = torch.stack([bx[:, 0].clamp(0, cfg.img_width - 1), bx[:, 1].clamp(0, cfg.img_height - 1),
                          bx[:, 2].clamp(0, cfg.img_width - 1), bx[:, 3].clamp(0, cfg.img_height - 1)], 1)
        order = torch.sort(scores[b], descending=True, stable=True)[1]
        s, bx, c = scores[b][order], bx[order], cls[b][order]
        nz = torch.nonzero(c > 0)[:, 0]
        if len(nz) > 0:
            s, bx, c = s[nz], bx[nz], c[nz]
            k = torch.tensor(greedy_nms_keep(bx, nms_thresh), dtype=torch.long)
            s, bx, c = s[k], bx[k], c[k]                       # :742-746 (nested-list index == keep[0])
        res = {}
        for ci in range(1, nc + 1):
            w = torch.nonzero(c == ci)[:, 0]
            if len(w) == 0:
                res[str(ci)] = dict(bbox_coord=torch.Tensor(), scores=torch.Tensor())
                continue
            cb, cs = bx[w], s[w]
            k = torch.tensor(greedy_nms_keep(cb, nms_thresh)[:cfg.proposal_number], dtype=torch.long)
            cb, cs = cb[k], cs[k]
            m = torch.nonzero(cs > min_score)[:, 0]
            if len(m) == 0:
                res[str(ci)] = dict(bbox_coord=torch.tensor([]), scores=torch.tensor([]))
            else:
                res[str(ci)] = dict(bbox_coord=cb[m], scores=cs[m][None])
        out.append(res)
    return out


# --------------------------------------------------------------------------- full model
def sine_position_encoding(x, one_dim=True):
    """PositionEmbeddingSine(normalize=True, only_y_scale=one_dim) position_encoding.py:35-56: [B, C, h, w] with
    num_pos_feats = the channel count of x."""
    bs, c, h, w = x.shape
    ones = torch.ones((bs, h, w))
    y_embed, x_embed = ones.cumsum(1, dtype=torch.float32), ones.cumsum(2, dtype=torch.float32)
    y_embed = y_embed / (y_embed[:, -1:, :] + 1e-6) * (2 * math.pi)
    x_embed = x_embed / (x_embed[:, :, -1:] + 1e-6) * (2 * math.pi)
    dim_t = torch.arange(c, dtype=torch.float32)
    dim_t = 10000 ** (2 * torch.div(dim_t, 2, rounding_mode='trunc') / c)
    enc = lambda e: torch.stack(((e[..., None] / dim_t)[..., 0::2].sin(), (e[..., None] / dim_t)[..., 1::2].cos()), dim=4).flatten(3)
    pos = enc(y_embed) if one_dim else torch.cat((enc(y_embed), enc(x_embed)), dim=3)
    return pos.permute(0, 3, 1, 2)


def forward_first_stage(sd, cfg, x, training=False, new_buffers=None):
    """NbmModel.forward_first_stage nbm_model.py:39-54: fpn(attn(features)) by default, attn(fpn(.)) with `fpn_first`,
    attn[1](fpn(attn[0](.))) with `sandwich_attn`; `add_posenc` adds the sine encoding to the backbone taps first."""
    feats = backbone_forward(sd, x, getattr(cfg, 'dilation', False))
    if getattr(cfg, 'add_posenc', False):
        feats = [f + sine_position_encoding(f, getattr(cfg, 'one_dim_posenc', True)) for f in feats]
    top_n = cfg.pyramid_top_n_attn
    if getattr(cfg, 'fpn_first', False):
        fpn_out = sa_pyramid(sd, fpn_forward(sd, feats), top_n)
    elif getattr(cfg, 'sandwich_attn', False):
        fpn_out = sa_pyramid(sd, fpn_forward(sd, sa_pyramid(sd, feats, top_n, 'attn.0')), top_n, 'attn.1')
    elif getattr(cfg, 'fpn', 'fpn') == 'bifpn':
        fpn_out = bifpn_forward(sd, sa_pyramid(sd, feats, top_n), cfg.n_bifpn_layers, training, new_buffers)
    else:
        fpn_out = fpn_forward(sd, sa_pyramid(sd, feats, top_n))
    cls, reg = rpn_forward(sd, cfg, fpn_out, training, new_buffers)
    with torch.no_grad():
        rois, roi_scores = proposal_layer(cfg, cls.detach(), reg.detach(), training)
    return {'rois': rois, 'roi_scores': roi_scores, 'rpn_cls_scores': cls, 'rpn_bbox_reg': reg, 'fpn_out': fpn_out}


def forward_second_stage(sd, cfg, fpn_out, rois, nms_thresh=0.3, min_score=0.5, training=False, new_buffers=None,
                         bn_training=None):
    """NbmModel.forward_second_stage nbm_model.py:56-64 / FastRCNN.forward layers.py:668-685.
    `training` selects raw outputs vs post-processed detections (the reference's `training` flag);
    `bn_training` is the module's own train/eval mode (defaults to `training`), Appendix C-11."""
    pool, pe, _ = roi_pooling(cfg, rois, fpn_out)
    if cfg.tf_rcnn:
        reg, cls = transformer_rcnn_forward(sd, cfg, pool, pe)
    else:
        reg, cls = rcnn_forward(sd, cfg, pool, pe, training if bn_training is None else bn_training, new_buffers)
    if training:
        return {'bbox_reg': reg, 'bbox_classes': cls}
    return fast_rcnn_post(cfg, rois, reg, cls, nms_thresh, min_score)


def forward(sd, cfg, x, nms_thresh=0.3, min_score=0.5):
    """NbmModel.forward nbm_model.py:66-80 (eval)."""
    o = forward_first_stage(sd, cfg, x, False)
    return forward_second_stage(sd, cfg, o['fpn_out'], o['rois'], nms_thresh, min_score, False)


# --------------------------------------------------------------------------- merge_images (M10)
def merge_images(w_pix, hop_spectro, spectrogram_length, outputs, num_classes, nms_thresh=0.3):
    """merge_images run_detection.py:163-249.  `outputs` = flat list of per-window dicts."""
    min_border = 0.9 * (w_pix - hop_spectro)
    boxes, scores, species = [], [], []
    n = len(outputs)
    for j in range(1, num_classes + 1):
        for i, o in enumerate(outputs):
            bb = o[str(j)]['bbox_coord']
            if len(bb) == 0:
                continue
            sc = o[str(j)]['scores'].reshape(-1)
            wd = bb[:, 2] - bb[:, 0]
            if i == 0:                                           # if/elif chain :195-200 (C-5)
                drop = (bb[:, 2] >= w_pix - 5) & (wd < min_border)
            elif i == n - 1:
                drop = (bb[:, 0] <= 4) & (wd < min_border)
            else:
                drop = ((bb[:, 0] <= 4) | (bb[:, 2] >= w_pix - 5)) & (wd < min_border)
            bb, sc = bb[~drop].clone(), sc[~drop]
            bb[:, 0] += hop_spectro * i
            bb[:, 2] += hop_spectro * i
            ok = ~(bb[:, 2] >= spectrogram_length)
            bb, sc = bb[ok], sc[ok]
            if len(bb) == 0:
                continue
            boxes.append(bb), scores.append(sc), species.extend([j] * len(bb))
    res = {str(j): {'bbox_coord': torch.tensor([]), 'scores': torch.tensor([])} for j in range(1, num_classes + 1)}
    if boxes:
        boxes, scores, species = torch.cat(boxes), torch.cat(scores), np.array(species)
        k = greedy_nms_keep(boxes, nms_thresh)                   # input order, NOT re-sorted (:233)
        boxes, scores, species = boxes[k], scores[k], species[k]
        for j in range(1, num_classes + 1):
            m = torch.from_numpy(species == j)
            if m.any():
                res[str(j)] = {'bbox_coord': boxes[m], 'scores': scores[m]}
    return res


# --------------------------------------------------------------------------- training targets + losses (L1..L4)
class NumpySampler:
    """Default subsampler = the reference's `np.random.choice(arr, n, replace=False)` on the global
    NumPy stream (layers.py:187,196,370-376); tests may inject recorded indices instead."""

    def choice(self, arr, n):
        return np.random.choice(arr, n, replace=False)


def anchor_targets(cfg, gt_bbox, lengths, sampler=None):
    """AnchorTargetLayer.forward layers.py:134-216 -> labels [B,A,h,w] (int64, -1/0/1),
    reg_targets [B,4A,h,w]."""
    sampler = sampler or NumpySampler()
    h, w = cfg.top_size
    alla = all_anchors(cfg)
    inside = np.where((alla[:, 0] >= 0) & (alla[:, 1] >= 0) & (alla[:, 2] < cfg.img_width) &
                      (alla[:, 3] < cfg.img_height))[0]
    anc = torch.from_numpy(alla[inside]).float()
    A = len(base_anchors(cfg))
    B = len(lengths)
    ov = pair_iou(anc, gt_bbox)
    labels = torch.full((B, len(inside)), -1, dtype=torch.long)
    tgt = torch.zeros(B, len(inside), 4)
    idx = np.cumsum([0] + list(lengths))
    for b, (i0, i1) in enumerate(zip(idx[:-1], idx[1:])):
        o = ov[:, i0:i1]
        mx, amx = o.max(1)
        gmx, _ = o.max(0)
        labels[b, mx < cfg.rpn_neg_label] = 0
        labels[b, mx >= cfg.rpn_pos_label] = 1
        if gmx.max().item() > 0:
            pos = torch.nonzero(gmx > 0)[:, 0]
            labels[b, torch.nonzero(o[:, pos] == gmx[pos])[:, 0]] = 1
        num_fg = int(cfg.rpn_fg_fraction * cfg.rpn_batchsize)
        fg = torch.nonzero(labels[b] == 1)[:, 0]
        if len(fg) > num_fg:
            labels[b, sampler.choice(fg.numpy(), len(fg) - num_fg)] = -1
        num_bg = cfg.rpn_batchsize - int((labels[b] == 1).sum())
        bg = torch.nonzero(labels[b] == 0)[:, 0]
        if len(bg) > num_bg:
            labels[b, sampler.choice(bg.numpy(), len(bg) - num_bg)] = -1
        tgt[b] = encode_boxes(anc, gt_bbox[i0:i1][amx])
    tgt = labels.unsqueeze(2).clamp(min=0) * tgt
    all_l = torch.full((B, len(alla)), -1, dtype=torch.long)
    all_l[:, inside] = labels
    all_t = torch.zeros(B, len(alla), 4)
    all_t[:, inside] = tgt
    return (all_l.view(B, h, w, A).permute(0, 3, 1, 2), all_t.view(B, h, w, A * 4).permute(0, 3, 1, 2))


def proposal_targets(cfg, rois, gt_bbox, bird_ids, lengths, sampler=None):
    """ProposalTargetLayer.forward layers.py:312-396 -> (rois [B,16,4], bbox_targets [B,16,4(1+nc)],
    labels [B,16] float) or (None, None, None)."""
    sampler = sampler or NumpySampler()
    nc, nb = cfg.num_classes, cfg.rcnn_batch_size
    out_r, out_t, out_l = [], [], []
    idx = np.cumsum([0] + list(lengths))
    for b, (i0, i1) in enumerate(zip(idx[:-1], idx[1:])):
        gt = gt_bbox[i0:i1]
        allr = torch.cat([rois[b], gt], 0) if gt.max().item() > -1 else rois[b]
        mx, asg = pair_iou(allr, gt).max(-1)
        lab = bird_ids[i0:i1][asg].clone()
        lab[mx < cfg.fg_threshold] = 0
        gt = gt[asg]
        fg = torch.nonzero(mx > cfg.fg_threshold)[:, 0]
        bg = torch.nonzero((cfg.bg_threshold_hi > mx) & (mx >= cfg.bg_threshold_lo))[:, 0]
        other = list(set(range(len(mx))) - set(bg.numpy()) - set(fg.numpy()))
        nfg = min(len(fg), int(cfg.rcnn_fg_prop * nb))
        if len(bg) + len(other) < nb - nfg:
            if len(bg) + len(other) < nb - len(fg):
                return None, None, None
            nfg = max(nfg, nb - (len(bg) + len(other)))
        nbg = min(len(bg), nb - nfg)
        fgi = sampler.choice(fg.numpy(), nfg)
        bgi = sampler.choice(bg.numpy(), nbg)
        if len(fgi) + len(bgi) < nb:
            bgi = np.hstack([bgi, sampler.choice(other, nb - len(fgi) - len(bgi))])
        keep = torch.from_numpy(np.hstack((fgi, bgi)).astype(np.int64))
        bl, br = lab[keep], allr[keep]
        t4 = encode_boxes(br, gt[keep])
        exp = torch.zeros(nb, 4 * (1 + nc))                       # get_bbox_regression_targets nets_utils.py:248-259
        li = bl.long()
        for r in range(nb):
            if li[r] >= 1:
                exp[r, 4 * li[r]:4 * li[r] + 4] = t4[r]
        out_r.append(br), out_t.append(exp), out_l.append(bl)
    return torch.stack(out_r), torch.stack(out_t), torch.stack(out_l)


def smooth_l1(a, b):
    """smooth_l1_loss_rcnn nets_utils.py:275-281 (beta=1)."""
    d = (a - b).abs()
    big = d >= 1
    return (~big).float() * 0.5 * d ** 2 + big.float() * (d - 0.5)


def first_stage_loss(cfg, cls, reg, gt_bbox=None, lengths=None, neg=False, sampler=None):
    """SetCriterion.first_stage_loss nbm_model.py:102-164.  The negative branch reproduces the
    reference's broadcasting gather (Appendix C-15a): only the top-1 anchor per image contributes,
    through BOTH of its probabilities."""
    if neg:
        B = cls.shape[0]
        p = cls.permute(0, 2, 3, 1).reshape(B, -1, 2)
        top = torch.sort(p[..., 1], dim=1, descending=True, stable=True)[1][:, 0]
        top_p = p[torch.arange(B), top]                          # [B,2]
        return {'first_neg_class_loss': (-torch.log(top_p)).mean()}
    labels, tgt = anchor_targets(cfg, gt_bbox, lengths, sampler)
    p = cls.permute(0, 2, 3, 1).reshape(-1, 2)
    lab = labels.permute(0, 2, 3, 1).flatten()
    keep = torch.nonzero(lab != -1)[:, 0]
    p, lab = p[keep], lab[keep]
    ce = (-torch.log(p[torch.arange(len(p)), lab])).sum() * (1 / len(p))
    r = reg.permute(0, 2, 3, 1).reshape(-1, 4)[keep]
    t = tgt.permute(0, 2, 3, 1).reshape(-1, 4)[keep]
    rl = (smooth_l1(r, t) * (lab == 1).float()[:, None]).sum()
    if rl > 0:
        rl = rl * (4 / (lab > 0).sum())
    return {'first_class_loss': ce, 'first_regression_loss': rl}


def second_stage_loss(cfg, bbox_reg, bbox_classes, bbox_targets=None, labels=None, neg=False):
    """SetCriterion.second_stage_loss nbm_model.py:171-217.  Negative branch: the reference's n x n
    gather has value and gradient identical to mean(-log p[:,0]) (Appendix C-15b)."""
    if neg:
        return {'sec_neg_class_loss': (-torch.log(bbox_classes[:, 0])).mean()}
    B, nb, nc = len(bbox_targets), cfg.rcnn_batch_size, cfg.num_classes
    t = bbox_targets.view(B * nb, 4 * (nc + 1))
    lab = labels.flatten().long()
    pg = bbox_classes[torch.arange(len(lab)), lab]
    if cfg.focal_loss:
        ce = (-(1 - pg).pow(1.5) * torch.log(pg)).mean()            # focal_loss_rcnn nets_utils.py:319-329
    else:
        ce = (-torch.log(pg)).sum() * (1 / (B * nb))
    mask = torch.zeros_like(bbox_reg)
    ar = torch.arange(len(lab))
    for i in range(4):
        mask[ar, i + lab * 4] = 1
    mask[:, 0:4] = 0
    rl = (mask * smooth_l1(bbox_reg, t)).sum()
    if rl > 0:
        rl = rl * (4 / (lab > 0).sum())
    return {'sec_class_loss': ce, 'sec_regression_loss': rl}


def train_step_losses(sd, cfg, img, bb_coord, bird_ids, lengths, neg=False, training=True, sampler=None,
                      new_buffers=None):
    """`step` train.py:220-257.  img [B,H,W]; returns the loss dict (+ 'cardinality_error')."""
    o = forward_first_stage(sd, cfg, img[:, None], training, new_buffers)
    loss = dict(first_stage_loss(cfg, o['rpn_cls_scores'], o['rpn_bbox_reg'], bb_coord, lengths, neg, sampler))
    if len(o['rois']) == 0:
        return loss
    if not neg:
        rois, tg, lab = proposal_targets(cfg, o['rois'], bb_coord, bird_ids, lengths, sampler)
        if rois is None:
            return loss
    else:
        rois, tg, lab = o['rois'], None, None
    s = forward_second_stage(sd, cfg, o['fpn_out'], rois, training=True, new_buffers=new_buffers,
                             bn_training=training)
    loss.update(second_stage_loss(cfg, s['bbox_reg'], s['bbox_classes'], tg, lab, neg))
    if not neg:
        loss['cardinality_error'] = int((s['bbox_classes'].argmax(-1) != 0).sum()) - int((lab != 0).sum())
    return loss
