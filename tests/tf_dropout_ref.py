"""Torch statement of the Transformer_RCNN head (`--tf_rcnn`, both encoder flavours) with a keep mask injected at each of the four
dropout sites of every encoder layer -- what nn.TransformerEncoderLayer / the DETR-style layer of the reference compute in training
mode once the random draws are given.  With all-ones masks it is oracle.nets_ref.transformer_rcnn_forward (tests/test_tf_dropout_cpu.py),
which is pinned on the real reference.

Tokens are kept as [B, R, E] (image, RoI slot).  Mask layouts are those of the library (include/nbm_hip.h, `nbm_dropout` /
`nbm_mha_small_drop`): sites 1 and 3 a [B * R, E] tensor, site 2 [B * R, dim_feedforward], row b * R + r; site 0 a dense
[N, nhead, S, S] tensor (query row, key column) with (N, S) = (R, B) for the default flavour, which attends across the images of
the batch for every RoI slot, and (B, R) for `tf_pe_qk`, which attends across the RoIs of an image."""
import math

import torch
import torch.nn.functional as F

from birdsoundclassif_amd import ops


def mask_shapes(cfg, B, R, E):
    """{site: shape} of the four masks of one encoder layer."""
    N, S = (B, R) if cfg.tf_pe_qk else (R, B)
    return {0: (N, cfg.tf_nhead, S, S), 1: (B * R, E), 2: (B * R, cfg.tf_dim_feedforward), 3: (B * R, E)}


def reference_masks(cfg, B, R, E, p, seed, call):
    """{(layer, site): bool tensor} from `ops.dropout_keep_reference`, site_id = 4 * layer + site."""
    out = {}
    for layer in range(cfg.tf_num_encoder_layers):
        for site, shape in mask_shapes(cfg, B, R, E).items():
            keep = ops.dropout_keep_reference(seed, call, 4 * layer + site, math.prod(shape), p)
            out[layer, site] = torch.from_numpy(keep).view(shape)
    return out


def ones_masks(cfg, B, R, E):
    return {(layer, site): torch.ones(shape, dtype=torch.bool) for layer in range(cfg.tf_num_encoder_layers)
            for site, shape in mask_shapes(cfg, B, R, E).items()}


def _drop(x, keep, p):
    """y = keep ? x / (1 - p) : 0."""
    return torch.where(keep.view(x.shape), x / (1.0 - p), torch.zeros_like(x))


def head_forward(sd, cfg, pool, pe, masks, p):
    """sd: state_dict with the 'head.fast_rcnn.rcnn.' prefix (any float dtype), pool / pe [B, R, C, ph, pw]
    -> (bbox_reg [B*R, 4(1+nc)], bbox_classes [B*R, 1+nc])."""
    pre = 'head.fast_rcnn.rcnn.'
    B, R = pool.shape[:2]
    nh = cfg.tf_nhead
    pos = F.leaky_relu(F.linear(pe.flatten(-3), sd[pre + 'pos_embedding.0.weight'], sd[pre + 'pos_embedding.0.bias']))
    x = F.leaky_relu(F.linear(pool.flatten(-3), sd[pre + 'rois_embedding.0.weight'], sd[pre + 'rois_embedding.0.bias']))
    E = x.shape[-1]
    hd = E // nh
    if not cfg.tf_pe_qk:
        x = x + pos
    for i in range(cfg.tf_num_encoder_layers):
        lp = f'{pre}encoder.layers.{i}.'
        w, b = sd[lp + 'self_attn.in_proj_weight'], sd[lp + 'self_attn.in_proj_bias']
        qk_in = x + pos if cfg.tf_pe_qk else x
        q = F.linear(qk_in, w[:E], b[:E]).view(B, R, nh, hd)
        k = F.linear(qk_in, w[E:2 * E], b[E:2 * E]).view(B, R, nh, hd)
        v = F.linear(x, w[2 * E:], b[2 * E:]).view(B, R, nh, hd)
        if cfg.tf_pe_qk:            # [B, nh, R, R]: queries and keys are the RoIs of one image
            att = _drop(torch.softmax(torch.einsum('brhd,bshd->bhrs', q, k) / math.sqrt(hd), -1), masks[i, 0], p)
            a = torch.einsum('bhrs,bshd->brhd', att, v)
        else:                       # [R, nh, B, B]: queries and keys are the images of the batch, per RoI slot
            att = _drop(torch.softmax(torch.einsum('brhd,crhd->rhbc', q, k) / math.sqrt(hd), -1), masks[i, 0], p)
            a = torch.einsum('rhbc,crhd->brhd', att, v)
        a = F.linear(a.reshape(B, R, E), sd[lp + 'self_attn.out_proj.weight'], sd[lp + 'self_attn.out_proj.bias'])
        x = F.layer_norm(x + _drop(a, masks[i, 1], p), (E,), sd[lp + 'norm1.weight'], sd[lp + 'norm1.bias'], 1e-5)
        h = F.linear(x, sd[lp + 'linear1.weight'], sd[lp + 'linear1.bias'])
        h = _drop(F.leaky_relu(h) if cfg.tf_pe_qk else F.relu(h), masks[i, 2], p)
        h = F.linear(h, sd[lp + 'linear2.weight'], sd[lp + 'linear2.bias'])
        x = F.layer_norm(x + _drop(h, masks[i, 3], p), (E,), sd[lp + 'norm2.weight'], sd[lp + 'norm2.bias'], 1e-5)
    reg = F.linear(x, sd[pre + 'bbox_reg_layer.weight'], sd[pre + 'bbox_reg_layer.bias']).flatten(end_dim=1)
    cls = F.linear(x, sd[pre + 'bbox_classif_layer.weight'], sd[pre + 'bbox_classif_layer.bias']).softmax(-1).flatten(end_dim=1)
    return reg, cls
