"""Per-file detection driver (reference nbm_model/run_detection.py): `load_model`, `run_detection`, `merge_images`.

`run_detection` keeps the reference's signature and output dict; the spectrogram windows stay on the GPU between the
front end and the detector, and the whole cross-window merge of the file runs on the device (csrc/merge.hip): collect,
greedy NMS and gather, then one device-to-host copy.  `merge_images` is the reference-named dictionary API; its NMS runs
on the same device entry point.  Both take up to ops.MERGE_MAX_N = 131 072 candidate boxes per file."""
import json
import os

import numpy as np
import torch

from . import ops
from .nbm_datasets.prepare_dataset import File_Processor
from .nets.backbone import build_backbone
from .nets.fpn import build_fpn
from .nets.head import build_head
from .nets.nbm_model import NbmModel, initialize_model
from .nets.self_attention import build_sa_layers
from .nets.util.nets_utils import setattr_others

device = 'cuda'


def merge_images(fp, outputs, num_classes, nms_thresh=0.3):
    """Cross-window merge (reference run_detection.py:163-249): drop narrow border boxes (first / last / inner window
    rules, if/elif chain kept: Appendix C-5), shift by HOP_SPECTRO*i, drop boxes past the end of the file, then one
    class-agnostic greedy NMS over the file IN THE COLLECTED ORDER (class-major, not re-sorted by score)."""
    min_border_size = 0.9 * (fp.W_PIX - fp.HOP_SPECTRO)
    out = []
    for b_outputs in outputs:
        out.extend(b_outputs)
    boxes, scores, species = [], [], []
    for j in range(1, num_classes + 1):
        for i, img_out in enumerate(out):
            bb = img_out[str(j)]['bbox_coord']
            if len(bb) == 0:
                continue
            bb = bb.detach().float().cpu().clone()
            sc = img_out[str(j)]['scores'].detach().float().cpu().reshape(-1)
            widths = bb[:, 2] - bb[:, 0]
            if i == 0:
                drop = (bb[:, 2] >= fp.W_PIX - 5) & (widths < min_border_size)
            elif i == len(out) - 1:
                drop = (bb[:, 0] <= 4) & (widths < min_border_size)
            else:
                drop = ((bb[:, 0] <= 4) | (bb[:, 2] >= fp.W_PIX - 5)) & (widths < min_border_size)
            bb, sc = bb[~drop], sc[~drop]
            bb[:, 0] += fp.HOP_SPECTRO * i
            bb[:, 2] += fp.HOP_SPECTRO * i
            ok = ~(bb[:, 2] >= fp.spectrogram_length)
            bb, sc = bb[ok], sc[ok]
            if len(bb) == 0:
                continue
            boxes.append(bb), scores.append(sc), species.extend([j] * len(bb))
    class_bbox = {str(j): {'bbox_coord': torch.tensor([]), 'scores': torch.tensor([])} for j in range(1, num_classes + 1)}
    if not boxes:
        return class_bbox
    boxes, scores, species = torch.cat(boxes), torch.cat(scores), np.array(species)
    n = len(boxes)
    if n > ops.MERGE_MAX_N:
        raise ValueError(f'{n} candidate boxes in one file: the device merge handles up to {ops.MERGE_MAX_N}')
    n_in = torch.full((1,), n, device=device, dtype=torch.int32)
    kept_idx, n_out = ops.merge_nms(boxes.to(device).contiguous(), n_in, nms_thresh)
    keep = kept_idx[:int(n_out.item())].long().cpu()
    boxes, scores, species = boxes[keep], scores[keep], species[keep.numpy()]
    for j in range(1, num_classes + 1):
        m = torch.from_numpy(species == j)
        if m.any():
            class_bbox[str(j)] = {'bbox_coord': boxes[m], 'scores': scores[m]}
    return class_bbox


def run_detection(model, config, wav_path, bird_dicts_path, min_score=0.5, bs=10, visualise_outputs=False, show_sp_name=True):
    """reference run_detection.py:28-84 -> {species_name: {'bbox_coord': [[x1,y1,x2,y2]...], 'scores': [...]}}."""
    if visualise_outputs:
        raise NotImplementedError('visualisation is outside the hot-path scope')
    fp = File_Processor(wav_path)
    img_db, _ = fp.process_file(device=device)
    if img_db is None:
        return {}
    if len(img_db) > 0 and isinstance(img_db[0], list):
        # recordings longer than 56 min: process_file returns one image list per split (reference process_long_file);
        # the reference's own run_detection indexes that as a flat image list and fails (run_detection.py:44-55)
        raise NotImplementedError('recordings longer than 1.5e8 samples come back as nested per-split image lists, which '
                                  'the reference detection loop cannot consume either; split the recording first')
    imgs = fp.images_device                                   # [n_img, 375, 1024] on the GPU
    n_img = imgs.shape[0]
    if n_img == 0:
        return {}
    det_all, n_all = None, None
    for s in range(0, n_img, bs):
        # the same model calls (and batch coupling of the proposal counts) as `model(...)` per group of bs windows; the rows
        # live in reused scratch, so they are copied out before the next call
        det, n_det = model.detect(imgs[s:s + bs][:, None].contiguous(), 0.3, min_score)
        if det_all is None:
            det_all = torch.empty((n_img,) + tuple(det.shape[1:]), device=det.device, dtype=det.dtype)
            n_all = torch.empty((n_img,), device=det.device, dtype=torch.int32)
        det_all[s:s + det.shape[0]].copy_(det)
        n_all[s:s + det.shape[0]].copy_(n_det)
    with open(bird_dicts_path, 'r') as f:
        birds_dict = json.load(f)
    rows = merge_device(fp, det_all, n_all, config.num_classes)
    return rows_to_output(rows, config.num_classes, species_names(birds_dict))


def species_names(birds_dict):
    """bird_dict.json content {name: id} -> {id: name} with 0 = 'Non bird sound' (reference run_detection.py:60-62)."""
    birds_dict = dict(birds_dict)
    birds_dict.update({'Non bird sound': 0})
    return {idx: name for name, idx in birds_dict.items()}


def rows_to_output(rows, num_classes, reverse_dict):
    """Merged rows (float32 CPU [n,6] {species,x1,y1,x2,y2,score}, `merge_device`) -> the per-file output dictionary of
    `run_detection`: {species name: {'bbox_coord': [[x1,y1,x2,y2]...], 'scores': [...]}}, species ascending."""
    species = rows[:, 0].to(torch.int64).numpy()
    out = {}
    for idx in range(1, num_classes + 1):
        m = species == idx
        if m.any():
            sel = rows[torch.from_numpy(m)]
            out[reverse_dict[idx]] = {'bbox_coord': sel[:, 1:5].numpy().tolist(), 'scores': sel[:, 5].numpy().tolist()}
    return out


def merge_device(fp, det, n_det, num_classes, nms_thresh=0.3):
    """`merge_images` on the detector's device rows of one file: det [n_img,cap,6] ({class,x1,y1,x2,y2,score}, sorted by
    (class, score desc) per window), n_det int32 [n_img] -> float32 CPU rows [n,6] {species,x1,y1,x2,y2,score} in the kept
    (class-major) order.  Collect, NMS and gather are queued without a host sync; one copy brings the result back."""
    return ops.unpack_merged(merge_device_async(fp, det, n_det, num_classes, nms_thresh))


def merge_device_async(fp, det, n_det, num_classes, nms_thresh=0.3):
    """The device half of `merge_device`: -> the device buffer of `ops.merge_gather` (`ops.unpack_merged` reads it).  No host
    sync for any file the per-file driver takes (<= 1.5e8 samples).  `fp`: anything with W_PIX, HOP_SPECTRO,
    spectrogram_length."""
    boxes, scores, species, n = ops.merge_collect(det, n_det, fp.W_PIX, fp.HOP_SPECTRO, fp.spectrogram_length, num_classes)
    cap = boxes.shape[0]
    if cap > ops.MERGE_MAX_N:
        # only reachable past ~2 600 windows, longer than the 1.5e8-sample split limit: the count decides
        if int(n.item()) > ops.MERGE_MAX_N:
            raise ValueError(f'{int(n.item())} candidate boxes in one file: the device merge handles up to {ops.MERGE_MAX_N}')
        cap = ops.MERGE_MAX_N
    keep, n_keep = ops.merge_nms(boxes, n, nms_thresh, cap)
    return ops.merge_gather(boxes, scores, species, keep, n_keep, cap)


def load_model(mod_p):
    """reference run_detection.py:87-122: directory with JSON `args` + `model_chkpt.pt`."""
    class Args:
        def __init__(self, **kwargs):
            for (k, v) in kwargs.items():
                setattr(self, k, v)

    with open(os.path.join(mod_p, 'args'), 'rb') as f:
        args = Args(**json.load(f))
    args.device = device          # placement follows this process, not the string stored in the file (Appendix C-13)
    setattr_others(args)
    backbone = build_backbone(args, inference=True)
    attn = build_sa_layers(args, backbone.num_channels)
    fpn = build_fpn(args, backbone.num_channels)
    head = build_head(args)
    model = NbmModel(args, backbone, attn, fpn, head).to(device)
    model = initialize_model(model, path=os.path.join(mod_p, 'model_chkpt.pt'), train=False)
    return model, args
