"""RoI pooling forward and backward at several pool sizes; prints a table and one JSON line.

    python scripts/bench_roi_pool.py [--rounds 7] [--window_ms 40] [--skip_steps] [--out profiles/roi_pool.txt]

Dense random FPN maps of the real sizes (C = 256) and seeded boxes spread over all pyramid levels, at B = 64 with 50 RoIs per
image (the evaluation step) and at B = 128 with 1 000 (the negative training step).  The library entry points are called
directly on preallocated outputs (no fills in the timed region), HIP events around windows of about --window_ms of
back-to-back calls after a warm-up, --rounds windows per variant, the variants of one leg alternating; median, minimum and
maximum per call.  Variants: nbm_roi_pool_hw / nbm_roi_pool_hw_bwd at 2 x 2, 3 x 3 and 7 x 7.  `bytes` is what a launch has to move -- the window pixels once (twice for the backward pass: an atomic reads and
writes) plus the pooled rows -- and `of peak` that figure over the median time as a fraction of 6.3 TB/s.

Without --skip_steps: the eager detect step at B = 64 and one positive training step at B = 128 with `--roi_pool_h 3
--roi_pool_w 3` (dense FPN maps) beside the 2 x 2 default (on-demand maps) of the same run."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IMG_W, IMG_H, C_FPN = 1024, 375, 256
FMAP_HW = [(188, 512), (94, 256), (47, 128), (24, 64), (12, 32)]
PEAK = 6.3e12


def timed(fn, window_ms):
    import torch
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(), fn(), e1.record()
    torch.cuda.synchronize()
    reps = max(3, min(2000, int(window_ms / max(e0.elapsed_time(e1), 1e-3))))

    def window():
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps
    return window, reps


def alternate(variants, rounds, window_ms):
    windows = {name: timed(fn, window_ms) for name, fn in variants.items()}
    ms = {name: [] for name in variants}
    for _ in range(rounds):
        for name, (window, _) in windows.items():
            ms[name].append(window())
    return {name: {'median_us': round(1e3 * statistics.median(ms[name]), 1), 'min_us': round(1e3 * min(ms[name]), 1),
                   'max_us': round(1e3 * max(ms[name]), 1), 'reps': windows[name][1]} for name in variants}


def boxes(B, R, seed):
    """[B, R, 4] float32 boxes inside the image, side lengths log-uniform between 12 and 340 pixels: every level gets RoIs."""
    import torch
    gen = torch.Generator().manual_seed(seed)
    u = torch.rand(B, R, 4, generator=gen)
    w = (12.0 * (340.0 / 12.0) ** u[..., 0]).clamp(max=IMG_W - 1).round()
    h = (12.0 * (340.0 / 12.0) ** u[..., 1]).clamp(max=IMG_H - 1).round()
    x1 = (u[..., 2] * (IMG_W - 1 - w)).round()
    y1 = (u[..., 3] * (IMG_H - 1 - h)).round()
    return torch.stack([x1, y1, x1 + w, y1 + h], -1).contiguous()


def window_pixels(rois, ph, pw):
    """Pixels under the RoI windows (the oracle's geometry), summed over all RoIs."""
    import torch
    from oracle import nets_ref as O
    lvl, x1, y1, x2, y2 = O.roi_geometry(O.make_cfg(roi_pool_h=ph, roi_pool_w=pw), rois, [h for h, _ in FMAP_HW],
                                         [w for _, w in FMAP_HW])
    W = torch.tensor([w for _, w in FMAP_HW])[lvl]
    return int(((y2 - y1 + 1) * (torch.minimum(x2, W - 1) - x1 + 1)).sum())


def pool_leg(B, R, rounds, window_ms):
    import torch
    from birdsoundclassif_amd import _lib, ops
    from birdsoundclassif_amd.nets.position_encoding import one_dimension_positional_encoding as pe1d
    lib = ops.lib()
    st = ops._stream()
    gen = torch.Generator(device='cuda').manual_seed(B)
    fm = [torch.randn(B, h, w, C_FPN, generator=gen, device='cuda') for h, w in FMAP_HW]
    gf = [torch.zeros_like(f) for f in fm]
    rois_h = boxes(B, R, B)
    rois = rois_h.cuda()
    n_roi = torch.full((B,), R, device='cuda', dtype=torch.int32)
    pe_f, pe_t = pe1d(IMG_H, C_FPN // 2).cuda().contiguous(), pe1d(IMG_W, C_FPN // 2).cuda().contiguous()
    n = len(fm)
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in gf])
    fh = (ctypes.c_int * n)(*[h for h, _ in FMAP_HW])
    fw = (ctypes.c_int * n)(*[w for _, w in FMAP_HW])
    variants, info, keep = {}, {}, []
    for name, ph, pw in (('2x2', 2, 2), ('3x3', 3, 3), ('7x7', 7, 7)):
        d = _lib.RoiHwDesc()
        for i, f in enumerate(fm):
            d.fmap[i], d.fh[i], d.fw[i] = f.data_ptr(), f.shape[1], f.shape[2]
        pool = torch.zeros(B * R, ph, pw, C_FPN, device='cuda')
        pe = torch.zeros_like(pool)
        level = torch.zeros(B, R, device='cuda', dtype=torch.int32)
        gpool = torch.randn(B * R, ph, pw, C_FPN, generator=gen, device='cuda')
        keep += [pool, pe, level, gpool, d]
        d.n_levels, d.C, d.rois, d.n_roi, d.B, d.roi_cap = n, C_FPN, rois.data_ptr(), n_roi.data_ptr(), B, R
        d.pe_f, d.pe_t, d.img_h, d.img_w = pe_f.data_ptr(), pe_t.data_ptr(), IMG_H, IMG_W
        d.pool, d.pe, d.level = pool.data_ptr(), pe.data_ptr(), level.data_ptr()
        d.pool_h, d.pool_w = ph, pw

        def fwd(d=d):
            ops.check(lib.nbm_roi_pool_hw(ctypes.byref(d), st), 'nbm_roi_pool_hw')

        def bwd(level=level, gpool=gpool, ph=ph, pw=pw):
            ops.check(lib.nbm_roi_pool_hw_bwd(ptrs, fh, fw, n, C_FPN, rois.data_ptr(), level.data_ptr(), B, R, ph, pw,
                                              gpool.data_ptr(), st), 'nbm_roi_pool_hw_bwd')
        fwd()                                          # `level` for the backward pass
        px = window_pixels(rois_h, ph, pw)
        rows = B * R * ph * pw
        variants['fwd ' + name], variants['bwd ' + name] = fwd, bwd
        info['fwd ' + name] = {'bytes': 4 * C_FPN * (px + 2 * rows)}
        info['bwd ' + name] = {'bytes': 4 * C_FPN * (2 * px + rows)}
    res = alternate(variants, rounds, window_ms)
    for name, s in res.items():
        s.update(info[name])
        s['of_peak'] = round(s['bytes'] / (s['median_us'] * 1e-6) / PEAK, 4)
    return res


def steps_leg(rounds):
    """Eager detect step at B = 64 and one positive training step at B = 128: pool 3 x 3 (dense maps) beside 2 x 2 (on demand)."""
    import numpy as np
    import torch
    from birdsoundclassif_amd import synth
    from birdsoundclassif_amd.nets import build_model
    from birdsoundclassif_amd.train import build_optimizer, default_args, train_one_step
    gen = torch.Generator(device='cuda').manual_seed(1)
    imgs = torch.rand(64, 1, 375, 1024, generator=gen, device='cuda')
    variants, keep = {}, []
    for p in (2, 3):
        model, _ = build_model(default_args(device='cuda', roi_pool_h=p, roi_pool_w=p))
        model.load_state_dict(synth.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}))
        model = model.cuda().eval()
        keep.append(model)
        variants[f'detect step B=64, pool {p}x{p}'] = lambda model=model: model.detect(imgs, 0.3, 0.05, independent=True)
    with torch.no_grad():
        res = alternate(variants, rounds, 400.0)
    del keep, variants
    torch.cuda.empty_cache()
    Bt = 128
    img = torch.from_numpy(np.concatenate([synth.image_batch(0, 8)] * (Bt // 8)))
    bb8, ids8, len8 = synth.label_batch(0, 8)
    bb, ids, lengths = torch.cat([bb8] * (Bt // 8)), torch.cat([ids8] * (Bt // 8)), list(len8) * (Bt // 8)
    for p in (2, 3):
        args = default_args(device='cuda', roi_pool_h=p, roi_pool_w=p)
        model, crit = build_model(args)
        model.load_state_dict(synth.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}))
        model = model.cuda().train()
        crit.train()
        opt, _ = build_optimizer(model, args)
        np.random.seed(7)
        ms = []
        for it in range(2 + max(3, rounds // 2)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            train_one_step(model, crit, opt, [img, img, bb, ids, lengths], args.clip_max_norm, 'cuda', negative_sample=False)
            e1.record()
            torch.cuda.synchronize()
            if it >= 2:
                ms.append(e0.elapsed_time(e1))
        res[f'train step B=128 (positive), pool {p}x{p}'] = {'median_us': round(1e3 * statistics.median(ms), 1), 'min_us': round(1e3 * min(ms), 1),
                                                            'max_us': round(1e3 * max(ms), 1), 'reps': 1}
        del model, crit, opt
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--window_ms', type=float, default=40.0)
    ap.add_argument('--skip_steps', action='store_true')
    ap.add_argument('--out', default=None, help='also write the table to this file')
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'bench_roi_pool.py measures on the GPU; there is nothing to report without one'
    res = {'bench': 'roi_pool', 'rounds': a.rounds, 'window_ms': a.window_ms, 'C': C_FPN, 'peak_bytes_per_s': PEAK}
    with torch.no_grad():
        res['B64_R50'] = pool_leg(64, 50, a.rounds, a.window_ms)
        res['B128_R1000'] = pool_leg(128, 1000, a.rounds, a.window_ms)
    if not a.skip_steps:
        res['steps'] = steps_leg(a.rounds)
    lines = []
    for leg in ('B64_R50', 'B128_R1000', 'steps'):
        if leg in res:
            lines.append(leg)
            for name, s in res[leg].items():
                lines.append(f'  {name:44s} median {s["median_us"]:11.1f} us   min {s["min_us"]:11.1f}   max {s["max_us"]:11.1f}   '
                             f'reps {s["reps"]:5d}' + (f'   bytes {s["bytes"]:13d}   of peak {s["of_peak"]:.3f}' if 'bytes' in s else ''))
    print('\n'.join(lines))
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
