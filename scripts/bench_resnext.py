"""The grouped 3x3 convolution (nbm_gconv3x3, csrc/gconv.hip) at the sizes of the ResNeXt backbones; prints one JSON line.

    python scripts/bench_resnext.py [--batch 64] [--height 375] [--width 1024] [--rounds 5] [--window_ms 60] [--skip_detect]

1. every distinct grouped launch of resnext50_32x4d and resnext101_32x8d (map, channels, group width, stride) on a --batch of
   --height x --width images, with bn2 + ReLU in its epilogue, next to the only thing a user could do without the kernel: the same
   convolution as a dense block-diagonal weight through the existing 3x3 route (the fused Winograd kernel where the ResNet blocks
   use it, the implicit GEMM otherwise).  HIP events around windows of about --window_ms of back-to-back launches after a warm-up,
   --rounds windows per variant, the two variants alternating; median, minimum and maximum per launch.
   hbm_frac = algorithmic bytes (input + output + weights, each once) / median time / 6.3 TB/s (the achievable HBM bandwidth);
   mfma_frac = issued matrix FLOPs (the block-diagonal zeros of Cg < 16 included) / median time / 155 TFLOP/s (the measured rate of
   the fp32 matrix instruction); `bound` names the larger of the two floors.
2. the whole `detect` step of both models on the same batch (filler weights), against resnet50 / resnet101."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.3e12
MFMA_F32_FLOPS = 155e12


def launches(name, H, W):
    """[(label, H, W, C, Cg, stride)] of the distinct grouped launches of a backbone on an H x W image, in network order."""
    from birdsoundclassif_amd.nets import backbone as BB
    layers, groups, base = BB._RESNEXT[name]
    h, w = (H - 1) // 2 + 1, (W - 1) // 2 + 1            # stem
    h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1            # max-pool
    out = []
    for li, (planes, n) in enumerate(zip((64, 128, 256, 512), layers), start=1):
        C = int(planes * base / 64) * groups
        if li > 1:
            out.append((f'layer{li}.0', h, w, C, C // groups, 2))
            h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        if n > (li > 1):
            out.append((f'layer{li}.x', h, w, C, C // groups, 1))
    return out


def timed(fn, rounds, window_ms):
    """-> [ms per call] of `rounds` windows of back-to-back calls (window length chosen from a first timed call)."""
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


def stats(ms):
    return {'median_us': round(1e3 * statistics.median(ms), 1), 'min_us': round(1e3 * min(ms), 1), 'max_us': round(1e3 * max(ms), 1)}


def launch_leg(B, H, W, rounds, window_ms):
    import torch
    from birdsoundclassif_amd import ops
    from birdsoundclassif_amd.nets import _prep, functional as Fn
    rows, seen = [], {}
    for name in ('resnext50_32x4d', 'resnext101_32x8d'):
        for label, h, w, C, Cg, stride in launches(name, H, W):
            key = (h, w, C, Cg, stride)
            if key in seen:
                seen[key]['where'].append(f'{name} {label}')
                continue
            G = C // Cg
            gen = torch.Generator(device='cuda')
            gen.manual_seed(C + Cg + stride)
            x = torch.randn(B, h, w, C, generator=gen, device='cuda')
            wt = torch.randn(C, Cg, 3, 3, generator=gen, device='cuda') * (2.0 / (9 * Cg)) ** 0.5
            scale = 1 + 0.1 * torch.randn(C, generator=gen, device='cuda')
            shift = 0.1 * torch.randn(C, generator=gen, device='cuda')
            dense = torch.zeros(C, C, 3, 3, device='cuda')
            for g in range(G):
                dense[g * Cg:(g + 1) * Cg, g * Cg:(g + 1) * Cg] = wt[g * Cg:(g + 1) * Cg]
            wp = _prep.gconv(wt, G)
            ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
            y = torch.empty(B, ho, wo, C, device='cuda')
            wino = stride == 1 and Fn._winograd_ok(x, dense, 3, 3, 1, 1)

            def grouped():
                ops.gconv3x3(x, wp, G, stride=stride, scale=scale, shift=shift, relu=True, out=y)

            def blockdiag():          # what nets/backbone._Bottleneck runs for its conv2
                if wino:
                    return ops.conv3x3_winograd(x, _prep.wino23(dense), shift, scale=scale, relu=True)
                return Fn.conv(x, dense, scale=scale, shift=shift, kh=3, kw=3, stride=stride, pad=1, act=ops.ACT_RELU)

            with torch.no_grad():
                ref = blockdiag()
                grouped()
                err = float((ref - y).abs().max() / ref.abs().max())
                del ref
                wg, reps_g = timed(grouped, rounds, window_ms)
                wd, reps_d = timed(blockdiag, rounds, window_ms)
                tg, td = [], []
                for _ in range(rounds):                     # alternating: drift of the clock hits both alike
                    tg.append(wg()), td.append(wd())
            nbytes = 4.0 * (x.numel() + y.numel() + wt.numel())
            flops = 2.0 * 9 * Cg * C * B * ho * wo
            issued = flops * max(Cg, 16) / Cg
            med = statistics.median(tg) * 1e-3
            hbm_frac, mfma_frac = nbytes / med / HBM_BYTES_PER_S, issued / med / MFMA_F32_FLOPS
            row = {'where': [f'{name} {label}'], 'map': [h, w], 'C': C, 'Cg': Cg, 'stride': stride, 'MB': round(nbytes / 1e6, 1),
                   'GFLOP': round(flops / 1e9, 2), 'grouped': stats(tg), 'blockdiag': dict(stats(td), route='winograd' if wino else 'igemm'),
                   'speedup': round(statistics.median(td) / statistics.median(tg), 2),
                   'faster_beyond_spread': bool(max(tg) < min(td)), 'hbm_frac': round(hbm_frac, 3), 'mfma_frac': round(mfma_frac, 3),
                   'bound': 'hbm' if nbytes / HBM_BYTES_PER_S > issued / MFMA_F32_FLOPS else 'mfma', 'max_rel_diff': float(f'{err:.2e}'),
                   'reps': [reps_g, reps_d]}
            seen[key] = row
            rows.append(row)
            del x, y, dense, wt, wp
            _prep.clear()
            torch.cuda.empty_cache()
    return rows


def detect_leg(B, H, W, rounds):
    import torch
    from birdsoundclassif_amd import synth
    from birdsoundclassif_amd.nets import build_model
    from birdsoundclassif_amd.train import default_args
    gen = torch.Generator(device='cuda')
    gen.manual_seed(1)
    imgs = torch.rand(B, 1, H, W, generator=gen, device='cuda')
    out = {}
    for name in ('resnet50', 'resnext50_32x4d', 'resnet101', 'resnext101_32x8d'):
        model, _ = build_model(default_args(device='cuda', backbone=name))
        model.load_state_dict(synth.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}))
        model = model.cuda().eval()
        with torch.no_grad():
            window, reps = timed(lambda: model.detect(imgs, 0.3, 0.05, independent=True), rounds, 400.0)
            ms = [window() for _ in range(rounds)]
        out[name] = {'median_ms': round(statistics.median(ms), 2), 'min_ms': round(min(ms), 2), 'max_ms': round(max(ms), 2), 'reps': reps}
        del model
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--height', type=int, default=375)
    ap.add_argument('--width', type=int, default=1024)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--window_ms', type=float, default=60.0)
    ap.add_argument('--skip_detect', action='store_true')
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'bench_resnext.py measures on the GPU; there is nothing to report without one'
    res = {'bench': 'resnext', 'batch': a.batch, 'image': [a.height, a.width], 'rounds': a.rounds,
           'hbm_achievable_TB_per_s': HBM_BYTES_PER_S / 1e12, 'mfma_f32_TFLOP_per_s': MFMA_F32_FLOPS / 1e12,
           'launches': launch_leg(a.batch, a.height, a.width, a.rounds, a.window_ms)}
    if not a.skip_detect:
        res['detect_step'] = detect_leg(a.batch, a.height, a.width, a.rounds)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
