"""The gradients of the grouped 3x3 convolution (nbm_gconv3x3_dgrad / nbm_gconv3x3_wgrad, csrc/gconv_bwd.hip) at the sizes of the
ResNeXt backbones; prints one JSON line.

    python scripts/bench_resnext_bwd.py [--batch 64] [--height 375] [--width 1024] [--rounds 5] [--window_ms 60]
                                        [--skip_step] [--step_batch 128] [--step_rounds 3]

1. every distinct grouped launch of resnext50_32x4d and resnext101_32x8d (the 14 of scripts/bench_resnext.py): the data gradient and
   the weight gradient, each with the ReLU mask y and the FrozenBN scale as the training chain passes them, next to the control: the
   same gradients of the dense block-diagonal weight through the routes `Fn.Bottleneck.backward` takes for a ResNet 3x3 -- the
   Winograd F(4x4,3x3) pair where that block uses Winograd (stride 1, >= 128 channels), `ops.conv_dgrad` / `ops.conv_wgrad` otherwise
   (the control gets its gradient already masked, applies no mask of its own and accumulates into a buffer that is zeroed outside
   the timed windows, so it does less than the route does in a training step).  HIP events around windows of about
   --window_ms of back-to-back launches, --rounds windows per variant, grouped and control alternating; median, minimum, maximum.
   hbm_frac = algorithmic bytes (g, y, the other operand, the result; each once) / median time / 6.3 TB/s; mfma_frac = issued matrix
   FLOPs (block-diagonal zeros of Cg < 16 included) / median time / 155 TFLOP/s.
2. the whole training step (train_one_step, --step_batch images, filler weights) of resnext50_32x4d with --lr_backbone 1e-5, next to
   resnet50 and to resnext50_32x4d behind a frozen backbone (--lr_backbone 0)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_resnext import HBM_BYTES_PER_S, MFMA_F32_FLOPS, launches, stats, timed          # noqa: E402


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
            ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
            x = torch.randn(B, h, w, C, generator=gen, device='cuda')
            g = torch.randn(B, ho, wo, C, generator=gen, device='cuda')
            y = torch.randn(B, ho, wo, C, generator=gen, device='cuda')
            wt = torch.randn(C, Cg, 3, 3, generator=gen, device='cuda') * (2.0 / (9 * Cg)) ** 0.5
            scale = 1 + 0.1 * torch.randn(C, generator=gen, device='cuda')
            dense = torch.zeros(C, C, 3, 3, device='cuda')
            for gi in range(G):
                dense[gi * Cg:(gi + 1) * Cg, gi * Cg:(gi + 1) * Cg] = wt[gi * Cg:(gi + 1) * Cg]
            wp = _prep.gconv_dgrad(wt, G, scale)
            gx = torch.empty_like(x)
            dw = torch.empty_like(wt)
            splits, ws_bytes = ops.gconv_wgrad_plan(B, ho, wo, G, Cg, stride)
            wino = stride == 1 and Fn._winograd_ok(x, dense, 3, 3, 1, 1)
            gm = g * (y > 0)                                   # what the control is handed
            kd = _prep.krsc(dense)
            gxd = torch.empty_like(x)
            dwd = torch.zeros_like(kd)
            geom = dict(B=B, H=h, W=w, Cin=C, N=C, kh=3, kw=3, stride=stride, pad=1)
            m = Fn.WINO_BWD_TILE

            def dgrad():
                ops.gconv3x3_dgrad(g, wp, G, h, w, stride=stride, y=y, out=gx)

            def wgrad():
                ops.gconv3x3_wgrad(g, x, G, stride=stride, scale=scale, y=y, out=dw)

            def dgrad_dense():
                if wino:
                    return ops.conv3x3_winograd(gm, _prep.wino23(dense, transposed=True, m=m, scale=scale), None, m=m)
                return ops.conv_dgrad(gm.view(-1, C), kd, gxd, g_ld=C, w_ld=kd.shape[1], a_scale=scale, **geom)

            def wgrad_dense():
                if wino:
                    dU, _ = ops.conv3x3_winograd_wgrad(x, gm, m=m)
                    return _prep.wino23_weight_grad(dU, m, row_scale=scale)
                return ops.conv_wgrad(gm.view(-1, C), x, dwd, row_scale=scale, g_ld=C, out_ld=kd.shape[1], **geom)

            with torch.no_grad():
                ref = dgrad_dense()
                dgrad()
                err_d = float((ref - gx).abs().max() / ref.abs().max())
                dwd.zero_()
                ref = wgrad_dense()
                if not wino:
                    ref = Fn._w_to_ref_layout(ref, dense)
                wgrad()
                blocks = torch.stack([ref[gi * Cg:(gi + 1) * Cg, gi * Cg:(gi + 1) * Cg] for gi in range(G)]).reshape(C, Cg, 3, 3)
                err_w = float((blocks - dw).abs().max() / blocks.abs().max())
                del ref, blocks
                fns = {'dgrad': dgrad, 'dgrad_dense': dgrad_dense, 'wgrad': wgrad, 'wgrad_dense': wgrad_dense}
                win = {k: timed(f, rounds, window_ms) for k, f in fns.items()}
                t = {k: [] for k in fns}
                for _ in range(rounds):                     # alternating: drift of the clock hits all alike
                    for k in fns:
                        t[k].append(win[k][0]())
            flops = 2.0 * 9 * Cg * C * B * ho * wo
            issued = flops * max(Cg, 16) / Cg
            bytes_d = 4.0 * (2 * g.numel() + x.numel() + wt.numel())
            bytes_w = 4.0 * (2 * g.numel() + x.numel() + wt.numel()) + 2.0 * ws_bytes
            row = {'where': [f'{name} {label}'], 'map': [h, w], 'C': C, 'Cg': Cg, 'stride': stride, 'GFLOP': round(flops / 1e9, 2),
                   'route': 'winograd4' if wino else 'igemm', 'splits': splits, 'workspace_MB': round(ws_bytes / 1e6, 1)}
            for kind, nbytes in (('dgrad', bytes_d), ('wgrad', bytes_w)):
                med = statistics.median(t[kind]) * 1e-3
                row[kind] = dict(stats(t[kind]), dense=stats(t[kind + '_dense']), MB=round(nbytes / 1e6, 1),
                                 speedup=round(statistics.median(t[kind + '_dense']) / statistics.median(t[kind]), 2),
                                 faster_beyond_spread=bool(max(t[kind]) < min(t[kind + '_dense'])),
                                 hbm_frac=round(nbytes / med / HBM_BYTES_PER_S, 3), mfma_frac=round(issued / med / MFMA_F32_FLOPS, 3))
            row['max_rel_diff'] = [float(f'{err_d:.2e}'), float(f'{err_w:.2e}')]
            seen[key] = row
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            del x, g, y, gm, dense, kd, gxd, dwd, gx, wt, wp
            _prep.clear()
            torch.cuda.empty_cache()
    return rows


def step_leg(B, rounds, steps=3, warmup=4):
    import numpy as np
    import torch
    from birdsoundclassif_amd import synth
    from birdsoundclassif_amd.nets import build_model
    from birdsoundclassif_amd.train import build_optimizer, default_args, train_one_step
    img = torch.from_numpy(synth.image_batch(0, B)).cuda()
    neg = torch.from_numpy(synth.image_batch(100000, B)).cuda()
    bb, ids, lens = synth.label_batch(0, B)
    data = [img, neg, bb, ids, list(lens)]
    out = {}
    for label, name, lr in (('resnet50', 'resnet50', 1e-5), ('resnext50_32x4d', 'resnext50_32x4d', 1e-5),
                            ('resnext50_32x4d frozen', 'resnext50_32x4d', 0.0)):
        args = default_args(device='cuda', backbone=name, lr_backbone=lr)
        model, crit = build_model(args)
        model.load_state_dict(synth.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}))
        model = model.cuda().train()
        crit.train()
        opt, _ = build_optimizer(model, args)
        np.random.seed(1000)
        for _ in range(warmup):
            train_one_step(model, crit, opt, data, args.clip_max_norm, 'cuda', negative_sample=False)
        ms = []
        for _ in range(rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                train_one_step(model, crit, opt, data, args.clip_max_norm, 'cuda', negative_sample=False)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / steps)
        out[label] = {'median_ms': round(statistics.median(ms), 1), 'min_ms': round(min(ms), 1), 'max_ms': round(max(ms), 1),
                      'steps_per_window': steps}
        print(json.dumps({label: out[label]}), file=sys.stderr, flush=True)
        del model, crit, opt
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--height', type=int, default=375)
    ap.add_argument('--width', type=int, default=1024)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--window_ms', type=float, default=60.0)
    ap.add_argument('--skip_step', action='store_true')
    ap.add_argument('--step_batch', type=int, default=128)
    ap.add_argument('--step_rounds', type=int, default=3)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'bench_resnext_bwd.py measures on the GPU; there is nothing to report without one'
    res = {'bench': 'resnext_bwd', 'batch': a.batch, 'image': [a.height, a.width], 'rounds': a.rounds,
           'hbm_achievable_TB_per_s': HBM_BYTES_PER_S / 1e12, 'mfma_f32_TFLOP_per_s': MFMA_F32_FLOPS / 1e12,
           'launches': launch_leg(a.batch, a.height, a.width, a.rounds, a.window_ms)}
    if not a.skip_step:
        res['train_step'] = dict(step_leg(a.step_batch, a.step_rounds), batch=a.step_batch)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
