"""The MBConv launches (csrc/mbconv.hip and the GEMMs around them) at the sizes of the EfficientNet backbones; prints one JSON line.

    python scripts/bench_efficientnet.py [--batch 64] [--height 375] [--width 1024] [--rounds 5] [--window_ms 60] [--skip_detect]

1. every distinct depthwise launch of efficientnet_b0 and efficientnet_b4 on a --batch of --height x --width images: the fused kernel
   (`nbm_dwconv_bn_act`: norm + SiLU + pool partials) and, for the 3 x 3 shapes, the control a user had before it: `nbm_dwconv3x3` with the
   norm folded into its weights and bias, then `nbm_silu` as a pass of its own.  HIP events around windows of about --window_ms of
   back-to-back launches after a warm-up, --rounds windows per variant, the variants alternating; median, minimum and maximum per launch.
   hbm_frac = algorithmic bytes (input + output + weights + partials, each once) / median time / 6.3 TB/s (the achievable HBM bandwidth).
2. the squeeze-and-excitation launches (`nbm_se_gate`, with the folded project weights) behind them;
3. the project 1x1 GEMMs on the per-image-weights route (groups = B), next to the same GEMM with ONE weight matrix (no gate: what the
   convolution alone costs), and the expand 1x1 GEMMs by plan path (fast: channels a multiple of 32; general: the gather path);
4. the whole eager `detect` step of efficientnet_b0 and efficientnet_b4 beside resnet50 on the same batch (filler weights)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from bench_resnext import HBM_BYTES_PER_S, stats, timed          # noqa: E402


def blocks(name, H, W):
    """[(label, h, w, cin, cexp, cout, k, stride, residual)] of every MBConv block on an H x W image (h, w: the block's input map)."""
    from birdsoundclassif_amd.nets import backbone as BB
    h, w = (H - 1) // 2 + 1, (W - 1) // 2 + 1                    # stem
    out = []
    for si, (t, k, s, cin, cout, n) in enumerate(BB.efficientnet_stages(name), start=1):
        for bi in range(n):
            st, ci = (s, cin) if bi == 0 else (1, cout)
            out.append((f'{si}.{bi}', h, w, ci, BB._make_divisible(ci * t), cout, k, st, st == 1 and ci == cout))
            h, w = (h - 1) // st + 1, (w - 1) // st + 1
    return out


def _alternate(windows, rounds):
    ts = [[] for _ in windows]
    for _ in range(rounds):
        for t, wnd in zip(ts, windows):
            t.append(wnd())
    return ts


def launch_leg(B, H, W, rounds, window_ms):
    import torch
    from birdsoundclassif_amd import ops
    from birdsoundclassif_amd.nets import _prep
    dw_rows, se_rows, proj_rows, exp_rows = [], [], [], []
    seen_dw, seen_proj, seen_exp = {}, {}, {}
    gen = torch.Generator(device='cuda')
    gen.manual_seed(5)
    rnd = lambda *shape: torch.randn(*shape, generator=gen, device='cuda')
    for name in ('efficientnet_b0', 'efficientnet_b4'):
        for label, h, w, cin, cexp, cout, k, stride, res in blocks(name, H, W):
            where = f'{name} {label}'
            # ---- expand 1x1 (+ norm + SiLU)
            if cexp != cin:
                key = (h, w, cin, cexp)
                if key in seen_exp:
                    seen_exp[key]['where'].append(where)
                else:
                    x, wk = rnd(B, h, w, cin), rnd(cexp, (cin + 31) // 32 * 32) * (2.0 / cin) ** 0.5
                    sc, sh = 1 + 0.1 * rnd(cexp), 0.1 * rnd(cexp)
                    y = torch.empty(B, h, w, cexp, device='cuda')
                    wnd, reps = timed(lambda: ops.conv2d(x, wk, scale=sc, shift=sh, act=ops.ACT_SILU, out=y), rounds, window_ms)
                    (t,) = _alternate([wnd], rounds)
                    nbytes = 4.0 * (x.numel() + y.numel() + wk.numel())
                    row = {'where': [where], 'map': [h, w], 'Cin': cin, 'N': cexp, 'path': 'fast' if cin % 32 == 0 else 'general',
                           'MB': round(nbytes / 1e6, 1), **stats(t), 'hbm_frac': round(nbytes / (statistics.median(t) * 1e-3) / HBM_BYTES_PER_S, 3),
                           'reps': reps}
                    seen_exp[key] = row
                    exp_rows.append(row)
                    del x, y
            # ---- depthwise (+ norm + SiLU + pool partials), SE, project
            ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
            key = (h, w, cexp, k, stride)
            if key in seen_dw:
                seen_dw[key]['where'].append(where)
                part = None
            else:
                x = rnd(B, h, w, cexp)
                wt = rnd(cexp, 1, k, k) * (2.0 / (k * k)) ** 0.5
                sc, sh = 1 + 0.1 * rnd(cexp), 0.1 * rnd(cexp)
                taps = _prep.dw_taps(wt)
                y, part = ops.dwconv_bn_act(x, taps, k, stride, scale=sc, shift=sh, act=ops.ACT_SILU, pool=True)
                nbytes = 4.0 * (x.numel() + y.numel() + wt.numel() + part.numel())
                windows = [timed(lambda: ops.dwconv_bn_act(x, taps, k, stride, scale=sc, shift=sh, act=ops.ACT_SILU, pool=True), rounds, window_ms)]
                row = {'where': [where], 'map': [h, w], 'C': cexp, 'k': k, 'stride': stride, 'MB': round(nbytes / 1e6, 1)}
                if k == 3:
                    wf, bf = (wt * sc.view(-1, 1, 1, 1)).contiguous(), sh
                    ctl = ops.silu(ops.dwconv3x3(x, wf, bf, 1, stride))
                    row['max_rel_diff_vs_control'] = float(f'{float((ctl - y).abs().max() / ctl.abs().max()):.2e}')
                    del ctl
                    windows.append(timed(lambda: ops.silu(ops.dwconv3x3(x, wf, bf, 1, stride)), rounds, window_ms))
                ts = _alternate([wnd for wnd, _ in windows], rounds)
                med = statistics.median(ts[0]) * 1e-3
                row.update(fused=stats(ts[0]), hbm_frac=round(nbytes / med / HBM_BYTES_PER_S, 3), reps=[r for _, r in windows])
                if k == 3:
                    row.update(control=stats(ts[1]), speedup=round(statistics.median(ts[1]) / statistics.median(ts[0]), 2),
                               fused_slower_than_control=bool(statistics.median(ts[0]) > statistics.median(ts[1])))
                seen_dw[key] = row
                dw_rows.append(row)
                del x
            key = (ho, wo, cexp, cout, cin, res)
            if key in seen_proj:
                seen_proj[key]['where'].append(where)
                continue
            if part is None:
                y = rnd(B, ho, wo, cexp)
                part = torch.rand(B, ops.dwconv_pool_slots(cexp, ho, wo), cexp, generator=gen, device='cuda')
            csq = max(1, cin // 4)
            w1, b1, w2, b2 = rnd(csq, cexp) * (2.0 / cexp) ** 0.5, 0.02 * rnd(csq), rnd(cexp, csq) * (2.0 / csq) ** 0.5, 1 + 0.5 * rnd(cexp)
            wp = rnd(cout, (cexp + 31) // 32 * 32) * (2.0 / cexp) ** 0.5
            wnd, reps = timed(lambda: ops.se_gate(part, ho * wo, w1, b1, w2, b2, wproj=wp), rounds, window_ms)
            (t,) = _alternate([wnd], rounds)
            _, wb = ops.se_gate(part, ho * wo, w1, b1, w2, b2, wproj=wp)
            nbytes = 4.0 * (part.numel() + wp.numel() + wb.numel() + w1.numel() + w2.numel())
            se_rows.append({'where': [where], 'map': [ho, wo], 'C': cexp, 'Csq': csq, 'N': cout, 'slots': part.shape[1], 'MB': round(nbytes / 1e6, 2),
                            **stats(t), 'hbm_frac': round(nbytes / (statistics.median(t) * 1e-3) / HBM_BYTES_PER_S, 3), 'reps': reps})
            sc, sh = 1 + 0.1 * rnd(cout), 0.1 * rnd(cout)
            r_ = rnd(B, ho, wo, cout) if res else None
            out = torch.empty(B, ho, wo, cout, device='cuda')
            wa, ra = timed(lambda: ops.conv1x1_per_image(y, wb, cout, scale=sc, shift=sh, residual=r_), rounds, window_ms)
            wc, rc = timed(lambda: ops.conv2d(y, wp, scale=sc, shift=sh, residual=r_, out=out), rounds, window_ms)
            ta, tc = _alternate([wa, wc], rounds)
            nbytes = 4.0 * (y.numel() + out.numel() * (2 if res else 1) + wb.numel())
            row = {'where': [where], 'map': [ho, wo], 'Cin': cexp, 'N': cout, 'residual': bool(res), 'route': 'per_image_weights',
                   'path': 'fast' if cexp % 32 == 0 else 'general', 'MB': round(nbytes / 1e6, 1), 'per_image': stats(ta),
                   'one_weight_matrix_no_gate': stats(tc), 'hbm_frac': round(nbytes / (statistics.median(ta) * 1e-3) / HBM_BYTES_PER_S, 3),
                   'wb_over_map_bytes': round(wb.numel() / y.numel(), 3), 'reps': [ra, rc]}
            seen_proj[key] = row
            proj_rows.append(row)
            del y, part, wb, out, r_
            _prep.clear()
            torch.cuda.empty_cache()
    return {'depthwise': dw_rows, 'se_gate': se_rows, 'project': proj_rows, 'expand': exp_rows}


def detect_leg(B, H, W, rounds):
    import torch
    from birdsoundclassif_amd import synth
    from birdsoundclassif_amd.nets import backbone as BB, build_model
    from birdsoundclassif_amd.train import default_args
    gen = torch.Generator(device='cuda')
    gen.manual_seed(1)
    imgs = torch.rand(B, 1, H, W, generator=gen, device='cuda')
    models, out = {}, {}
    for name in ('resnet50', 'efficientnet_b0', 'efficientnet_b4'):
        kw = {'lr_backbone': 0.0} if name in BB._EFFICIENTNET else {}
        model, _ = build_model(default_args(device='cuda', backbone=name, **kw))
        model.load_state_dict(synth.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}))
        models[name] = model.cuda().eval()
    with torch.no_grad():
        windows = {n: timed(lambda m=m: m.detect(imgs, 0.3, 0.05, independent=True), rounds, 400.0) for n, m in models.items()}
        ts = _alternate([wnd for wnd, _ in windows.values()], rounds)          # the three models alternating
    for (n, (_, reps)), ms in zip(windows.items(), ts):
        out[n] = {'median_ms': round(statistics.median(ms), 2), 'min_ms': round(min(ms), 2), 'max_ms': round(max(ms), 2), 'reps': reps}
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
    assert torch.cuda.is_available(), 'bench_efficientnet.py measures on the GPU; there is nothing to report without one'
    res = {'bench': 'efficientnet', 'batch': a.batch, 'image': [a.height, a.width], 'rounds': a.rounds,
           'hbm_achievable_TB_per_s': HBM_BYTES_PER_S / 1e12, **launch_leg(a.batch, a.height, a.width, a.rounds, a.window_ms)}
    if not a.skip_detect:
        res['detect_step'] = detect_leg(a.batch, a.height, a.width, a.rounds)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
