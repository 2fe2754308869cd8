"""Live BatchNorm in the backbone (`--norm_layer_backbone batchnorm`, csrc/bnorm.hip); writes profiles/bn_backbone.txt and prints one
JSON line.

    python scripts/bench_bn_backbone.py [--batch 64] [--height 375] [--width 1024] [--rounds 5] [--window_ms 60]
                                        [--step_batches 128,64] [--steps 3] [--skip_step] [--out profiles/bn_backbone.txt]

(a) every distinct (M, C, relu, residual) of resnet50's 53 norms on a --batch of --height x --width images: `ops.bn_act_train_fwd` /
    `ops.bn_act_train_bwd` against a CONTROL built from the kernels that existed before them -- forward: `ops.bn_train_fwd`, then the add
    (`ops.axpby`), then the ReLU (there is no forward ReLU kernel: `ops.relu_bwd(t, t)` = t * (t > 0), the same pass with its operand read
    twice); backward: `ops.relu_bwd`, then `ops.bn_train_bwd`.  HIP events around windows of about --window_ms of back-to-back calls
    after a warm-up, --rounds windows per variant, the variants alternating in one process; median, minimum and maximum per call.
    hbm_frac = algorithmic bytes / median time / 6.3 TB/s: forward 2 reads of z + 1 write of y (+ 1 read of the residual); backward
    2 reads each of gy, z (and y with ReLU) + 1 write of gz (+ 1 write of gres).
(b) one whole training step (`train_one_step`, --lr_backbone 1e-5) of resnet50 with `batchnorm` against `frozen_batchnorm` at the
    largest of --step_batches that fits, the two alternating; peak allocated memory of each.
(c) the losses of a default (`frozen_batchnorm`) --lr_backbone 1e-5 step at B = 2, printed with all digits: to be compared with the same
    line of the parent commit (the frozen path must run the launches it ran before)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from bench_resnext import HBM_BYTES_PER_S, stats, timed          # noqa: E402


def norm_shapes(B, H, W, layers=(3, 4, 6, 3)):
    """{(M, C, relu, residual): [where]} of the 53 norms of a ResNet-50 body on B images of H x W, in network order."""
    out = {}
    add = lambda h, w, c, relu, res, where: out.setdefault((B * h * w, c, relu, res), []).append(where)
    h, w = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    add(h, w, 64, True, False, 'bn1')
    h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    for li, (planes, n) in enumerate(zip((64, 128, 256, 512), layers), start=1):
        for bi in range(n):
            st = 2 if (bi == 0 and li > 1) else 1
            ho, wo = (h - 1) // st + 1, (w - 1) // st + 1
            add(h, w, planes, True, False, f'layer{li}.{bi}.bn1')
            add(ho, wo, planes, True, False, f'layer{li}.{bi}.bn2')
            if bi == 0:
                add(ho, wo, 4 * planes, False, False, f'layer{li}.{bi}.downsample.1')
            add(ho, wo, 4 * planes, True, True, f'layer{li}.{bi}.bn3')
            h, w = ho, wo
    return out


def kernel_leg(B, H, W, rounds, window_ms):
    import torch
    from birdsoundclassif_amd import ops
    rows = []
    gen = torch.Generator(device='cuda')
    gen.manual_seed(11)
    for (M, C, relu, res), where in norm_shapes(B, H, W).items():
        z = torch.randn(M, C, generator=gen, device='cuda') * 1.5 + 0.3
        r = torch.randn(M, C, generator=gen, device='cuda') if res else None
        gy = torch.randn(M, C, generator=gen, device='cuda')
        gamma = 1 + 0.1 * torch.randn(C, generator=gen, device='cuda')
        beta = 0.1 * torch.randn(C, generator=gen, device='cuda')
        rm, rv = torch.zeros(C, device='cuda'), torch.ones(C, device='cuda')
        y, mean, invstd = ops.bn_act_train_fwd(z, gamma, beta, 1e-5, 0.1, rm, rv, residual=r, relu=relu)

        def fwd_new():
            ops.bn_act_train_fwd(z, gamma, beta, 1e-5, 0.1, rm, rv, residual=r, relu=relu)

        def fwd_ctl():
            t, _, _ = ops.bn_train_fwd(z, gamma, beta, 1e-5, 0.1, rm, rv)
            if res:
                t = ops.axpby(t, r)
            if relu:
                ops.relu_bwd(t, t)

        def bwd_new():
            ops.bn_act_train_bwd(gy, y if relu else None, z, mean, invstd, gamma, relu=relu, want_gres=relu and res)

        def bwd_ctl():
            g = ops.relu_bwd(gy, y) if relu else gy
            ops.bn_train_bwd(g, z, mean, invstd, gamma)

        # results must agree before a time means anything
        t0, _, _ = ops.bn_train_fwd(z, gamma, beta, 1e-5, 0.1, rm, rv)
        t0 = t0 + r if res else t0
        t0 = t0.clamp_min(0) if relu else t0
        d_fwd = float((y - t0).abs().max())
        g0 = ops.bn_train_bwd(ops.relu_bwd(gy, y) if relu else gy, z, mean, invstd, gamma)
        g1 = ops.bn_act_train_bwd(gy, y if relu else None, z, mean, invstd, gamma, relu=relu)
        d_bwd = float((g1[0] - g0[0]).abs().max())
        del t0, g0, g1
        windows = [timed(f, rounds, window_ms)[0] for f in (fwd_new, fwd_ctl, bwd_new, bwd_ctl)]
        ts = [[] for _ in windows]
        for _ in range(rounds):
            for t, wnd in zip(ts, windows):
                t.append(wnd())
        n = M * C * 4
        fwd_bytes = n * (3 + (1 if res else 0))
        bwd_bytes = n * ((6 if relu else 4) + 1 + (1 if (relu and res) else 0))
        row = {'M': M, 'C': C, 'relu': relu, 'residual': res, 'norms': len(where), 'first': where[0], 'parts': ops.bn_act_plan(M, C)[0],
               'max_abs_diff_fwd': d_fwd, 'max_abs_diff_gz': d_bwd}
        for tag, t, nbytes in (('fwd_new', ts[0], fwd_bytes), ('fwd_control', ts[1], fwd_bytes), ('bwd_new', ts[2], bwd_bytes),
                               ('bwd_control', ts[3], bwd_bytes)):
            row[tag] = dict(stats(t), hbm_frac=round(nbytes / (statistics.median(t) * 1e-3) / HBM_BYTES_PER_S, 3))
        row['fwd_speedup'] = round(row['fwd_control']['median_us'] / row['fwd_new']['median_us'], 2)
        row['bwd_speedup'] = round(row['bwd_control']['median_us'] / row['bwd_new']['median_us'], 2)
        rows.append(row)
        del z, r, gy, y
        torch.cuda.empty_cache()
    return rows


def _trainer(norm, B):
    import numpy as np
    import torch
    from birdsoundclassif_amd import synth
    from birdsoundclassif_amd.nets import build_model
    from birdsoundclassif_amd.train import build_optimizer, default_args, train_one_step
    args = default_args(device='cuda', norm_layer_backbone=norm, lr_backbone=1e-5)
    model, crit = build_model(args)
    model.load_state_dict(synth.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}))
    model = model.cuda().train()
    crit.train()
    opt, _ = build_optimizer(model, args)
    img = torch.from_numpy(synth.image_batch(0, B)).cuda()
    bb, ids, lens = synth.label_batch(0, B)
    data = [img, img, bb, ids, list(lens)]
    np.random.seed(1000)
    return lambda: train_one_step(model, crit, opt, data, args.clip_max_norm, 'cuda', negative_sample=False)


def step_leg(batches, steps):
    import time
    import torch
    for B in batches:
        try:
            out = {'batch': B}
            runs = {}
            for norm in ('frozen_batchnorm', 'batchnorm'):
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                step = _trainer(norm, B)
                for _ in range(4):
                    loss = step()
                torch.cuda.synchronize()
                runs[norm] = step
                out[norm] = {'peak_allocated_GiB': round(torch.cuda.max_memory_allocated() / 2 ** 30, 1),
                             'losses': {k: float(v.detach() if torch.is_tensor(v) else v) for k, v in loss.items()}, 'ms_per_step': []}
            for _ in range(3):                      # alternating rounds of `steps` steps
                for norm, step in runs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(steps):
                        step()
                    torch.cuda.synchronize()
                    out[norm]['ms_per_step'].append(round((time.perf_counter() - t0) / steps * 1e3, 1))
            return out
        except torch.OutOfMemoryError as e:
            print(f'B = {B} does not fit: {str(e)[:120]}', file=sys.stderr, flush=True)
            runs = step = None
            torch.cuda.empty_cache()
    return {'batch': None}


def default_step_losses():
    """The losses of one default step at B = 2 (tests' data), every digit."""
    import numpy as np
    import torch
    from birdsoundclassif_amd import synth
    from birdsoundclassif_amd.nets import build_model
    from birdsoundclassif_amd.train import build_optimizer, default_args, train_one_step
    args = default_args(device='cuda', lr_backbone=1e-5)
    model, crit = build_model(args)
    model.load_state_dict(synth.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}))
    model = model.cuda().train()
    crit.train()
    opt, _ = build_optimizer(model, args)
    img = torch.from_numpy(synth.image_batch(0, 2))
    bb, ids, lens = synth.label_batch(0, 2)
    np.random.seed(7)
    loss = train_one_step(model, crit, opt, [img, img, bb, ids, lens], args.clip_max_norm, 'cuda', negative_sample=False)
    torch.cuda.synchronize()
    return {k: repr(float(v.detach() if torch.is_tensor(v) else v)) for k, v in loss.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--height', type=int, default=375)
    ap.add_argument('--width', type=int, default=1024)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--window_ms', type=float, default=60.0)
    ap.add_argument('--step_batches', default='128,64')
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--skip_step', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bn_backbone.txt'))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'needs a GPU: there is no CPU path to time'
    res = {'device': torch.cuda.get_device_name(0), 'batch': a.batch, 'image': [a.height, a.width]}
    res['default_step_losses_B2'] = default_step_losses()
    res['kernels'] = kernel_leg(a.batch, a.height, a.width, a.rounds, a.window_ms)
    if not a.skip_step:
        res['train_step'] = step_leg([int(b) for b in a.step_batches.split(',')], a.steps)
    lines = [f'# scripts/bench_bn_backbone.py --batch {a.batch} --height {a.height} --width {a.width} --rounds {a.rounds} '
             f'--window_ms {a.window_ms}  ({res["device"]})', '',
             '(a) BatchNorm (+ residual) (+ ReLU) per distinct shape of resnet50; us per call: median [min .. max]; hbm = algorithmic bytes / '
             'median / 6.3 TB/s', '',
             f'{"M":>10} {"C":>5} relu res norms parts | {"fwd new":>24} hbm | {"fwd control":>24} hbm |  x   | {"bwd new":>24} hbm | '
             f'{"bwd control":>24} hbm |  x', '-' * 190]
    cell = lambda r: f'{r["median_us"]:>8.1f} [{r["min_us"]:>6.1f} ..{r["max_us"]:>7.1f}] {r["hbm_frac"]:.2f}'
    for r in res['kernels']:
        lines.append(f'{r["M"]:>10} {r["C"]:>5} {int(r["relu"]):>4} {int(r["residual"]):>3} {r["norms"]:>5} {r["parts"]:>5} | '
                     f'{cell(r["fwd_new"])} | {cell(r["fwd_control"])} | {r["fwd_speedup"]:>4.2f} | {cell(r["bwd_new"])} | '
                     f'{cell(r["bwd_control"])} | {r["bwd_speedup"]:>4.2f}')
    lines += ['', 'largest |new - control| per shape (y; gz): ' +
              '; '.join(f'{r["max_abs_diff_fwd"]:.1e} {r["max_abs_diff_gz"]:.1e}' for r in res['kernels'])]
    if 'train_step' in res:
        t = res['train_step']
        lines += ['', f'(b) one training step of resnet50, --lr_backbone 1e-5, B = {t["batch"]} (three alternating rounds of {a.steps} steps)']
        for norm in ('frozen_batchnorm', 'batchnorm'):
            if norm in t:
                lines.append(f'    {norm:>17}: ms per step {t[norm]["ms_per_step"]}  peak allocated {t[norm]["peak_allocated_GiB"]} GiB  '
                             f'losses {t[norm]["losses"]}')
    lines += ['', '(c) losses of one default (frozen_batchnorm) --lr_backbone 1e-5 step at B = 2:', f'    {res["default_step_losses_B2"]}']
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
