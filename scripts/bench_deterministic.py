"""Per-kernel cost of the deterministic twins against their default kernels at shapes of the B = 128 training step:
`python scripts/bench_deterministic.py [B]`.  Each op runs 3 warm-up and 10 timed launches per mode, the modes alternating; prints the
median and the min-max of both and the ratio.  (The whole step in both modes: scripts/trainbench.py B N --deterministic.)"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from birdsoundclassif_amd import ops  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 128
dev = 'cuda'


def timed(fn, reps=10, warm=3):
    out = {False: [], True: []}
    for it in range(warm + reps):
        for mode in (False, True):
            with ops.set_deterministic(mode):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                if it >= warm:
                    out[mode].append(a.elapsed_time(b))
    return out


def show(name, t):
    d, t_ = np.array(t[False]), np.array(t[True])
    print(f'{name:58s} default {np.median(d):8.3f} ms [{d.min():.3f}-{d.max():.3f}]   twin {np.median(t_):8.3f} ms [{t_.min():.3f}-{t_.max():.3f}]'
          f'   x{np.median(t_) / np.median(d):.2f}', flush=True)


def r(*shape):
    return torch.randn(shape, device=dev)


def wgrad(name, H, W, Cin, N, k=1, stride=1, pad=0, bias=False):
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    g, x = r(B, Ho, Wo, N), r(B, H, W, Cin)
    out = torch.zeros((N, k * k * Cin), device=dev)
    bg = torch.zeros((N,), device=dev) if bias else None
    show(f'conv_wgrad {name}', timed(lambda: ops.conv_wgrad(g, x, out, B=B, H=H, W=W, Cin=Cin, N=N, kh=k, kw=k, stride=stride, pad=pad,
                                                            bias_grad=bg)))


wgrad('layer1 3x3 64->64 @94x256', 94, 256, 64, 64, 3, 1, 1)
wgrad('layer2 3x3 128->128 @47x128', 47, 128, 128, 128, 3, 1, 1)
wgrad('layer3 1x1 1024->256 @24x64', 24, 64, 1024, 256)
wgrad('layer4 3x3 512->512 @12x32', 12, 32, 512, 512, 3, 1, 1)
wgrad('lateral 1x1 256->384 @94x256 + bias', 94, 256, 256, 384, bias=True)

img, g = r(B, 375, 1024, 1), r(B, 188, 512, 64)
show('stem7x7_wgrad 375x1024', timed(lambda: ops.stem7x7_wgrad(img, g)))
del img, g

x, g = r(B, 24, 64, 384), r(B, 24, 64, 256)
show('conv3x3_winograd_wgrad F(4x4) 384->256 @24x64 + bias', timed(lambda: ops.conv3x3_winograd_wgrad(x, g, want_bias=True, m=4)))
del x, g

fm_hw = [(188, 512), (94, 256), (47, 128), (24, 64), (12, 32)]
R_ = 16
rois = torch.zeros(B, R_, 4)
u = torch.rand(B, R_, 4)
size = 8.0 * 2.0 ** (u[..., 2] * 5.0)
rois[..., 0], rois[..., 1] = (u[..., 0] * (1000 - size).clamp(min=0)).floor(), (u[..., 1] * (370 - size.clamp(max=360)).clamp(min=0)).floor()
rois[..., 2], rois[..., 3] = (rois[..., 0] + size).clamp(max=1023), (rois[..., 1] + size.clamp(max=360)).clamp(max=374)
rois = rois.cuda()
fm = [torch.zeros(B, h, w, 256, device=dev) for h, w in fm_hw]
pe_f, pe_t = torch.zeros(375, 128, device=dev), torch.zeros(1024, 128, device=dev)
_, _, level = ops.roi_pool(fm, rois, torch.full((B,), R_, dtype=torch.int32, device=dev), pe_f, pe_t, 375, 1024)
gp = r(B * R_, 2, 2, 256)
gf = [torch.zeros_like(f) for f in fm]
bases = {i: (gf[i], None) for i in range(5)}                     # pre-zeroed maps handed in: the fills are not part of the kernel's time
show('roi_pool_bwd 16 RoIs / image, C = 256, 5 levels', timed(lambda: ops.roi_pool_bwd(gp, rois, level, [tuple(f.shape) for f in fm], bases=bases)))
del fm, gf, gp

g2 = r(B * 24 * 64, 256)
show('colsum [196608, 256]', timed(lambda: ops.colsum(g2)))
flat = r(44_000_000)
sq = torch.zeros(1, dtype=torch.float64, device=dev)
show('sqnorm_accum 44 M', timed(lambda: ops.sqnorm_accum(flat, sq)))
del flat
x, gg, w = r(B, 24, 64, 256), r(B, 24, 64, 512), r(512, 1, 3, 3)
show('dwconv3x3_bwd weight 256 x2 @24x64', timed(lambda: ops.dwconv3x3_bwd(x, gg, w, 2, 1, need_gx=False)))
xb, gb_, wb = r(B * R_, 1024), r(B * R_, 1024), r(1024)
mean, invstd = torch.zeros(1024, device=dev), torch.ones(1024, device=dev)
show('bn_train_bwd [2048, 1024]', timed(lambda: ops.bn_train_bwd(gb_, xb, mean, invstd, wb)))
