"""CPU checks behind tests/test_gpu_pointwise_edges.py: (1) every hand-written float64 reference of tests/pointwise_ref.py against
torch float64 autograd or an independent formulation, at two small shapes each; (2) every case of tests/pointwise_cases.py sits on
the code path its comment names -- the path is recomputed here with the host-side dispatch arithmetic of csrc/pointwise.hip and
csrc/pointwise_bwd.hip, copied as arithmetic (grid_for, the bilinear dispatch condition, the kernels' own fp32 weights)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pointwise_cases as K
import pointwise_ref as R
from birdsoundclassif_amd import synth

f32 = np.float32


def rnd(key, *shape, scale=1.0):
    return torch.from_numpy((synth.normal(key, int(np.prod(shape))) * scale).astype(np.float32).reshape(shape))


def same(a, b, tol=1e-12):
    a, b = R.t64(a), R.t64(b)
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= tol * (1.0 + float(b.abs().max())), float((a - b).abs().max())


# =========================================================================== (1) the references
@pytest.mark.parametrize('shape', [(3, 4, 7, 9, 2), (1, 5, 8, 10, 3)])
def test_bilinear_references_agree_with_the_dense_operator(shape):
    Hi, Wi, Ho, Wo, C = shape
    src, gy = rnd(('b.s', shape), 2, Hi, Wi, C), rnd(('b.g', shape), 2, Ho, Wo, C)
    My, Mx = torch.from_numpy(R.bilinear_matrix(Hi, Ho)), torch.from_numpy(R.bilinear_matrix(Wi, Wo))
    v, a = R.bilinear_fwd(src, Ho, Wo)
    same(v, torch.einsum('oy,px,byxc->bopc', My, Mx, src.double()))
    same(a, torch.einsum('oy,px,byxc->bopc', My, Mx, src.double().abs()))
    gv, ga = R.bilinear_bwd(gy, Hi, Wi)
    same(gv, torch.einsum('oy,px,bopc->byxc', My, Mx, gy.double()))
    same(ga, torch.einsum('oy,px,bopc->byxc', My, Mx, gy.double().abs()))
    assert bool((ga >= gv.abs() - 1e-15).all())


@pytest.mark.parametrize('shape', [(3, 5), (4, 70)])
def test_softmax_backward_formulas_against_autograd(shape):
    x = rnd(('s.x', shape), *shape, scale=2.0).double().requires_grad_(True)
    g = rnd(('s.g', shape), *shape).double()
    p = x.softmax(-1)
    p.backward(g)
    v, a = R.softmax_rows_bwd(p.detach(), g)
    same(v, x.grad)
    assert bool((a >= v.abs() - 1e-15).all())
    v2, _ = R.softmax_rows_bwd(p.detach(), g, alpha=0.25)
    same(v2, 0.25 * x.grad)
    if shape[1] % 2 == 0:
        xp = rnd(('ps.x', shape), shape[0], shape[1] + 2, scale=2.0).double()
        n = shape[1] // 2
        y, _ = R.pair_softmax(xp, n)
        xr = xp[:, :2 * n].clone().requires_grad_(True)
        xr.view(shape[0], n, 2).softmax(-1).view(shape[0], 2 * n).backward(g)
        same(y, xr.detach().view(shape[0], n, 2).softmax(-1).view(shape[0], 2 * n))
        same(R.pair_softmax_bwd(y, g)[0], xr.grad)


@pytest.mark.parametrize('shape', [(3, 5), (6, 70)])
def test_layernorm_formulas_against_autograd(shape):
    rows, E = shape
    x = (rnd(('l.x', shape), rows, E) + 3.0).double().requires_grad_(True)
    w = (1 + 0.1 * rnd(('l.w', shape), E)).double().requires_grad_(True)
    b = (0.1 * rnd(('l.b', shape), E)).double().requires_grad_(True)
    g = rnd(('l.g', shape), rows, E).double()
    y = F.layer_norm(x, (E,), w, b, 1e-5)
    y.backward(g)
    v, a = R.layernorm(x, w, b, 1e-5)
    same(v, y)
    assert bool((a >= v.abs() - 1e-12).all())
    (gx, gxa), (gw, gwa), (gb, gba) = R.layernorm_bwd(x, w, g, 1e-5)
    same(gx, x.grad, 1e-10), same(gw, w.grad, 1e-10), same(gb, b.grad)
    assert bool((gxa >= gx.abs() - 1e-12).all()) and bool((gwa >= gw.abs() - 1e-12).all()) and bool((gba >= gb.abs()).all())


@pytest.mark.parametrize('n', [7, 40])
def test_elementwise_formulas_against_torch(n):
    x = rnd(('e.x', n), n, scale=3.0).double().requires_grad_(True)
    g = rnd(('e.g', n), n).double()
    y = F.silu(x)
    y.backward(g)
    same(R.silu(x)[0], y), same(R.silu_bwd(g, x)[0], x.grad)
    yy = rnd(('e.y', n), n).double().requires_grad_(True)
    F.leaky_relu(yy, 0.01).backward(g)
    same(R.leaky_relu_bwd(g, F.leaky_relu(yy, 0.01).detach(), 0.01)[0], yy.grad, 1e-8)        # slope enters as the fp32 0.01
    yy.grad = None
    F.relu(yy).backward(g)
    same(R.relu_bwd(g, F.relu(yy).detach())[0], yy.grad)
    C = 3
    z = rnd(('e.z', n), n, C).double().requires_grad_(True)
    fl = rnd(('e.f', n), n, 2 * C).double().requires_grad_(True)
    gz = rnd(('e.gz', n), n, C).double()
    out = z * fl[:, :C] + fl[:, C:]
    out.backward(gz)
    same(R.film_fwd(z, fl)[0], out)
    (a, _), (bb, _) = R.film_bwd(gz, z, fl)
    same(a, z.grad), same(bb, fl.grad)
    av = rnd(('e.a', n), 2 * n).double()
    same(R.axpby(av, g, 0.5, -2.0)[0], 0.5 * av - 2.0 * torch.cat([g, g]))
    same(R.axpby(av, None, 0.5)[0], 0.5 * av)
    xi, wi, bi = rnd(('e.ix', n), 1, n, 2, 1), rnd('e.iw', 3), rnd('e.ib', 3)
    same(R.init_conv(xi, wi, bi)[0].permute(0, 3, 1, 2), F.conv2d(xi.double().permute(0, 3, 1, 2), wi.double().view(3, 1, 1, 1), bi.double()))


@pytest.mark.parametrize('raw', [(0.7, -0.3, 1.1), (0.2, 0.5)])
def test_weighted_sum_formulas_against_autograd(raw):
    xs = [rnd(('w.x', raw, i), 2, 3, 4).double().requires_grad_(True) for i in range(len(raw))]
    w = torch.tensor(raw, dtype=torch.float32).double().requires_grad_(True)
    g = rnd(('w.g', raw), 2, 3, 4).double()
    rw = F.relu(w)
    out = sum(rw[i] * xs[i] for i in range(len(raw))) / (rw.sum() + R.WS_EPS)
    out.backward(g)
    v, a = R.weighted_sum([x.detach() for x in xs], w.detach())
    same(v, out)
    assert bool((a >= v.abs() - 1e-15).all())
    gxs, (gw, gwa) = R.weighted_sum_bwd([x.detach() for x in xs], w.detach(), g)
    for (gx, _), x in zip(gxs, xs):
        same(gx, x.grad)
    same(gw, w.grad)
    assert bool((gwa >= gw.abs() - 1e-15).all())
    assert all(float(gw[i]) == 0.0 for i, r in enumerate(raw) if r <= 0)


@pytest.mark.parametrize('shape', [(5, 3), (2, 70)])
def test_batchnorm_formulas_against_torch(shape):
    M, C = shape
    x = (rnd(('bn.x', shape), M, C) + 2.0).double().requires_grad_(True)
    w = (1 + 0.1 * rnd(('bn.w', shape), C)).double().requires_grad_(True)
    b = (0.1 * rnd(('bn.b', shape), C)).double().requires_grad_(True)
    rm, rv = 0.05 * rnd(('bn.rm', shape), C).double(), 1 + 0.1 * rnd(('bn.rv', shape), C).double().abs()
    rm_t, rv_t = rm.clone(), rv.clone()
    mom, eps = float(f32(0.1)), float(f32(1e-5))
    y = F.batch_norm(x, rm_t, rv_t, w, b, True, mom, eps)
    g = rnd(('bn.g', shape), M, C).double()
    y.backward(g)
    r = R.bn_train_fwd(x, w, b, 1e-5, 0.1, rm, rv)
    same(r['y'][0], y, 1e-10), same(r['run_mean'][0], rm_t), same(r['run_var'][0], rv_t)
    assert bool((r['y'][1] >= r['y'][0].abs() - 1e-12).all())
    (gx, gxa), (gw, _), (gb, _) = R.bn_train_bwd(g, x, r['mean'][0], r['invstd'][0], w)
    same(gx, x.grad, 1e-9), same(gw, w.grad, 1e-9), same(gb, b.grad)
    assert bool((gxa >= gx.abs() - 1e-12).all())
    same(R.colsum(x.detach(), C - 1)[0], x.detach()[:, :C - 1].sum(0))
    # M == 1 (torch refuses): variance 0, unbiased variance = the variance itself, invstd = 1 / sqrt(eps), y = b
    r1 = R.bn_train_fwd(x.detach()[:1], w, b, 1e-5, 0.1, rm, rv)
    same(r1['invstd'][0], torch.full((C,), eps ** -0.5, dtype=torch.float64)), same(r1['y'][0], b.detach()[None])
    same(r1['run_var'][0], (1 - mom) * rv), same(r1['run_mean'][0], (1 - mom) * rm + mom * x.detach()[0])


@pytest.mark.parametrize('shape', [(1, 3, 2, 4), (2, 5, 7, 4)])
def test_maxpool_references(shape):
    B, H, W, C = shape
    x = torch.round(rnd(('mp.x', shape), B, H, W, C) * 2) / 2              # many ties
    y, idx = R.maxpool(x)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert y.shape == (B, Ho, Wo, C) and idx.dtype == torch.uint8
    gy = rnd(('mp.g', shape), B, Ho, Wo, C)
    # independent formulation: scan every window in (r, s) order, strict '>' keeps the first maximum; scatter the gradient there
    gx = torch.zeros(B, H, W, C, dtype=torch.float64)
    for b in range(B):
        for oy in range(Ho):
            for ox in range(Wo):
                for c in range(C):
                    best, where = -np.inf, None
                    for r in range(3):
                        for s in range(3):
                            iy, ix = 2 * oy - 1 + r, 2 * ox - 1 + s
                            if 0 <= iy < H and 0 <= ix < W and float(x[b, iy, ix, c]) > best:
                                best, where = float(x[b, iy, ix, c]), (r, s, iy, ix)
                    assert float(y[b, oy, ox, c]) == best and int(idx[b, oy, ox, c]) == where[0] * 3 + where[1]
                    gx[b, where[2], where[3], c] += float(gy[b, oy, ox, c])
    same(R.maxpool_bwd(x, gy), gx)
    res, mask = rnd(('mp.r', shape), B, H, W, C), rnd(('mp.m', shape), B, H, W, C)
    same(R.maxpool_bwd(x, gy, res, mask), (gx + res.double()) * (mask > 0))


@pytest.mark.parametrize('cfg', [(1, 3, 4, 4, 2, 1), (2, 5, 6, 4, 3, 2)])
def test_dwconv_and_pool_references(cfg):
    B, H, W, Cin, mult, st = cfg
    x, w = rnd(('d.x', cfg), B, H, W, Cin), rnd(('d.w', cfg), Cin * mult, 1, 3, 3)
    b = rnd(('d.b', cfg), Cin * mult)
    v, a = R.dwconv(x, w, b, mult, st)
    # independent formulation: output channel o reads input channel o // mult
    Ho, Wo = (H - 1) // st + 1, (W - 1) // st + 1
    ref = torch.zeros(B, Ho, Wo, Cin * mult, dtype=torch.float64)
    xp = F.pad(x.double(), (0, 0, 1, 1, 1, 1))
    for o in range(Cin * mult):
        for r in range(3):
            for s in range(3):
                ref[..., o] += xp[:, r:r + (Ho - 1) * st + 1:st, s:s + (Wo - 1) * st + 1:st, o // mult] * float(w[o, 0, r, s])
        ref[..., o] += float(b[o])
    same(v, ref)
    assert bool((a >= v.abs() - 1e-12).all())
    g = rnd(('d.g', cfg), B, Ho, Wo, Cin * mult)
    gx, gw, gb = R.dwconv_bwd(x, g, w, mult, st)
    same(gb, g.double().sum((0, 1, 2)))
    assert gx.shape == x.shape and gw.shape == w.shape
    # <grad, perturbation> identity of a linear map: sum(g * conv(dx)) == sum(gx * dx)
    dx = rnd(('d.dx', cfg), B, H, W, Cin)
    same((g.double() * R.dwconv(dx, w, None, mult, st)[0]).sum(), (gx * dx.double()).sum(), 1e-10)
    dw = rnd(('d.dw', cfg), Cin * mult, 1, 3, 3)
    same((g.double() * R.dwconv(x, dw, None, mult, st)[0]).sum(), (gw * dw.double()).sum(), 1e-10)
    # 2x2 average pooling in the kernel's stated order == torch's CPU result, bit for bit; space to batch is a permutation
    t = rnd(('d.ap', cfg), B, 2 * H, 2 * W, 4)
    tr = t.permute(0, 3, 1, 2).clone().requires_grad_(True)
    r = F.adaptive_avg_pool2d(tr, (H, W))
    assert torch.equal(R.avgpool2x2_f32(t), r.detach().permute(0, 2, 3, 1))
    g2 = rnd(('d.apg', cfg), B, H, W, 4)
    r.backward(g2.permute(0, 3, 1, 2))
    assert torch.equal(R.avgpool2x2_bwd_f32(g2), tr.grad.permute(0, 2, 3, 1))
    p = R.space_to_batch2(t)
    assert torch.equal(p[3 * B:4 * B], t[:, 1::2, 1::2]) and torch.equal(p[B:2 * B], t[:, 0::2, 1::2]) and p.shape == (4 * B, H, W, 4)


@pytest.mark.parametrize('step', [1, 7])
def test_adamw_formula_against_torch_optim(step):
    p0 = rnd(('a.p', step), 33).double()
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([ref], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    p, m, v = p0.clone(), torch.zeros(33, dtype=torch.float64), torch.zeros(33, dtype=torch.float64)
    for it in range(1, step + 1):
        g = rnd(('a.g', step, it), 33, scale=3.0).double()
        sqn = R.sqnorm(g)
        assert abs(sqn - float((g * g).sum())) <= 1e-12 * sqn
        coef = R.clip_coef(sqn, 0.5)
        ref.grad = g.clone()
        torch.nn.utils.clip_grad_norm_([ref], 0.5)
        opt.step()
        (p, _), (m, _), (v, _) = R.adamw_step(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 1e-2, it, coef)
    same(p, ref.detach(), 1e-7)           # lr, betas, eps, decay enter the reference as the fp32 values the kernel is handed
    assert R.clip_coef(0.01, 0.5) == 1.0


# =========================================================================== (2) the cases sit on their paths
def grid_for(n, per_block=256, cap=4096):
    g = (n + per_block - 1) // per_block
    return 1 if g < 1 else min(g, cap)


def sweeps(n, per_block=256, cap=4096):
    """Grid-stride iterations of the busiest thread over n items."""
    g = grid_for(n, per_block, cap)
    return (n + g * per_block - 1) // (g * per_block)


def bilinear_axis(n_coarse, n_fine):
    """The host's fp32 scale of one axis and the contributor count of every coarse index under the kernels' fp32 weights."""
    s = f32(n_coarse - 1) / f32(n_fine - 1) if n_fine > 1 else f32(0)
    cnt = [0] * n_coarse
    for o in range(n_fine):
        fy = f32(s * f32(o))
        y0 = int(fy)
        y1 = y0 + (1 if y0 < n_coarse - 1 else 0)
        l = min(max(f32(fy - f32(y0)), f32(0)), f32(1))
        wts = [0.0] * n_coarse
        wts[y0] += float(f32(1) - l)
        wts[y1] += float(l)
        for p in range(n_coarse):
            cnt[p] += wts[p] != 0.0
    return s, cnt


def bilinear_path(Hi, Wi, Ho, Wo, C):
    NF = 5
    sh, ch = bilinear_axis(Hi, Ho)
    sw, cw = bilinear_axis(Wi, Wo)
    fast = sh > 0 and sw > 0 and f32(2) / sh <= f32(NF - 0.05) and f32(2) / sw <= f32(NF - 0.05) and Ho < (1 << 20) and Wo < (1 << 20)
    C4 = C // 4
    return dict(kernel='fast' if fast else 'general', maxc=(max(ch), max(cw)), minc=(min(ch), min(cw)), sh0=bool(sh == 0), sw0=bool(sw == 0),
                two_over_s=float(f32(2) / sh) if sh > 0 else None, share=C4 >= 32, ragged=(Wi * C4) % 256 != 0,
                identity=(Hi, Wi) == (Ho, Wo))


def claimed(path, got):
    for k, v in path.items():
        assert got[k] == v, (k, v, got[k])


@pytest.mark.parametrize('case', K.BILINEAR + [K.TIMED], ids=lambda c: 'x'.join(map(str, c['shape'])))
def test_bilinear_cases_take_the_kernel_they_name(case):
    got = bilinear_path(*case['shape'])
    claimed(case['path'], got)
    Hi, Wi, Ho, Wo, _ = case['shape']
    assert (bilinear_axis(Hi, Ho), bilinear_axis(Wi, Wo)) == (R.bilinear_axis_f32(Hi, Ho), R.bilinear_axis_f32(Wi, Wo))
    # the float64 operator agrees on the contributor counts (a weight the fp32 arithmetic rounds to zero would be a different case)
    assert got['maxc'] == (int((R.bilinear_matrix(Hi, Ho) != 0).sum(0).max()), int((R.bilinear_matrix(Wi, Wo) != 0).sum(0).max()))


def test_bilinear_case_set_covers_the_dispatch():
    paths = [bilinear_path(*c['shape']) for c in K.BILINEAR]
    general = [p for p in paths if p['kernel'] == 'general']
    assert sum(max(p['maxc']) > 6 for p in general) >= 4            # lists longer than the old fixed length
    assert any(max(p['maxc']) == 6 for p in general) and any(p['sh0'] and p['sw0'] for p in general) and any(p['sh0'] != p['sw0'] for p in general)
    assert any(p['kernel'] == 'fast' and p['share'] and p['ragged'] for p in paths) and any(p['kernel'] == 'fast' and not p['share'] and p['ragged'] for p in paths)
    m = K.MODULE_CASE
    down = bilinear_path(m['h'], m['w'], m['h'] // m['f'], m['w'] // m['f'], m['C'])     # backward of the down-sampling: coarse = the full map
    up = bilinear_path(m['h'] // m['f'], m['w'] // m['f'], m['h'], m['w'], m['C'])
    assert (down['kernel'], up['kernel'], up['maxc']) == (m['path']['down'], m['path']['up'], m['path']['up_maxc'])
    assert K.TIMED['path']['maxc'] <= (6, 6)                           # the parent's lists hold every contributor at the timed shape


@pytest.mark.parametrize('case', K.SOFTMAX, ids=lambda c: f"{c['rows']}x{c['cols']}")
def test_softmax_cases(case):
    REG = 24
    rows, cols = case['rows'], case['cols']
    got = dict(branch='reg' if cols <= 64 * REG else 'stream', clamp=cols < 64 * REG, sweeps=sweeps(rows, 4, 256 * 32))
    claimed(case['path'], got)
    assert rows % 4 != 0


def test_softmax_case_set():
    cols = [c['cols'] for c in K.SOFTMAX]
    assert {1, 63, 64, 65, 1536, 1537, 1600, 4099} <= set(cols) and any(c['path']['sweeps'] == 2 for c in K.SOFTMAX)
    assert K.SOFTMAX_PITCH['pad'] > 0 and K.SOFTMAX_PITCH['rows'] % 4 != 0


def test_layernorm_cases():
    for (E, rows), path in K.LAYERNORM_PATH.items():
        assert E in K.LAYERNORM_E and rows in K.LAYERNORM_ROWS
        blocks = grid_for(rows, 4, 256)                                     # both backward entries: at most 256 workgroups of 4 waves
        got = dict(slots=(E + 63) // 64, idle=max(blocks * 4 - rows, 0), sweeps=(rows + blocks * 4 - 1) // (blocks * 4))
        claimed(path, got)
    assert max(K.LAYERNORM_E) == 1024 and K.LAYERNORM_REFUSED_E == 1025       # E > 1024 is refused
    assert any(E < 64 for E in K.LAYERNORM_E) and any(E % 64 for E in K.LAYERNORM_E if E > 64)


def test_elementwise_cases_need_a_second_sweep():
    e = K.ELEMENTWISE
    assert e['n'] > 4096 * 256 and sweeps(e['n']) == 2
    assert e['n'] % e['axpby_period'] == 0 and e['n'] // e['axpby_period'] > 1
    assert sweeps(e['film_pix'] * e['film_C']) == 2
    assert sweeps(e['pair_pix'] * e['pair_anchor']) == 2 and e['pair_ld'] > 2 * e['pair_anchor']
    B, H, W, C = e['init_conv']
    assert sweeps(B * H * W * C) == 2
    for c in K.WEIGHTED_SUM_N:
        assert c['n'] % 4 == 0 and sweeps(c['n'] // 4, 256, 2048) == c['path']['bwd_sweeps']
    for c in K.SQNORM_N:
        assert sweeps(c['n'], 256, 2048) == c['path']['sweeps']
    assert any(all(w <= 0 for w in ws) for ws in K.WEIGHTED_SUM_W) and any(len(ws) == 2 for ws in K.WEIGHTED_SUM_W)


def test_reduction_cases():
    for M, path in K.REDUCE_PATH.items():
        blocks = grid_for(M, 4, 1024)
        claimed(path, dict(sweeps=(M + blocks * 4 - 1) // (blocks * 4), idle_lanes=max(blocks * 4 - M, 0)))
    assert set(K.COLSUM_M) | set(K.BN_M) <= set(K.REDUCE_PATH)
    assert any(n % 64 for n in K.COLSUM_N) and any(n > 128 for n in K.COLSUM_N) and any(c % 64 for c in K.BN_C)
    for (M, C), s in K.BN_APPLY_SWEEPS.items():
        assert sweeps(M * C) == s and M in K.BN_M and C in K.BN_C


def test_maxpool_cases():
    B, H, W, C = K.MAXPOOL_BIG['shape']
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    claimed(K.MAXPOOL_BIG['path'], dict(fwd_sweeps=sweeps(B * Ho * Wo * (C // 4)), bwd_sweeps=sweeps(B * H * W * (C // 4))))
    assert all(min(h, w) <= 3 for h, w in K.MAXPOOL_SMALL)


def dwconv_path(B, H, W, Cin, mult, stride):
    Cout = Cin * mult
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    vec = mult in (1, 2, 4) and Cout % 4 == 0 and Cin % (4 // mult) == 0          # operands from torch are 16-byte aligned
    got = dict(fwd='vec' if vec else 'scalar', wgrad='vec' if vec else 'scalar', out_pixels=B * Ho * Wo)
    if vec:
        items, C4 = B * Ho * Wo * (Cout // 4), Cout // 4
        got.update(fwd_fixed=(grid_for(items) * 256) % C4 == 0, fwd_sweeps=sweeps(items))
    if Cin % 4 == 0:
        C4 = Cin // 4
        gx = min((W * C4 + 255) // 256, 64)
        gy = min(B * H, 65535)
        hoist = mult == 2 and stride <= 2
        got.update(bwd='<2,hoist>' if hoist else '<2>' if mult == 2 else '<4>' if mult == 4 else '<0>',
                   bwd_fixed=hoist and (gx * 256) % C4 == 0, row_sweeps=(B * H + gy - 1) // gy)
    else:
        got.update(bwd=None)
    return got


@pytest.mark.parametrize('case', K.DWCONV, ids=lambda c: '-'.join(map(str, c['cfg'])))
def test_dwconv_cases(case):
    claimed(case['path'], dwconv_path(*case['cfg']))


def test_dwconv_case_set():
    paths = [dwconv_path(*c['cfg']) for c in K.DWCONV]
    assert any(p.get('fwd_fixed') and p.get('fwd_sweeps') == 2 for p in paths) and any(p.get('fwd_fixed') is False for p in paths)
    assert any(p['bwd'] == '<2,hoist>' and not p['bwd_fixed'] for p in paths) and any(p.get('row_sweeps') == 2 and p['bwd_fixed'] for p in paths)
    assert any(min(c['cfg'][1], c['cfg'][2]) == 1 for c in K.DWCONV) and any(p['out_pixels'] == 1 for p in paths)


def test_avgpool_and_optimiser_cases():
    for c in K.AVGPOOL:
        B, H, W, C = c['shape']
        assert H % 2 == 0 and W % 2 == 0 and sweeps(B * H * W * (C // 4)) == c['path']['full_sweeps']
        assert B * H * W * C * 4 < 50e6
    assert K.ADAMW_STEPS == [1, 100000]
