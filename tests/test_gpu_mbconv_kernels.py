"""GPU: the MBConv kernels alone through `ops` (csrc/mbconv.hip): `nbm_dwconv_bn_act` and `nbm_se_gate` against float64 torch CPU
references with bounds derived from the arithmetic, their determinism and batch-independence, and one whole MBConv block of each kind
against the float64 restatement (tests/effnet_ref.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import effnet_ref                                                             # noqa: E402
from birdsoundclassif_amd import _lib, ops, synth                             # noqa: E402
from birdsoundclassif_amd.nets import _prep, backbone as BB                   # noqa: E402

U = 2.0 ** -24          # unit round-off of fp32


def _randn(key, *shape):
    return torch.from_numpy(synth.normal(key, int(np.prod(shape))).astype(np.float32)).reshape(shape)


def _strip():
    return ops.lib().nbm_dwconv_strip_rows()


def _maps(stride):
    """2 x 3: smaller than a 5 x 5 kernel, every tap partly outside; odd and even sizes; 12 x 32: the coarsest level of the default image;
    the last: an OUTPUT one row higher than a workgroup's strip, so the seam between two strips is crossed."""
    return [(2, 3), (7, 9), (13, 21), (12, 32), ((_strip() + 1) * stride - (stride - 1), 5)]


_DW = {}


def _dw_case(k, stride, H, W, C, B=3):
    """Inputs, the kernel's outputs (act none / SiLU with pool partials) and the float64 reference, computed once and left unchanged."""
    key = (k, stride, H, W, C, B)
    if key not in _DW:
        x = _randn(('dw-x', key), B, H, W, C)
        w = _randn(('dw-w', key), C, 1, k, k) * (2.0 / (k * k)) ** 0.5
        sc = 1.0 + 0.3 * _randn(('dw-sc', key), C)
        sh = 0.2 * _randn(('dw-sh', key), C)
        wt = w.reshape(C, k * k).t().contiguous().cuda()
        xg, scg, shg = x.cuda(), sc.cuda(), sh.cuda()
        lin = ops.dwconv_bn_act(xg, wt, k, stride, scale=scg, shift=shg, act=ops.ACT_NONE)
        act, part = ops.dwconv_bn_act(xg, wt, k, stride, scale=scg, shift=shg, act=ops.ACT_SILU, pool=True)
        x64, w64 = x.double().permute(0, 3, 1, 2), w.double()
        conv = lambda a, b_: F.conv2d(a, b_, stride=stride, padding=(k - 1) // 2, groups=C).permute(0, 2, 3, 1)
        pre = conv(x64, w64) * sc.double() + sh.double()
        bound = (k * k + 3) * U * (conv(x64.abs(), w64.abs()) * sc.double().abs() + sh.double().abs())
        torch.cuda.synchronize()
        _DW[key] = dict(xg=xg, wt=wt, scg=scg, shg=shg, lin=lin.cpu(), act=act.cpu(), part=part.cpu(), pre=pre, bound=bound)
    return _DW[key]


@pytest.mark.parametrize('k,stride', [(3, 1), (3, 2), (5, 1), (5, 2)])
def test_dwconv_bn_act_against_float64(k, stride):
    worst, excess_max = 0.0, 0.0
    for H, W in _maps(stride):
        for C in (8, 20, 36):                                    # % 4 but not % 16: the channel chunk's tail
            c = _dw_case(k, stride, H, W, C)
            p = (k - 1) // 2
            assert tuple(c['lin'].shape) == (3, (H + 2 * p - k) // stride + 1, (W + 2 * p - k) // stride + 1, C)
            # act = none: k * k fused multiply-adds and the affine, each rounded once
            err = (c['lin'].double() - c['pre']).abs()
            assert bool((err <= c['bound']).all()), (k, stride, H, W, C, float((err / c['bound']).max()))
            worst = max(worst, float((err / c['bound']).max()))
            # SiLU: against float64 SiLU of the float64 pre-activation.  |silu'| <= 1.1 carries the pre-activation's error over; what the
            # activation itself adds is measured on existing code: ops.silu on the same pre-activations (rounded to fp32)
            ref = c['pre'] * torch.sigmoid(c['pre'])
            excess = float((ops.silu(c['pre'].float().cuda()).cpu().double() - ref).abs().max())
            excess_max = max(excess_max, excess)
            err = (c['act'].double() - ref).abs()
            assert bool((err <= 1.1 * c['bound'] + excess).all()), (k, stride, H, W, C, float(err.max()), excess)
            # pool partials: the slots summed against the float64 sum of the output the kernel wrote
            y = c['act'].double()
            Ho, Wo = y.shape[1:3]
            assert c['part'].shape[1] == ops.dwconv_pool_slots(C, Ho, Wo)
            perr = (c['part'].double().sum(1) - y.sum((1, 2))).abs()
            assert bool((perr <= Ho * Wo * U * y.abs().sum((1, 2))).all()), (k, stride, H, W, C)
    print(f'k={k} stride={stride}: worst |err| / bound (act none) = {worst:.3f}; ops.silu excess on the pre-activations = {excess_max:.3e}')


@pytest.mark.parametrize('k,stride', [(3, 1), (3, 2), (5, 1), (5, 2)])
def test_dwconv_bn_act_is_deterministic_and_batch_independent(k, stride):
    for H, W in _maps(stride)[2:]:
        c = _dw_case(k, stride, H, W, 20)
        a2, p2 = ops.dwconv_bn_act(c['xg'], c['wt'], k, stride, scale=c['scg'], shift=c['shg'], act=ops.ACT_SILU, pool=True)
        assert torch.equal(a2.cpu(), c['act']) and torch.equal(p2.cpu(), c['part'])                      # two runs, equal bits
        a1, p1 = ops.dwconv_bn_act(c['xg'][:1].contiguous(), c['wt'], k, stride, scale=c['scg'], shift=c['shg'], act=ops.ACT_SILU, pool=True)
        assert torch.equal(a1.cpu()[0], c['act'][0]) and torch.equal(p1.cpu()[0], c['part'][0])          # image 0 alone = image 0 of three


def test_dwconv_bits_do_not_depend_on_the_strip():
    """Rows below a strip seam equal the same rows computed as the top of a map that starts there (stride 1, 3 x 3: output row r of the
    lower map reads input rows r - 1 .. r + 1; away from its own top border those are the same values in the same (r, s) order)."""
    s = _strip()
    x = _randn('dw-seam', 1, s + 6, 9, 8).cuda()
    wt = _randn('dw-seam-w', 9, 8).cuda()
    full = ops.dwconv_bn_act(x, wt, 3, 1)
    low = ops.dwconv_bn_act(x[:, s - 2:].contiguous(), wt, 3, 1)
    assert torch.equal(full[:, s - 1:s + 5], low[:, 1:7])


def test_dwconv_refuses_what_it_does_not_implement():
    x = torch.zeros(1, 5, 5, 6, device='cuda')
    with pytest.raises(_lib.NbmHipError, match='UNSUPPORTED'):
        ops.dwconv_bn_act(x, torch.zeros(9, 6, device='cuda'), 3, 1)                         # C % 4 != 0
    x = torch.zeros(1, 9, 9, 8, device='cuda')
    with pytest.raises(_lib.NbmHipError, match='UNSUPPORTED'):
        ops.dwconv_bn_act(x, torch.zeros(49, 8, device='cuda'), 7, 1)
    with pytest.raises(_lib.NbmHipError, match='UNSUPPORTED'):
        ops.dwconv_bn_act(x, torch.zeros(9, 8, device='cuda'), 3, 3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.dwconv_bn_act(x.cpu(), torch.zeros(9, 8), 3, 1)


@pytest.mark.parametrize('C,Csq,N', [(8, 2, 24), (96, 4, 24), (144, 6, 40)])
def test_se_gate_and_folded_project_weights(C, Csq, N):
    B, slots, hw = 3, 5, 35
    part = (_randn(('se-part', C), B, slots, C).abs() * torch.tensor([0.5, 2.0, 7.0]).view(B, 1, 1)).contiguous()     # three different maps
    w1, b1 = _randn(('se-w1', C), Csq, C) * (2.0 / C) ** 0.5, 0.1 * _randn(('se-b1', C), Csq)
    w2, b2 = _randn(('se-w2', C), C, Csq) * (2.0 / Csq) ** 0.5, 0.5 * _randn(('se-b2', C), C)
    wp_ld = (C + 31) // 32 * 32
    wp = torch.zeros(N, wp_ld)
    wp[:, :C] = _randn(('se-wp', C), N, C)
    w_ld = (C + 31) // 32 * 32
    out = torch.full((B, N, w_ld), float('nan'), device='cuda')                       # unwritten pad would show
    g = [t.cuda() for t in (part, w1, b1, w2, b2, wp)]
    gate, wb = ops.se_gate(g[0], hw, g[1], g[2], g[3], g[4], wproj=g[5], out=out)
    assert wb.data_ptr() == out.data_ptr()
    gate_only = ops.se_gate(g[0], hw, g[1], g[2], g[3], g[4])
    assert torch.equal(gate_only, gate)
    gate, wb = gate.cpu().double(), wb.cpu().double()
    # float64 reference and a running bound on each stage's error
    d = lambda t: t.double()
    mean = d(part).sum(1) / hw
    e_mean = (slots + 1) * U * d(part).abs().sum(1) / hw
    zs = mean @ d(w1).t() + d(b1)
    e_zs = (C + 2) * U * (mean.abs() @ d(w1).abs().t() + d(b1).abs()) + e_mean @ d(w1).abs().t()
    s = zs * torch.sigmoid(zs)
    e_s = 1.1 * e_zs + 8 * U * s.abs() + 1e-30
    z = s @ d(w2).t() + d(b2)
    e_z = (Csq + 2) * U * (s.abs() @ d(w2).abs().t() + d(b2).abs()) + e_s @ d(w2).abs().t()
    ref = torch.sigmoid(z)
    e_gate = 0.25 * e_z + 8 * U
    assert bool(((gate - ref).abs() <= e_gate).all()), float(((gate - ref).abs() / e_gate).max())
    assert float((ref[0] - ref[2]).abs().max()) > 0.05                                 # the gates differ per image
    ref_wb = d(wp)[None, :, :C] * ref[:, None, :]
    e_wb = d(wp)[None, :, :C].abs() * e_gate[:, None, :] + U * ref_wb.abs()
    assert bool(((wb[:, :, :C] - ref_wb).abs() <= e_wb).all())
    assert bool((wb[:, :, C:] == 0).all()) and not torch.isnan(wb).any()               # the pad columns are written, as zeros
    print(f'C={C} Csq={Csq}: worst gate |err| / bound = {float(((gate - ref).abs() / e_gate).max()):.3f}')


# (ratio, k, stride, in, out): no expand convolution; stride 2 with 5 x 5; the residual
@pytest.mark.parametrize('kind,cfg', [('no-expand', (1, 3, 1, 32, 16)), ('stride2-5x5', (6, 5, 2, 24, 40)), ('residual', (6, 3, 1, 24, 24))])
def test_one_mbconv_block_against_the_float64_restatement(kind, cfg):
    t, k, s, cin, cout = cfg
    blk = BB._MBConv(t, k, s, cin, cout, BB.FrozenBatchNorm2d)
    p = 'backbone.0.body.3.0.'
    sd = synth.fill_state_dict({p + n: tuple(v.shape) for n, v in blk.state_dict().items()})
    sd = {n[len('backbone.0.'):]: v for n, v in sd.items()}
    blk.load_state_dict({n[len('body.3.0.'):]: v for n, v in sd.items()})
    x = _randn(('mbconv-x', kind), 2, cin, 13, 21)
    with torch.no_grad():
        got = blk.cuda().eval()(x.permute(0, 2, 3, 1).contiguous().cuda()).permute(0, 3, 1, 2).cpu().double()
        ref = effnet_ref.mbconv(x.double(), sd, 'body.3.0', t, k, s, cin, cout)
    assert got.shape == ref.shape
    e = float((got - ref).abs().max() / ref.abs().max())
    print(f'{kind}: relative error {e:.3e}, output max {float(ref.abs().max()):.3g}, std {float(ref.std()):.3g}')
    # Four chained stages (expand, depthwise, gate, project) whose longest dot product has K = 144 terms: the worst-case bound K * 2^-24
    # of one stage is 8.6e-6 of its absolute sum, a typical error sqrt(K) * 2^-24 = 7e-7.  2^-16 = 1.5e-5 allows the worst case of the
    # longest stage plus the others; an indexing, stride or gate-mapping error is of order 1, a bf16-level loss 2^-9.
    assert float(ref.std()) > 0.05 and e <= 2.0 ** -16
