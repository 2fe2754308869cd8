"""The point-wise kernels (csrc/pointwise.hip, csrc/pointwise_bwd.hip) at their edges, through birdsoundclassif_amd.ops, against the
float64 references of tests/pointwise_ref.py.  The cases are data (tests/pointwise_cases.py); tests/test_pointwise_ref_cpu.py proves
on the CPU that each sits on the code path it names (second grid-stride sweeps, register / streaming branches, cached / reloaded
weights, the bilinear backward's two kernels and its list length) and that the hand-written references are right.

Tolerances.  Bit-exact where the operation is a selection, a permutation or a sum the inputs make exact.  An operation with an older
test keeps that test's tolerance (`tol`: atol + rtol |ref| per element, `scaled`: a fraction of max |ref|).  Everything else:
|got - ref64| <= k * 2^-24 * absref per element (`bound`), k = the fp32 roundings on the longest path to one output element, counted
from the kernel source and derived beside each use; absref = the reference on absolute values, so a bound follows cancellation.
Every check prints `RATIO family case error/limit` before it asserts (the largest per family is recorded in
profiles/pointwise_edges.txt); the module writes nothing."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pointwise_cases as K                                      # noqa: E402
import pointwise_ref as R                                        # noqa: E402
from birdsoundclassif_amd import _lib, ops, synth                # noqa: E402
from birdsoundclassif_amd.nets import functional as Fn           # noqa: E402

U, U64 = R.U, R.U64


def rnd(key, *shape, scale=1.0, shift=0.0):
    return torch.from_numpy((synth.normal(key, int(np.prod(shape))) * scale + shift).astype(np.float32).reshape(shape))


def dyadic(key, *shape):
    """Multiples of 1/8 in about +-4: sums of a few of them are exact in fp32, so a gather / scatter of them can be compared bit for bit."""
    return torch.round(rnd(key, *shape) * 8) / 8


def dev(t):
    return t.cuda().contiguous()


def report(family, name, r):
    print(f'RATIO {family} {name} {r:.3g}')
    assert r <= 1.0, f'{family} {name}: error / limit = {r:.3g}'


def bound(family, name, got, ref, absref, k, extra=0.0):
    report(family, name, R.ratio(got, ref, absref, k, extra))


def tol(family, name, got, ref, atol, rtol):
    got, ref = R.t64(got), R.t64(ref)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    ok = bool(torch.isfinite(got).all())
    report(family, name, float(((got - ref).abs() / (atol + rtol * ref.abs())).max()) if ok else float('inf'))


def scaled(family, name, got, ref, frac):
    got, ref = R.t64(got), R.t64(ref)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    ok = bool(torch.isfinite(got).all())
    err = float((got - ref).abs().max())
    report(family, name, (err / (frac * (float(ref.abs().max()) + 1e-12)) if err else 0.0) if ok else float('inf'))


def exact(family, name, got, ref):
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    if got.dtype.is_floating_point:                                # bit for bit: -0.0 != +0.0 here, so compare the words
        same = torch.equal(got.float().contiguous().view(torch.int32), ref.float().contiguous().view(torch.int32))
    else:
        same = torch.equal(got, ref)
    report(family, name, 0.0 if same else float('inf'))


def sid(c):
    return 'x'.join(map(str, c['shape']))


# =========================================================================== bilinear
def bilinear_k(case_path_maxc, Ho, Wo):
    """Backward: a sum of my * mx terms w * g with w = wy * wx: my * mx - 1 adds, 2 products per term, 3 roundings in each of the two
    weights (f - p0, 1 - l, the sum of the two shares at a clamped border): k = my * mx + 7.  Position term: up-sampling, s * o is rounded
    below the magnitude of o: 3 * max(Ho, Wo) (down-sampling adds R.bilinear_position_absref)."""
    my, mx = case_path_maxc
    return my * mx + 7 + 3 * max(Ho, Wo)


@pytest.mark.parametrize('case', K.BILINEAR, ids=sid)
def test_bilinear_forward_and_backward(case):
    Hi, Wi, Ho, Wo, Cc = case['shape']
    B = 2
    src, add, gy = rnd(('bl.s', sid(case)), B, Hi, Wi, Cc), rnd(('bl.a', sid(case)), B, Ho, Wo, Cc), rnd(('bl.g', sid(case)), B, Ho, Wo, Cc)
    identity = (Hi, Wi) == (Ho, Wo)
    down = Ho < Hi or Wo < Wi
    pos_u = 4 * U * max(Hi, Wi)                                    # R.bilinear_position_absref: down-sampling only
    if not down:
        # forward, with and without the added map: the tolerance of test_maxpool_upsample_softmax_silu
        tol('bilinear', f'fwd {sid(case)}', ops.upsample_bilinear_add(dev(src), Ho, Wo), R.bilinear_fwd(src, Ho, Wo)[0], 2e-6, 2e-6)
        tol('bilinear', f'fwd+add {sid(case)}', ops.upsample_bilinear_add(dev(src), Ho, Wo, add=dev(add)), R.bilinear_fwd(src, Ho, Wo, add)[0], 2e-6, 2e-6)
    else:
        # the positions s * o are rounded at the magnitude of the COARSE index here: not the quantity the older test bounds.  Four
        # weights (1 each, 2 on a path), two products and an add inside, one product and one add outside, the added map: k = 8
        pa = pos_u * R.bilinear_position_absref(src, Hi, Wi, Ho, Wo, backward=False)
        bound('bilinear', f'fwd {sid(case)}', ops.upsample_bilinear_add(dev(src), Ho, Wo), *R.bilinear_fwd(src, Ho, Wo), 8, extra=pa)
        bound('bilinear', f'fwd+add {sid(case)}', ops.upsample_bilinear_add(dev(src), Ho, Wo, add=dev(add)), *R.bilinear_fwd(src, Ho, Wo, add), 8, extra=pa)
    # backward through the autograd Function the model uses
    sd, ad = dev(src).requires_grad_(True), dev(add).requires_grad_(True)
    y = Fn.UpsampleAdd.apply(sd, ad, Ho, Wo)
    y.backward(dev(gy))
    ref, absref = R.bilinear_bwd(gy, Hi, Wi)
    extra = pos_u * R.bilinear_position_absref(gy, Hi, Wi, Ho, Wo, backward=True) if down else 0.0
    bound('bilinear_bwd', sid(case), sd.grad, ref, absref, bilinear_k(case['path']['maxc'], Ho, Wo), extra=extra)
    scaled('bilinear_bwd', f'{sid(case)} (5e-6 of test_pointwise_backward)', sd.grad, ref, 5e-6)
    exact('bilinear_bwd', f'add grad {sid(case)}', ad.grad, gy)
    # coarse rows / columns that no fine pixel reads -- at the fp32 positions the kernels compute -- get exactly 0
    rows_ = torch.tensor(R.bilinear_axis_f32(Hi, Ho)[1]) == 0
    cols_ = torch.tensor(R.bilinear_axis_f32(Wi, Wo)[1]) == 0
    assert (bool(rows_.any()), bool(cols_.any())) == ((True, True) if case['path'].get('minc') == (0, 0) else (False, False))
    got = sd.grad.cpu()
    assert bool((got[:, rows_] == 0).all()) and bool((got[:, :, cols_] == 0).all())
    assert bool((got[:, ~rows_][:, :, ~cols_].abs().amax((0, 3)) > 0).all())          # and every other one received something
    if identity:
        exact('bilinear', 'identity fwd', ops.upsample_bilinear_add(dev(src), Ho, Wo), src)
        exact('bilinear_bwd', 'identity bwd', ops.upsample_bilinear_bwd(dev(gy), Hi, Wi), gy)


def test_bilinear_down_and_up_module():
    """SelfAttention(C, C, downscale_factor=4, position_encoding=True) returns inpt + up(down(inpt + 0.5 pe)): its backward runs the general
    kernel with 9 x 9 contributors (the x4 of the `pyramid_top_n_attn == n_levels` pyramid)."""
    from birdsoundclassif_amd.nets.position_encoding import one_dimension_positional_encoding
    from birdsoundclassif_amd.nets.self_attention import SelfAttention
    m = K.MODULE_CASE
    Cc, h, w, f = m['C'], m['h'], m['w'], m['f']
    x, g = rnd('blm.x', 2, h, w, Cc), rnd('blm.g', 2, h, w, Cc)
    mod = SelfAttention(Cc, Cc, downscale_factor=f, position_encoding=True).cuda()
    xd = dev(x).requires_grad_(True)
    out = mod(xd, residual=True)
    out.backward(dev(g))
    pe = 0.5 * one_dimension_positional_encoding(h, Cc).double()[:, None, :].expand(h, w, Cc)
    x64 = x.double()
    small = R.bilinear_fwd(x64 + pe, h // f, w // f)[0]
    small_a = R.bilinear_fwd(x64.abs() + pe.abs(), h // f, w // f)[0]
    ref, ref_a = x64 + R.bilinear_fwd(small, h, w)[0], x64.abs() + R.bilinear_fwd(small_a, h, w)[0]
    pos_u = 4 * U * max(h, w)                                      # the down-sampling's positions: R.bilinear_position_absref
    pos_f = R.bilinear_fwd(pos_u * R.bilinear_position_absref(x64.abs() + pe.abs(), h, w, h // f, w // f, backward=False), h, w)[0]
    # forward: + pe (1), two interpolations (8 each, see the down-sampling cases), the residual add (1); position of the up-sampling 3 x 32
    bound('bilinear', 'module fwd', out, ref, ref_a, 18 + 3 * max(h, w), extra=pos_f)
    # backward: g + down^T(up^T(g)): up^T 9 x 9 + 7, down^T 1 + 7, one add; position 2 x 3 x 32
    gu, gu_a = R.bilinear_bwd(g, h // f, w // f)
    gd, _ = R.bilinear_bwd(gu, h, w)
    gd_a, _ = R.bilinear_bwd(gu_a, h, w)
    my, mx = m['path']['up_maxc']
    pos_b = pos_u * R.bilinear_position_absref(gu_a, h, w, h // f, w // f, backward=True)
    bound('bilinear_bwd', 'module inpt.grad', xd.grad, g.double() + gd, g.double().abs() + gd_a, my * mx + 7 + 8 + 1 + 3 * max(h, w), extra=pos_b)


# =========================================================================== softmax rows
def softmax_case(family, name, x, alpha=1.0):
    """Forward at the tolerance of test_maxpool_upsample_softmax_silu (1e-6 + 1e-5 |ref|), backward at test_pointwise_backward's (5e-6 of max)."""
    p = ops.softmax_rows_(dev(x))
    ref, _ = R.softmax_rows(x)
    tol(family, f'fwd {name}', p, ref, 1e-6, 1e-5)
    gp = rnd(('sm.g', name), *x.shape)
    scaled(family, f'bwd {name}', ops.softmax_rows_bwd(p, dev(gp), alpha), R.softmax_rows_bwd(p, gp, alpha)[0], 5e-6)
    return p


@pytest.mark.parametrize('case', K.SOFTMAX, ids=lambda c: f"{c['rows']}x{c['cols']}")
def test_softmax_rows_edges(case):
    rows, cols = case['rows'], case['cols']
    x = rnd(('sm.x', rows, cols), rows, cols, scale=3.0)
    p = softmax_case('softmax', f'{rows}x{cols}', x, alpha=0.125 if cols == 65 else 1.0)
    assert float((p.double().sum(-1) - 1).abs().max()) < 1e-5


def test_softmax_rows_wide_range_and_partial_inf():
    x = rnd('sm.wide', 5, 200, scale=3.0)
    x[1] = torch.linspace(-80, 80, 200)
    x[3, ::3] = -math.inf
    p = ops.softmax_rows_(dev(x))
    ref, _ = R.softmax_rows(x)
    tol('softmax', 'fwd +-80 and partial -inf', p, ref, 1e-6, 1e-5)
    assert bool((p[3, ::3] == 0).all()) and abs(float(p[3].double().sum()) - 1) < 1e-5 and bool((p[3, 1::3] > 0).all())
    gp = rnd('sm.wide.g', 5, 200)
    scaled('softmax', 'bwd +-80 and partial -inf', ops.softmax_rows_bwd(p, dev(gp)), R.softmax_rows_bwd(p, gp)[0], 5e-6)


def test_softmax_rows_pitched_keeps_the_pad_columns():
    rows, cols, pad = K.SOFTMAX_PITCH['rows'], K.SOFTMAX_PITCH['cols'], K.SOFTMAX_PITCH['pad']
    ld = cols + pad
    host = rnd('sm.pitch', rows, ld, scale=3.0)
    host[:, cols:] = torch.tensor([math.inf, -0.0, 1e-45])[:pad]
    buf = dev(host)
    rc = ops.lib().nbm_softmax_rows(C.c_void_p(buf.data_ptr()), rows, cols, ld, None)
    torch.cuda.synchronize()
    assert rc == 0
    tol('softmax', 'pitched', buf[:, :cols], R.softmax_rows(host[:, :cols])[0], 1e-6, 1e-5)
    exact('softmax', 'pad columns', buf[:, cols:], host[:, cols:])


# =========================================================================== LayerNorm
def ln_ks(E, rows):
    """n = ceil(E / 64) lane adds + 6 butterfly levels.  mean: n + 1 (div); rstd: the squares' sum n, div, + eps, sqrt, reciprocal and half
    of 2 per square: n + 8; xhat = (x - mean) * rstd: (n + 1) + 1 + (n + 8) + 1 = 2n + 11.
    y = xhat * w + b: 2n + 13.  gx = rstd * (g w - c1 - xhat c2), c2 = mean(g w xhat): c2 1 + (2n + 11) + 1 + n + 1 = 3n + 14, xhat c2
    5n + 26, two subtractions, rstd (n + 8) and the product: 6n + 37.  gw = sum over the rows of g * xhat: rows adds in any order (lanes,
    atomics or slots) + 2n + 12 per term; gb: rows."""
    n = (E + 63) // 64 + 6
    return dict(y=2 * n + 13, gx=6 * n + 37, gw=rows + 2 * n + 12, gb=rows)


@pytest.mark.parametrize('rows', K.LAYERNORM_ROWS)
@pytest.mark.parametrize('E', K.LAYERNORM_E)
def test_layernorm_edges(E, rows):
    x, g = rnd(('ln.x', E, rows), rows, E), rnd(('ln.g', E, rows), rows, E)
    w, b = 1 + 0.1 * rnd(('ln.w', E), E), 0.1 * rnd(('ln.b', E), E)
    layernorm_case(f'E{E} rows{rows}', x, w, b, g)


def test_layernorm_large_mean():
    """Rows with mean 1e3 and unit spread: x - mean cancels three digits, which absref follows."""
    rows, E = 37, 200
    layernorm_case('mean 1e3', rnd('ln.big', rows, E, shift=1e3), 1 + 0.1 * rnd('ln.bw', E), 0.1 * rnd('ln.bb', E), rnd('ln.bg', rows, E))


def layernorm_case(name, x, w, b, g):
    rows, E = x.shape
    k = ln_ks(E, rows)
    xd, wd, bd, gd = dev(x), dev(w), dev(b), dev(g)
    ref, ref_a = R.layernorm(x, w, b, 1e-5)
    bound('layernorm', f'y {name}', ops.layernorm(xd, wd, bd, 1e-5), ref, ref_a, k['y'])
    (gx, gx_a), (gw, gw_a), (gb, gb_a) = R.layernorm_bwd(x, w, g, 1e-5)
    a = ops.layernorm_bwd(xd, wd, gd, 1e-5)
    d1 = ops.layernorm_bwd_det(xd, wd, gd, 1e-5)
    d2 = ops.layernorm_bwd_det(xd, wd, gd, 1e-5)
    for tag, got in (('atomic', a), ('det', d1)):
        bound('layernorm_bwd', f'gx {tag} {name}', got[0], gx, gx_a, k['gx'])
        bound('layernorm_bwd', f'gw {tag} {name}', got[1], gw, gw_a, k['gw'])
        bound('layernorm_bwd', f'gb {tag} {name}', got[2], gb, gb_a, k['gb'])
    for i, nm in enumerate(('gx', 'gw', 'gb')):
        exact('layernorm_bwd', f'det repeat {nm} {name}', d2[i], d1[i])
    exact('layernorm_bwd', f'det gx == atomic gx {name}', d1[0], a[0])


def test_layernorm_backward_refuses_more_than_1024_columns():
    E = K.LAYERNORM_REFUSED_E
    x, w, g = dev(rnd('ln.r.x', 3, E)), dev(rnd('ln.r.w', E)), dev(rnd('ln.r.g', 3, E))
    with pytest.raises(_lib.NbmHipError, match='NBM_EINVAL'):
        ops.layernorm_bwd(x, w, g, 1e-5)
    with pytest.raises(_lib.NbmHipError, match='NBM_EINVAL'):
        ops.layernorm_bwd_det(x, w, g, 1e-5)


# =========================================================================== element-wise sweeps beyond one grid
N = K.ELEMENTWISE_N


def plant(t, values, key):
    """Put `values` at seeded positions spread over both grid-stride sweeps (first, last and in between)."""
    n = t.numel()
    pos = [0, n - 1, 4096 * 256 - 1, 4096 * 256] + [int(p * n) for p in synth.uniform(('plant', key), 4 * len(values))]
    flat = t.view(-1)
    for i, p in enumerate(pos):
        flat[p] = values[i % len(values)]
    return pos


def test_silu_sweeps_and_overflow():
    x, gy = rnd('ew.silu.x', N, scale=3.0), rnd('ew.silu.g', N)
    pos = plant(x, [88.0, -88.0, 104.0, -104.0, 1e4, -1e4], 'silu')
    y = ops.silu(dev(x))
    gx = ops.silu_bwd(dev(gy), dev(x))
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(gx).all())
    tol('silu', 'fwd (1e-6 of test_maxpool_upsample_softmax_silu)', y, R.silu(x)[0], 1e-6, 1e-6)
    scaled('silu', 'bwd (2e-6 of test_pointwise_backward)', gx, R.silu_bwd(gy, x)[0], 2e-6)
    tol('silu', 'fwd planted', y.cpu().view(-1)[pos], R.silu(x)[0].view(-1)[pos], 1e-6, 1e-6)
    tol('silu', 'bwd planted', gx.cpu().view(-1)[pos], R.silu_bwd(gy, x)[0].view(-1)[pos], 2e-6, 2e-6)


def test_relu_and_leaky_relu_backward_sweeps_and_zeros():
    y, gy = rnd('ew.relu.y', N), rnd('ew.relu.g', N)
    pos = plant(y, [0.0, -0.0, 1e-45], 'relu')
    got = ops.relu_bwd(dev(gy), dev(y))
    exact('relu_bwd', 'sweep', got, R.relu_bwd(gy, y)[0].float())
    exact('relu_bwd', 'y in {+0, -0, 1e-45}', got.cpu()[pos], torch.where(y[pos] > 0, gy[pos], torch.zeros(len(pos))))
    assert float(y[pos[2]]) > 0 and float(got[pos[2]]) == float(gy[pos[2]])            # the smallest denormal is positive
    sgn = torch.where(gy >= 0, torch.ones(N), -torch.ones(N))
    got = ops.leaky_relu_bwd(dev(sgn), dev(y), 0.01)
    exact('leaky_relu_bwd', 'sweep, gy = +-1', got, R.leaky_relu_bwd(sgn, y, 0.01)[0].float())
    assert set(got.cpu()[pos[:3]].abs().tolist()) <= {1.0, float(np.float32(0.01))}


def test_axpby_film_pair_softmax_init_conv_sweeps():
    e = K.ELEMENTWISE
    a, b = rnd('ew.ax.a', N), rnd('ew.ax.b', e['axpby_period'])
    # alpha * a + beta * b: two products and an add, k = 3
    bound('axpby', 'period 70', ops.axpby(dev(a), dev(b), 0.75, -1.5), *R.axpby(a, b, 0.75, -1.5), 3)
    bound('axpby', 'b = None', ops.axpby(dev(a), None, 0.3), *R.axpby(a, None, 0.3), 1)
    bound('axpby', 'same size', ops.axpby(dev(a), dev(a.flip(0)), 1.0, 1.0), *R.axpby(a, a.flip(0)), 3)
    P_, Cc = e['film_pix'], e['film_C']
    z, film, gy = rnd('ew.fi.z', P_, Cc), rnd('ew.fi.f', P_, 2 * Cc), rnd('ew.fi.g', P_, Cc)
    bound('film', 'fwd', ops.film_fwd(dev(z), dev(film)), *R.film_fwd(z, film), 2)          # a product and an add
    gz, gf = ops.film_bwd(dev(gy), dev(z), dev(film))
    (rz, rza), (rf, rfa) = R.film_bwd(gy, z, film)
    bound('film', 'bwd gz', gz, rz, rza, 1)
    bound('film', 'bwd gfilm', gf, rf, rfa, 1)
    exact('film', 'bwd gbeta', gf[:, Cc:], gy)
    A, ld, px = e['pair_anchor'], e['pair_ld'], e['pair_pix']
    x = rnd('ew.ps.x', px, ld, scale=2.0)
    y = ops.pair_softmax(dev(x), A)
    tol('pair_softmax', 'fwd, x_ld > 2A', y[:, :2 * A], R.pair_softmax(x, A)[0], 1e-6, 1e-6)
    yc, gyc = y[:, :2 * A].contiguous(), rnd('ew.ps.g', px, 2 * A)
    scaled('pair_softmax', 'bwd', ops.pair_softmax_bwd(yc, dev(gyc)), R.pair_softmax_bwd(yc, gyc)[0], 5e-6)
    B, H, W, Cc = e['init_conv']
    xi, wi, bi = rnd('ew.ic.x', B, H, W, 1), rnd('ew.ic.w', Cc), rnd('ew.ic.b', Cc)
    tol('init_conv', 'sweep', ops.init_conv(dev(xi), dev(wi), dev(bi)), R.init_conv(xi, wi, bi)[0], 1e-6, 1e-6)


# =========================================================================== weighted sum
@pytest.mark.parametrize('ncase', K.WEIGHTED_SUM_N, ids=lambda c: str(c['n']))
@pytest.mark.parametrize('raw', K.WEIGHTED_SUM_W, ids=str)
def test_weighted_sum_edges(raw, ncase):
    n = ncase['n']
    xs = [rnd(('ws.x', raw, n, i), n) for i in range(len(raw))]
    g = rnd(('ws.g', raw, n), n)
    wt = torch.tensor(raw, dtype=torch.float32)
    xd = [dev(x) for x in xs]
    # den: 2 adds + the 1e-4 (3); numerator: 3 products + 2 adds (5); the division (1): k = 9
    bound('weighted_sum', f'fwd {raw} n={n}', ops.weighted_sum(xd, dev(wt)), *R.weighted_sum(xs, wt), 9)
    need = [True] * len(raw)
    need[1] = False                                                # one flag off
    gxs, gw = ops.weighted_sum_bwd(xd, dev(wt), dev(g), need)
    rgx, (rgw, rgw_a) = R.weighted_sum_bwd(xs, wt, g)
    assert gxs[1] is None and len(gxs) == len(raw)
    for i in range(len(raw)):
        if need[i]:
            bound('weighted_sum', f'gx{i} {raw} n={n}', gxs[i], rgx[i][0], rgx[i][1], 5)  # den (3), w / den, the product
    full, _ = ops.weighted_sum_bwd(xd, dev(wt), dev(g), [True] * len(raw))
    bound('weighted_sum', f'gx1 {raw} n={n}', full[1], rgx[1][0], rgx[1][1], 5)
    # gw: a thread adds 4 terms per sweep, then 6 butterfly levels, 2 levels over the waves, one atomic per workgroup; a term is
    # g * (x - out) with out at k = 9, the subtraction and the product; the division by den (3 + 1): k = 4 sweeps + 8 + workgroups + 15
    n4 = n // 4
    blocks = min(max((n4 + 255) // 256, 1), 2048)
    k_gw = 4 * ncase['path']['bwd_sweeps'] + 8 + blocks + 15
    bound('weighted_sum', f'gw {raw} n={n}', gw, rgw, rgw_a, k_gw)
    for i, r in enumerate(raw):
        if r <= 0:
            assert float(gw[i]) == 0.0 and math.copysign(1.0, float(gw[i])) == 1.0, (i, float(gw[i]))
    if all(r <= 0 for r in raw):                                   # den = 1e-4, every product is with an exact 0
        assert bool((ops.weighted_sum(xd, dev(wt)) == 0).all()) and all(bool((t == 0).all()) for t in full)


# =========================================================================== column reductions
@pytest.mark.parametrize('M', K.COLSUM_M)
@pytest.mark.parametrize('Nc', K.COLSUM_N)
def test_colsum_edges(M, Nc):
    """Every workgroup sums its rows in double, rounds once to fp32 and adds that with ONE fp32 atomic per column: one rounding per
    workgroup of the column, min(ceil(M / 4), 1024) of them (the first lands on the zeroed output exactly): k = workgroups."""
    ld = Nc + K.COLSUM_PAD
    k = min((M + 3) // 4, 1024)
    g = rnd(('cs.g', M, Nc), M, ld)
    bound('colsum', f'M{M} N{Nc} ld{ld}', ops.colsum(dev(g), Nc), *R.colsum(g, Nc), k)
    big = rnd(('cs.big', M, Nc), M, ld, scale=1e-2, shift=1e4)
    bound('colsum', f'mean 1e4 M{M} N{Nc}', ops.colsum(dev(big), Nc), *R.colsum(big, Nc), k)


@pytest.mark.parametrize('M', K.BN_M)
@pytest.mark.parametrize('Cc', K.BN_C)
@pytest.mark.parametrize('big_mean', [False, True], ids=['randn', 'mean1e3'])
def test_batchnorm_train_edges(M, Cc, big_mean):
    """The sums run in double on the device (double atomics), so the statistics carry the final fp32 rounding only -- plus what the double
    `E[x^2] - mean^2` loses to cancellation, (M + 8) 2^-53 (E[x^2] + mean^2), which the mean-1e3 data makes visible."""
    x = rnd(('bn.x', M, Cc, big_mean), M, Cc, scale=0.1, shift=1e3) if big_mean else rnd(('bn.x', M, Cc), M, Cc, scale=2.0)
    w, b = 1 + 0.1 * rnd(('bn.w', Cc), Cc), 0.1 * rnd(('bn.b', Cc), Cc)
    rm, rv = 0.05 * rnd(('bn.rm', Cc), Cc), 1 + 0.1 * rnd(('bn.rv', Cc), Cc).abs()
    g = rnd(('bn.g', M, Cc), M, Cc)
    name = f'M{M} C{Cc} {"mean 1e3" if big_mean else "randn"}'
    eps, mom = 1e-5, 0.1
    r = R.bn_train_fwd(x, w, b, eps, mom, rm, rv)
    rmd, rvd = dev(rm), dev(rv)
    y, mean, invstd = ops.bn_train_fwd(dev(x), dev(w), dev(b), eps, mom, rmd, rvd)
    var = r['var'][0]
    dvar = (M + 8) * U64 * r['var_cancel']                         # absolute error of the device's double variance
    rel = 0.5 * dvar / (var + float(np.float32(eps)))              # relative error it leaves in invstd
    bound('bn', f'mean {name}', mean, *r['mean'], 1, extra=(M + 8) * U64 * r['mean'][1])
    bound('bn', f'invstd {name}', invstd, *r['invstd'], 1, extra=rel * r['invstd'][0])
    # y = (x - mean) * invstd * w + b: mean (1), the subtraction, invstd (1), two products, the add: k = 6
    xm = (x.double() - r['mean'][0]).abs() * r['invstd'][0] * w.double().abs()
    bound('bn', f'y {name}', y, *r['y'], 6, extra=rel * xm)
    # running statistics: 1 - momentum, the cast of the new value, two products, the add: k = 5
    bound('bn', f'running mean {name}', rmd, *r['run_mean'], 5)
    bound('bn', f'running var {name}', rvd, *r['run_var'], 5, extra=float(np.float32(mom)) * (M / (M - 1) if M > 1 else 1.0) * dvar)
    gx, gw, gb = ops.bn_train_bwd(dev(g), dev(x), mean, invstd, dev(w))
    (rgx, rgx_a), (rgw, rgw_a), (rgb, rgb_a) = R.bn_train_bwd(g, x, mean, invstd, w)
    # xhat 2 (fp32, before the double sum); mean(g xhat) 2 + cast = 3; xhat * that: 6; g - sg - (..): sg (1) + 2; w * invstd, the product: k = 12
    bound('bn', f'gx {name}', gx, rgx, rgx_a, 12, extra=(M + 8) * U64 * rgx_a)
    bound('bn', f'gw {name}', gw, rgw, rgw_a, 3, extra=(M + 8) * U64 * rgw_a)            # xhat (2) + the cast of the double sum
    bound('bn', f'gb {name}', gb, rgb, rgb_a, 1, extra=(M + 8) * U64 * rgb_a)
    if M == 1:                                                      # variance 0: invstd = 1 / sqrt(eps), y = b, gx = 0
        exact('bn', f'y == b {name}', y, b[None])
        assert bool((gx == 0).all())


# =========================================================================== max pooling
def maxpool_case(name, x, residual_mask=((False, False),)):
    B, H, W, Cc = x.shape
    y, idx = ops.maxpool3x3s2(dev(x), with_index=True)
    ry, ridx = R.maxpool(x)
    exact('maxpool', f'y {name}', y, ry.float())
    exact('maxpool', f'y without index {name}', ops.maxpool3x3s2(dev(x)), ry.float())
    exact('maxpool', f'idx {name}', idx, ridx)
    gy = dyadic(('mp.g', name), *ry.shape)
    res, mask = dyadic(('mp.r', name), B, H, W, Cc), rnd(('mp.m', name), B, H, W, Cc)
    for use_res, use_mask in residual_mask:
        rr, mm = (res if use_res else None), (mask if use_mask else None)
        got = ops.maxpool3x3s2_bwd(idx, dev(gy), H, W, residual=dev(rr) if use_res else None, mask=dev(mm) if use_mask else None)
        ref = R.maxpool_bwd(x, gy, rr, mm).float()
        exact('maxpool', f'bwd {name} res={use_res} mask={use_mask}', got + 0.0, ref + 0.0)       # + 0.0: a masked -0.0 is a zero


ALL_RM = ((False, False), (True, False), (False, True), (True, True))


@pytest.mark.parametrize('hw', K.MAXPOOL_SMALL, ids=lambda s: f'{s[0]}x{s[1]}')
def test_maxpool_tiny_maps(hw):
    H, W = hw
    maxpool_case(f'{H}x{W}', rnd(('mp.x', hw), 2, H, W, 4), ALL_RM)
    maxpool_case(f'{H}x{W} ties', torch.round(rnd(('mp.t', hw), 2, H, W, 4)) + 0.0, ALL_RM)       # + 0.0: no -0.0, whose maximum with +0.0 has no defined sign


def test_maxpool_constant_map_gradient_goes_to_the_first_position():
    H, W = 5, 6
    x = torch.full((2, H, W, 4), 0.5)
    maxpool_case('constant', x, ALL_RM)
    _, idx = ops.maxpool3x3s2(dev(x), with_index=True)
    # first in-image position of every window in (r, s) scan order: r = 1 on the top row of windows (row -1 is outside), else 0; s alike
    want = torch.tensor([[(1 if oy == 0 else 0) * 3 + (1 if ox == 0 else 0) for ox in range(3)] for oy in range(3)], dtype=torch.uint8)
    assert torch.equal(idx.cpu(), want[None, :, :, None].expand(2, 3, 3, 4))


def test_maxpool_second_sweep():
    B, H, W, Cc = K.MAXPOOL_BIG['shape']
    maxpool_case('182x182x64', torch.relu(rnd('mp.big', B, H, W, Cc)), ((True, True),))


# =========================================================================== depthwise 3x3
@pytest.mark.parametrize('case', K.DWCONV, ids=lambda c: '-'.join(map(str, c['cfg'])))
def test_dwconv_edges(case):
    """Tolerances of test_dwconv (2e-6 + 2e-6 |ref|), test_dwconv_film_backward (dx 1e-5, dw / db 2e-5 of max) and
    test_dwconv_data_gradient_added_into_a_map (2e-6 of max)."""
    B, H, W, Cin, mult, st = cfg = case['cfg']
    name = '-'.join(map(str, cfg))
    Cout = Cin * mult
    x, w, b = rnd(('dw.x', cfg), B, H, W, Cin), rnd(('dw.w', cfg), Cout, 1, 3, 3, scale=0.3), rnd(('dw.b', cfg), Cout, scale=0.1)
    xd, wd = dev(x), dev(w)
    y = ops.dwconv3x3(xd, wd, dev(b), mult, st)
    tol('dwconv', f'fwd {name}', y, R.dwconv(x, w, b, mult, st)[0], 2e-6, 2e-6)
    tol('dwconv', f'fwd bias=None {name}', ops.dwconv3x3(xd, wd, None, mult, st), R.dwconv(x, w, None, mult, st)[0], 2e-6, 2e-6)
    g = rnd(('dw.g', cfg), *y.shape)
    gd = dev(g)
    rgx, rgw, rgb = R.dwconv_bwd(x, g, w, mult, st)
    has_gx = case['path']['bwd'] is not None
    gx, gw, gb = ops.dwconv3x3_bwd(xd, gd, wd, mult, st, need_gx=has_gx)
    scaled('dwconv_bwd', f'gw {name}', gw, rgw, 2e-5)
    scaled('dwconv_bwd', f'gb {name}', gb, rgb, 2e-5)
    _, gw2, gb2 = ops.dwconv3x3_bwd(xd, gd, wd, mult, st, need_gx=False, has_bias=False)
    assert gb2 is None
    scaled('dwconv_bwd', f'gw without bias {name}', gw2, rgw, 2e-5)
    if not has_gx:
        with pytest.raises(_lib.NbmHipError, match='NBM_EALIGN'):           # no slow path for Cin % 4 != 0: refused, not approximated
            ops.dwconv3x3_bwd(xd, gd, wd, mult, st, need_gx=True, need_gw=False)
        return
    scaled('dwconv_bwd', f'gx {name}', gx, rgx, 1e-5)
    base = rnd(('dw.base', cfg), B, H, W, Cin)
    acc = dev(base).clone()
    ops.dwconv3x3_bwd_acc(gd, wd, mult, st, acc)
    scaled('dwconv_bwd', f'acc {name}', acc, base.double() + rgx, 2e-6)


# =========================================================================== 2x2 average pooling, space to batch
@pytest.mark.parametrize('case', K.AVGPOOL, ids=sid)
def test_avgpool_and_space_to_batch_edges(case):
    B, H, W, Cc = case['shape']
    x = rnd(('ap.x', sid(case)), B, H, W, Cc)
    xd = dev(x)
    exact('avgpool', f'fwd {sid(case)}', ops.avgpool2x2(xd), R.avgpool2x2_f32(x))
    gy = rnd(('ap.g', sid(case)), B, H // 2, W // 2, Cc)
    exact('avgpool', f'bwd {sid(case)}', ops.avgpool2x2_bwd(dev(gy)), R.avgpool2x2_bwd_f32(gy))
    p = ops.space_to_batch2(xd)
    exact('space_to_batch', f'fwd {sid(case)}', p, R.space_to_batch2(x))
    exact('space_to_batch', f'inverse {sid(case)}', ops.space_to_batch2(p, inverse=True), x)
    exact('space_to_batch', f'inverse of a fresh map {sid(case)}', ops.space_to_batch2(dev(R.space_to_batch2(x)), inverse=True), x)


# =========================================================================== optimiser
def sqnorm_case(name, g, init, sweeps_):
    """`out` is a double and the squares are taken in double: a thread's sweeps, 6 butterfly levels, 4 waves, one double atomic per
    workgroup (<= 2048) and the add onto `out`: k = sweeps + 11 + workgroups roundings of 2^-53."""
    out = torch.tensor([init], dtype=torch.float64).cuda()
    ops.sqnorm_accum(dev(g), out)
    ref = init + R.sqnorm(g)
    k = sweeps_ + 11 + min((g.numel() + 255) // 256, 2048)
    r = abs(float(out) - ref) / (k * U64 * ref)
    report('sqnorm', name, r if math.isfinite(float(out)) else float('inf'))
    return float(out)


@pytest.mark.parametrize('ncase', K.SQNORM_N, ids=lambda c: str(c['n']))
def test_sqnorm_accum_edges(ncase):
    n, s = ncase['n'], ncase['path']['sweeps']
    g = rnd(('sq.g', n), n)
    sqnorm_case(f'n={n} onto 0', g, 0.0, s)
    sqnorm_case(f'n={n} onto 3.5', g, 3.5, s)
    tiny = rnd(('sq.tiny', n), n) * 1e-30 + 1e-30                      # fp32 squares would all be 0
    assert sqnorm_case(f'n={n} values 1e-30', tiny, 0.0, s) > 0
    huge = g.clone()
    huge[0] = 1e-30
    huge[n // 2] = 1e19                                            # an fp32 square would be inf
    assert sqnorm_case(f'n={n} with 1e19 and 1e-30', huge, 3.5, s) >= 9.9e37
    huge2 = rnd(('sq.h2', n), n) * 1e19
    sqnorm_case(f'n={n} values 1e19', huge2, 0.0, s)


@pytest.mark.parametrize('step', K.ADAMW_STEPS)
@pytest.mark.parametrize('wd', [1e-2, 0.0])
def test_adamw_step_edges(step, wd):
    n = 100003
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    p, g = rnd(('aw.p', step), n), rnd(('aw.g', step), n, scale=3.0)
    m, v = 0.1 * rnd(('aw.m', step), n), 0.01 * rnd(('aw.v', step), n).abs()
    sqn = R.sqnorm(g)
    norm = math.sqrt(sqn)

    def run(sq, max_norm):
        t = [dev(a).clone() for a in (p, g, m, v)]
        ops.adamw_step(t[0], t[1], t[2], t[3], lr, b1, b2, eps, wd, step,
                       sqnorm=None if sq is None else torch.tensor([sq], dtype=torch.float64).cuda(), max_norm=max_norm)
        return t[0], t[2], t[3]

    def check(name, got, coef, kc):
        (rp, _), (rm_, rm_a), (rv_, rv_a) = R.adamw_step(p, g, m, v, lr, b1, b2, eps, wd, step, coef)
        scaled('adamw', f'p {name} (2e-6 of test_fused_adamw_matches_torch)', got[0], rp, 2e-6)
        # m = beta1 m + (1 - beta1) g coef: coef (kc: sqrt, + 1e-6, the division when it clips), g coef, 1 - beta1, two products, the add
        bound('adamw', f'm {name}', got[1], rm_, rm_a, kc + 5)
        bound('adamw', f'v {name}', got[2], rv_, rv_a, 2 * (kc + 1) + 5)                  # (g coef)^2: twice its error, one more product

    plain = run(None, 0.0)
    check(f'unclipped step={step} wd={wd}', plain, 1.0, 0)
    inactive = run(sqn, 2.0 * norm)                                # norm < max_norm: the coefficient is exactly 1
    for a, b_, nm in zip(inactive, plain, 'pmv'):
        exact('adamw', f'inactive clip == unclipped {nm} step={step} wd={wd}', a, b_)
    check(f'clipped step={step} wd={wd}', run(sqn, 0.5), R.clip_coef(sqn, 0.5), 3)
