"""GPU: `ops.set_deterministic(True)` (train.py --deterministic) -- two optimiser steps at B = 2 from the same weights, data and
seed, run twice on freshly built models: every loss value, every parameter and both AdamW moment buffers must come out bit-identical, for
four configurations.  For the default configuration also: the gradients of a step in deterministic mode agree with the default mode's within
the bound the suite already uses for re-ordered fp32 sums, and torch's own deterministic-algorithms state is restored when the mode is
switched off."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from birdsoundclassif_amd import ops, synth                                   # noqa: E402
from helpers import filler_state_dict                                         # noqa: E402

CONFIGS = {
    'default': dict(),
    'tf_rcnn-dropout': dict(tf_rcnn=True, dropout=0.1),
    'bifpn': dict(fpn='bifpn'),
    'resnext50-batchnorm': dict(backbone='resnext50_32x4d', norm_layer_backbone='batchnorm'),
}


_BUILT = []


@pytest.fixture(autouse=True)
def _leave_nothing_behind():
    """These tests build ten models with their optimisers, about 1.6 GiB each: `FusedAdamW.release()` gives their memory back, or it would
    still be allocated when a later test of the session measures its peak memory (tests/test_gpu_fullsize.py)."""
    import gc
    from birdsoundclassif_amd.nets import _prep
    yield
    for _, opt in _BUILT:
        opt.release()
    _BUILT.clear()
    _prep.clear()                                           # prepared (transformed) copies of those weights
    gc.collect()
    torch.cuda.empty_cache()


def _build(cfg):
    from birdsoundclassif_amd.nets import build_model
    from birdsoundclassif_amd.train import build_optimizer, default_args, seed_everything
    seed_everything(42)
    args = default_args(device='cuda', **cfg)
    model, crit = build_model(args)
    model.load_state_dict(filler_state_dict(**cfg))
    model = model.cuda().train()
    crit.train()
    opt, _ = build_optimizer(model, args)
    _BUILT.append((model, opt))
    return args, model, crit, opt


def _batch():
    img = torch.from_numpy(synth.image_batch(0, 2))
    boxes, ids, lengths = synth.label_batch(0, 2)
    return [img, img, boxes, ids, lengths]


def _run(cfg, steps=2):
    """-> (loss values per step, parameters, AdamW moments) after `steps` optimiser steps of a freshly built model."""
    from birdsoundclassif_amd.train import train_one_step
    args, model, crit, opt = _build(cfg)
    batch = _batch()
    np.random.seed(7)
    losses = []
    for _ in range(steps):
        loss = train_one_step(model, crit, opt, batch, args.clip_max_norm, 'cuda', negative_sample=False)
        losses.append({k: float(v.detach() if torch.is_tensor(v) else v) for k, v in loss.items()})
    torch.cuda.synchronize()
    params = {n: p.detach().clone() for n, p in model.named_parameters()}
    moments = {}
    for n, p in model.named_parameters():
        st = opt.state.get(p, {})
        for k in ('exp_avg', 'exp_avg_sq'):
            if k in st:
                moments[f'{n}.{k}'] = st[k].detach().clone()
    return losses, params, moments


@pytest.mark.parametrize('name', list(CONFIGS))
def test_two_runs_of_two_steps_are_bit_identical(name):
    cfg = CONFIGS[name]
    with ops.set_deterministic(True):
        a = _run(cfg)
        b = _run(cfg)
    assert not ops.deterministic()
    assert a[0] == b[0], (a[0], b[0])                       # every loss value of every step, as floats: equal means the same bits
    assert all(np.isfinite(v) for step in a[0] for v in step.values())
    assert a[1].keys() == b[1].keys() and a[2].keys() == b[2].keys() and len(a[2]) > 0
    differing = [n for n in a[1] if not torch.equal(a[1][n], b[1][n])] + [n for n in a[2] if not torch.equal(a[2][n], b[2][n])]
    assert not differing, (len(differing), differing[:8])


def test_default_configuration_gradients_agree_with_the_default_mode_and_torch_state_is_restored():
    from birdsoundclassif_amd.nets import functional as Fn
    from birdsoundclassif_amd.train import step

    def grads(det):
        args, model, crit, opt = _build({})
        opt.zero_grad()
        np.random.seed(7)
        with ops.set_deterministic(det):
            assert ops.deterministic() == det and (not det or torch.are_deterministic_algorithms_enabled())
            loss = step(model, crit, _batch(), 'cuda', False)
            sum(loss[k] * crit.weight_dict[k] for k in loss if k in crit.weight_dict).backward()
            Fn.parked_flush()
            Fn.stash_check_empty()
        torch.cuda.synchronize()
        return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}

    before = torch.are_deterministic_algorithms_enabled()
    g_det = grads(True)
    assert torch.are_deterministic_algorithms_enabled() == before
    g_def = grads(False)
    assert g_det.keys() == g_def.keys() and len(g_def) > 100
    module_scale = {}
    for n, g in g_def.items():
        m = n.rsplit('.', 1)[0]
        module_scale[m] = max(module_scale.get(m, 0.0), float(g.abs().max()))
    worst = 0.0
    for n, g in g_det.items():
        assert bool(torch.isfinite(g).all()), n
        # the same sums in another order: 2^-12 of the largest gradient of the tensor's module, the bound of
        # tests/test_gpu_efficientnet_train.py:88-97 for two backward passes whose atomics add in a free order
        scale = module_scale[n.rsplit('.', 1)[0]]
        d = float((g - g_def[n]).abs().max())
        worst = max(worst, d / scale if scale else 0.0)
        assert d <= 2.0 ** -12 * scale, (n, d, scale)
    print(f'worst |g_det - g_default| / max |g_default| over {len(g_det)} tensors: {worst:.3e}')


def test_an_entry_point_without_a_twin_raises_in_deterministic_mode():
    x = torch.zeros((1, 4, 4, 4), device='cuda')
    tiles = torch.full((128,), -1, device='cuda', dtype=torch.int32)
    compact = torch.zeros((512, 4), device='cuda')
    with ops.set_deterministic(True):
        with pytest.raises(RuntimeError, match='not reproducible under --deterministic'):
            ops.upsample_bilinear_bwd(x, 2, 2, tiles_share=[(compact, tiles, 0, 1)])
