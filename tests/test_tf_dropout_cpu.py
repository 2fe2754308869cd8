"""CPU: the dropout scheme of the transformer head (`--tf_rcnn --dropout p`) -- Philox4x32-10 known answers, the keep mask as a
specification (`ops.dropout_keep_reference`), construction of the head with a non-zero dropout, and the torch restatement of the
head with injected masks (tests/tf_dropout_ref.py) against the oracle."""
import numpy as np
import pytest
import torch

import tf_dropout_ref as R
from birdsoundclassif_amd import ops, synth
from helpers import state_dict_shapes
from oracle import nets_ref as O

SEED = 0x5EEDC0FFEE123457


@pytest.mark.parametrize('counter,key,out', [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox4x32_10_known_answers(counter, key, out):
    assert tuple(int(v) for v in ops.philox4x32_10(counter, key)) == out


def test_keep_reference_is_philox_on_the_documented_counter():
    """Element i = word i & 3 of counter (q & 0xffffffff, q >> 32, site_id, call), q = i >> 2, key = (low, high) half of the seed."""
    seed, call, site, p = SEED, 9, 6, 0.25
    keep = ops.dropout_keep_reference(seed, call, site, 11, p)
    thr, scale = ops.dropout_params(p)
    assert thr == 2 ** 30 and scale == float(np.float32(1) / np.float32(0.75))
    for i in range(11):
        w = ops.philox4x32_10((i >> 2, 0, site, call), (seed & 0xffffffff, seed >> 32))
        assert bool(keep[i]) == (int(w[i & 3]) >= thr)
    big = (1 << 34) + 5                                             # q >= 2^32 moves into counter word 1
    words = ops.philox4x32_10(((big >> 2) & 0xffffffff, big >> 34, site, call), (seed & 0xffffffff, seed >> 32))
    assert words.shape == (4,) and words.dtype == np.uint32


@pytest.mark.parametrize('p', [0.1, 0.5])
def test_keep_reference_share_and_streams(p):
    n = 2 ** 20
    keep = ops.dropout_keep_reference(SEED, 0, 0, n, p)
    assert keep.dtype == np.bool_ and keep.shape == (n,)
    share = float(keep.mean())
    print(f'p = {p}: kept share {share:.6f}, bound {5 * np.sqrt(p * (1 - p) / n):.6f}')
    assert abs(share - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / n)
    assert np.array_equal(keep, ops.dropout_keep_reference(SEED, 0, 0, n, p))
    for other in (ops.dropout_keep_reference(SEED, 0, 1, n, p), ops.dropout_keep_reference(SEED, 1, 0, n, p),
                  ops.dropout_keep_reference(SEED + 1, 0, 0, n, p), ops.dropout_keep_reference(SEED + (1 << 32), 0, 0, n, p)):
        assert not np.array_equal(keep, other)
    assert np.array_equal(keep[:1031], ops.dropout_keep_reference(SEED, 0, 0, 1031, p))      # a prefix is a prefix


def test_keep_reference_p0_keeps_everything():
    assert ops.dropout_keep_reference(SEED, 3, 2, 4099, 0.0).all()


def _head(**kw):
    from birdsoundclassif_amd.nets.layers import Transformer_RCNN
    from birdsoundclassif_amd.train import default_args
    return Transformer_RCNN(default_args(device='cpu', tf_rcnn=True, tf_num_encoder_layers=2, **kw))


@pytest.mark.parametrize('pe_qk', [False, True])
def test_head_builds_with_dropout_and_keeps_its_state_dict(pe_qk):
    drop, plain = _head(tf_pe_qk=pe_qk, dropout=0.1), _head(tf_pe_qk=pe_qk)
    assert drop.dropout_p == pytest.approx(0.1) and plain.dropout_p == 0.0
    assert list(drop.state_dict()) == list(plain.state_dict())
    assert {k: tuple(v.shape) for k, v in drop.state_dict().items()} == {k: tuple(v.shape) for k, v in plain.state_dict().items()}
    drop.set_dropout_stream(SEED, 5)
    assert (drop.dropout_seed, drop.dropout_call) == (SEED, 5)
    assert list(drop.state_dict()) == list(plain.state_dict())         # seed and call are no buffers


@pytest.mark.parametrize('p', [1, -0.1, 1.5])
def test_head_refuses_dropout_outside_0_1(p):
    with pytest.raises(ValueError, match='--dropout'):
        _head(dropout=p)


def test_state_dict_shapes_with_dropout():
    assert state_dict_shapes(tf_rcnn=True, dropout=0.1) == state_dict_shapes(tf_rcnn=True)


def test_conv_head_ignores_dropout():
    """The reference's nn.Dropout lines in RCNN are commented out: `--dropout` without `--tf_rcnn` builds the same model."""
    assert state_dict_shapes(dropout=0.3) == state_dict_shapes()


@pytest.mark.parametrize('pe_qk', [False, True])
def test_restatement_with_all_ones_masks_is_the_oracle(pe_qk):
    """Bound: 5e-5 absolute, that of the oracle's own CPU tests on bbox_reg / bbox_classes (tests/test_oracle_golden.py)."""
    cfg = O.make_cfg(tf_rcnn=True, tf_pe_qk=pe_qk, tf_num_encoder_layers=2)
    pre = 'head.fast_rcnn.rcnn.'
    shapes = {k: v for k, v in state_dict_shapes(tf_rcnn=True, tf_pe_qk=pe_qk, tf_num_encoder_layers=2).items() if k.startswith(pre)}
    sd = synth.fill_state_dict(shapes)
    B, Rr, C = 5, 16, 256
    rnd = lambda key: torch.from_numpy(synth.normal(key, B * Rr * C * 4).astype(np.float32).reshape(B, Rr, C, 2, 2))
    pool, pe = rnd(('dropref-pool', pe_qk)).abs(), rnd(('dropref-pe', pe_qk))
    with torch.no_grad():
        reg, cls = O.transformer_rcnn_forward(sd, cfg, pool, pe)
        for p in (0.0, 0.1):                                         # with all-ones masks p only rescales: p = 0 is the oracle
            got_reg, got_cls = R.head_forward(sd, cfg, pool, pe, R.ones_masks(cfg, B, Rr, 512), p)
            if p == 0.0:
                assert float((got_reg - reg).abs().max()) <= 5e-5 and float((got_cls - cls).abs().max()) <= 5e-5
            else:
                assert float((got_reg - reg).abs().max()) > 1e-3     # the sites are live: 1 / (1 - p) reaches the output
    masks = R.reference_masks(cfg, B, Rr, 512, 0.1, SEED, 0)
    assert set(masks) == {(l, s) for l in range(2) for s in range(4)}
    assert masks[1, 0].shape == ((B, 8, Rr, Rr) if pe_qk else (Rr, 8, B, B)) and masks[0, 2].shape == (B * Rr, 1024)
