"""CPU: the oracle restatement beside the REAL reference on inputs the other golden files do not contain.  What the
reference computed is stored in tests/golden/reference_checks.npz (oracle/make_golden.py --reference-checks-only, which
imports the reference with the torchvision stand-in)."""
import builtins
import warnings

import numpy as np
import pytest
import torch

from birdsoundclassif_amd import synth
from helpers import check_packed, dets_to_rows, load_golden, state_dict_shapes
from oracle import nets_ref as O


def test_eval_forward_other_seed():
    warnings.filterwarnings('ignore')
    g = load_golden('reference_checks.npz')
    sd = synth.fill_state_dict(state_dict_shapes(), seed=5)
    cfg = O.make_cfg()
    x = torch.from_numpy(synth.image_batch(7, 1))[:, None]
    with torch.no_grad():
        oo = O.forward_first_stage(sd, cfg, x)
        for i, q in enumerate(oo['fpn_out']):
            check_packed(g, f'seed5.fpn{i}', q, atol=5e-5)
        check_packed(g, 'seed5.rois', oo['rois'], atol=0.0)
        od = O.forward(sd, cfg, x, min_score=0.05)
    # the same boxes in the same classes and order (scores are not compared)
    ref, got = g['seed5.dets_min0.05'], dets_to_rows(od)
    assert got.shape == ref.shape
    assert np.array_equal(got[:, :6], ref[:, :6])


def test_anchors_match_reference():
    from birdsoundclassif_amd.nets.util import nets_utils as mine
    g = load_golden('reference_checks.npz')
    cfg = O.make_cfg()
    ref = g['anchors.base']
    assert np.array_equal(ref, O.base_anchors(cfg)) and np.array_equal(ref, mine.generate_anchors_frcnn(16, [0.5, 1, 2], 2 ** np.arange(5)))
    sh = g['anchors.shifts']
    assert np.array_equal(sh, mine.get_anchor_shifts_frcnn(64, 24, 16))
    assert np.array_equal((ref + sh).reshape(-1, 4), O.all_anchors(cfg))


def test_learned_position_embedding_cannot_run_in_the_reference():
    """`--position_embedding learned` (position_encoding.py:59-83): the reference's Joiner evaluates the embedding for every
    pyramid level (backbone.py:139-148) and the module indexes nn.Embedding(50, .) with arange(w) -- the narrowest level of a
    375 x 1024 input is 32 columns wide, the next 64: its forward pass fails in the reference itself (with the exception
    stored in the fixture), so the build raises the same."""
    warnings.filterwarnings('ignore')
    err = str(load_golden('reference_checks.npz')['learned_pe.error'])
    assert err == 'IndexError'
    from birdsoundclassif_amd.nets import build_model
    from birdsoundclassif_amd.train import default_args
    with pytest.raises(getattr(builtins, err)):
        build_model(default_args(device='cpu', position_embedding='learned'))
