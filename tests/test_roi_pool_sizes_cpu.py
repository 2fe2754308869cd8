"""CPU: RoI pooling sizes other than 2 x 2 (`--roi_pool_h` / `--roi_pool_w`) -- the host-side plan and its two refusals, the
shapes a non-default pool gives the head, the dense-FPN route it selects, and the oracle's `roi_pooling` beside the real
reference's `ROIPooling.forward` at those sizes (skipped where the reference is not installed)."""
import warnings
from types import SimpleNamespace

import pytest
import torch

from birdsoundclassif_amd import ops
import detect_ref as D
from helpers import state_dict_shapes
from oracle import nets_ref as O
from oracle import ref_import

SIZES = [(3, 4), (7, 7), (12, 32), (2, 5)]
C_ROI = 16


def test_plan_picks_the_kernels_and_refuses_what_the_reference_cannot_run():
    assert ops.roi_pool_plan(2, 2, D.FMAP_HW) == 'ondemand'
    for ph, pw in SIZES + [(5, 2), (2, 3), (3, 2)]:
        assert ops.roi_pool_plan(ph, pw, D.FMAP_HW) == 'dense', (ph, pw)
    assert ops.roi_pool_plan(24, 64, [(188, 512), (24, 64)]) == 'dense'          # `--dilation`: the coarsest map is 24 x 64
    for ph, pw in [(1, 2), (2, 1), (0, 2), (1, 1), (-3, 4)]:
        with pytest.raises(ValueError, match=r'--roi_pool_h.*--roi_pool_w.*positional-encoding slice.*empty'):
            ops.roi_pool_plan(ph, pw, D.FMAP_HW)
    for ph, pw in [(13, 2), (2, 33), (13, 33), (188, 512)]:
        with pytest.raises(ValueError, match=r'--roi_pool_h.*--roi_pool_w.*growth loop.*does not terminate'):
            ops.roi_pool_plan(ph, pw, D.FMAP_HW)


def test_head_shapes_follow_the_pool_size():
    s = state_dict_shapes(roi_pool_h=3, roi_pool_w=4)
    assert s['head.fast_rcnn.rcnn.bbox_reg_layer.weight'] == (604, 3072)
    assert s['head.fast_rcnn.rcnn.bbox_classif_layer.weight'] == (151, 3072)
    t = state_dict_shapes(roi_pool_h=3, roi_pool_w=4, tf_rcnn=True)
    assert t['head.fast_rcnn.rcnn.pos_embedding.0.weight'] == (512, 3072)
    assert t['head.fast_rcnn.rcnn.rois_embedding.0.weight'] == (512, 3072)


def test_a_non_default_pool_selects_the_dense_fpn_route():
    from birdsoundclassif_amd.nets import build_model
    from birdsoundclassif_amd.train import default_args
    model, _ = build_model(default_args(device='cpu'))
    assert model._lazy_strides() == {0: 8, 1: 4}
    model.args.roi_pool_h, model.args.roi_pool_w = 3, 4
    assert model._lazy_strides() is None
    model.args.roi_pool_h, model.args.roi_pool_w = 2, 3
    assert model._lazy_strides() is None
    model.args.roi_pool_h, model.args.roi_pool_w = 2, 2
    assert model._lazy_strides() == {0: 8, 1: 4}


@pytest.fixture(scope='module')
def edge_inputs():
    rois = torch.cat([D.boundary_rois(), D.edge_rois().expand(3, -1, -1)], 1).contiguous()
    return rois, D.integer_fmaps(3, C_ROI), D.modular_fmaps(3, C_ROI)


@pytest.mark.skipif(not ref_import.available(), reason='the reference is not installed')
@pytest.mark.parametrize('ph,pw', SIZES)
def test_oracle_pooling_equals_the_reference_at_other_pool_sizes(edge_inputs, ph, pw):
    """The reference's own ROIPooling.forward on the level-boundary and edge RoIs: `pool` and `level` equal; `pe` within 2e-4
    (the reference sums the encoding in float32, the oracle in float64: 1.3e-4 measured, the same noise exists at 2 x 2)."""
    warnings.filterwarnings('ignore')
    ref_import.import_nets()
    from nbm_model.nets.layers import ROIPooling
    rois, ints, mods = edge_inputs
    cfg = O.make_cfg(roi_pool_h=ph, roi_pool_w=pw, out_fpn_chan=C_ROI)
    ref = ROIPooling(SimpleNamespace(n_layers=5, device='cpu', roi_pool_h=ph, roi_pool_w=pw, img_height=D.IMG_H,
                                     img_width=D.IMG_W, out_fpn_chan=C_ROI))
    with torch.no_grad():
        for name, fmaps in (('integer', ints), ('modular', mods)):
            r_pool, r_pe, r_lvl = ref(rois, fmaps)
            o_pool, o_pe, o_lvl = O.roi_pooling(cfg, rois, fmaps)
            assert torch.equal(torch.as_tensor(r_lvl).long(), o_lvl), name
            assert bool(torch.isfinite(r_pool).all()) and bool(torch.isfinite(r_pe).all()), name
            assert torch.equal(r_pool, o_pool), name
            err = float((r_pe - o_pe).abs().max())
            print(f'{ph}x{pw} {name}: pe max difference {err:.3e}')
            assert err <= 2e-4, (name, err)
