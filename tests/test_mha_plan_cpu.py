"""CPU: `ops.mha_plan` (nbm_mha_plan, host only) -- which kernel family an attention launch takes, its LDS, query rows per workgroup
and backward workspace -- and the transformer head's limit of `ops.MHA_SLONG` RoI slots per image in the DETR flavour, refused at
construction by flag name."""
import pytest

from birdsoundclassif_amd import ops
from birdsoundclassif_amd._lib import NbmHipError
from birdsoundclassif_amd.train import default_args

LDS_PER_CU = 160 * 1024


def test_limits():
    assert ops.MHA_SMAX == 128 and ops.MHA_SLONG == 1024


@pytest.mark.parametrize('S,hd,family', [(128, 64, 'narrow'), (1, 1, 'narrow'), (128, 65, 'wide'), (128, 512, 'wide'), (129, 24, 'long'),
                                         (129, 64, 'long'), (129, 512, 'long'), (1024, 512, 'long')])
def test_family_follows_S_then_hd(S, hd, family):
    p = ops.mha_plan(S, hd)
    assert p.family == family
    assert 0 < p.lds_bytes <= LDS_PER_CU and 0 < p.lds_bytes_bwd <= LDS_PER_CU
    assert p.rows == {'narrow': S, 'wide': 32, 'long': 8}[family]
    assert p.row_blocks == -(-S // p.rows)
    assert p.workspace_bytes == 8 * S * S


def test_long_lds_is_score_rows_plus_one_staging_chunk():
    """8 rows of 1 024 scores, 8 rows of a 64-column query chunk, 128 keys of a 64-column chunk padded to 65: two workgroups per CU,
    and the same for every S and hd of the family."""
    want = 4 * (8 * 1024 + 8 * 64 + 128 * 65)
    assert {ops.mha_plan(S, hd).lds_bytes for S in (129, 1024) for hd in (24, 512)} == {want}
    assert LDS_PER_CU // want == 2
    assert ops.mha_plan(128, 64).lds_bytes == 4 * (128 * 65 + 128 * 64 + 4 * 64 + 4 * 128)


@pytest.mark.parametrize('S,hd,N,nhead', [(1025, 64, 1, 1), (129, 513, 1, 1), (0, 64, 1, 1), (129, 64, 0, 1), (129, 64, 1, 0)])
def test_refused_geometries(S, hd, N, nhead):
    with pytest.raises(NbmHipError, match='NBM_EINVAL'):
        ops.mha_plan(S, hd, N, nhead)


def test_workspace_bytes_are_64_bit():
    """S = 1 024 with N * nhead = 1 024: 8 GiB, beyond 32 bits."""
    for S, N, nhead in ((1024, 128, 8), (256, 128, 8), (129, 3, 2), (50, 7, 8)):
        assert ops.mha_plan(S, 64, N, nhead).workspace_bytes == 8 * N * nhead * S * S
    assert ops.mha_plan(1024, 64, 128, 8).workspace_bytes == 1 << 33


TF = dict(device='cpu', tf_rcnn=True, tf_pe_qk=True, tf_num_encoder_layers=1)


@pytest.mark.parametrize('flag', ['post_nms_topN_eval', 'rcnn_batch_size'])
def test_more_than_1024_roi_slots_are_refused_at_construction_by_name(flag):
    from birdsoundclassif_amd.nets import build_model
    with pytest.raises(NotImplementedError, match=rf'--{flag} 1025.*limit|1024.*--{flag} 1025'):
        build_model(default_args(**TF, **{flag: 1025}))
    model, _ = build_model(default_args(**TF, **{flag: 1024}))
    assert model.head.fast_rcnn.rcnn.tf_pe_qk


def test_the_conv_head_and_the_default_flavour_have_no_such_limit():
    """The conv head works per RoI; in the default flavour the RoI slots are batch entries of the attention, not its sequence."""
    from birdsoundclassif_amd.nets import build_model
    build_model(default_args(device='cpu', post_nms_topN_eval=1025, rcnn_batch_size=1025))
    build_model(default_args(device='cpu', tf_rcnn=True, tf_num_encoder_layers=1, post_nms_topN_eval=1025))
