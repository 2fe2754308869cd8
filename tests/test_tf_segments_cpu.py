"""CPU: the geometry nbm_mha_segments must realise -- the token -> group maps of tf_segments_ref, built from the segment table
and the per-image counts, against an enumeration of the per-segment model calls, for ragged tables."""
import numpy as np
import pytest

from birdsoundclassif_amd import ops
from tf_segments_ref import ACROSS_IMAGES, ACROSS_ROIS, attention_f64, image_counts, table_of, token_groups, token_groups_per_call

CASES = [([1] * 8, [50, 0, 37, 1, 50, 12, 3, 49]), ([4, 4, 3, 1, 2], [37, 0, 50, 5, 1]), ([64], [41]), ([128], [50]),
         ([3, 1, 1, 7, 2], [0, 50, 0, 2, 60])]


@pytest.mark.parametrize('sizes,counts', CASES)
@pytest.mark.parametrize('mode', [ACROSS_ROIS, ACROSS_IMAGES])
def test_token_groups_equal_the_per_call_enumeration(sizes, counts, mode):
    R = 50
    table = table_of(sizes)
    assert np.array_equal(table, ops.segment_table(sizes, 'cpu').numpy())
    got = token_groups(mode, table, image_counts(sizes, counts), R)
    ref = token_groups_per_call(mode, sizes, counts, R)
    assert got == ref
    assert len(got) == sum(k * min(n, R) for k, n in zip(sizes, counts))
    for row, keys in got.items():
        b, r = divmod(row, R)
        assert row in keys and keys == sorted(keys)
        assert all(table[0, kr // R] == table[0, b] for kr in keys)          # a group never leaves its segment
        assert len(keys) == (min(counts[np.searchsorted(np.cumsum(sizes), b, 'right')], R) if mode == ACROSS_ROIS else table[1, b])


def test_constants_agree_with_the_op_layer():
    assert (ACROSS_ROIS, ACROSS_IMAGES) == (ops.MHA_ACROSS_ROIS, ops.MHA_ACROSS_IMAGES)
    assert ops.MHA_SMAX == 128


def test_float64_attention_of_a_singleton_group_is_the_value_row():
    rng = np.random.default_rng(0)
    q, k, v = (rng.standard_normal((6, 16)) for _ in range(3))
    groups = token_groups(ACROSS_IMAGES, table_of([1, 1, 1]), [2, 0, 1], 2)
    assert sorted(groups) == [0, 1, 4]
    out = attention_f64(q, k, v, groups, 4)
    assert np.array_equal(out[[0, 1, 4]], v[[0, 1, 4]]) and not out[[2, 3, 5]].any()
