"""CPU: `ops.proposal_plan`, the host-only choice of the proposal kernels from the pre-NMS budget and the anchor count."""
import pytest

from birdsoundclassif_amd import ops


@pytest.mark.parametrize('pre,ka,expected', [
    (3000, 23040, (3000, 4096, 'small')),           # the training default
    (500, 23040, (500, 512, 'small')),              # the evaluation default
    (4096, 23040, (4096, 4096, 'small')),
    (4097, 23040, (4097, 8192, 'big')),
    (6000, 450, (450, 512, 'small')),               # a budget above 4096 on a small map is cut to the map
    (10 ** 6, 23040, (23040, 32768, 'big')),
    (50000, 38400, (38400, 65536, 'big')),          # --n_ratios 5: the largest map the flags can produce
])
def test_plan(pre, ka, expected):
    assert ops.proposal_plan(pre, ka) == expected


def test_a_budget_of_4096_or_less_is_never_cut_to_the_map():
    """Today's launches: top_n = pre even where the map holds fewer anchors."""
    assert ops.proposal_plan(3000, 450) == (3000, 4096, 'small')


def test_more_than_65536_boxes_names_the_flag():
    with pytest.raises(ValueError, match='pre_nms_topN'):
        ops.proposal_plan(70000, 70000)
