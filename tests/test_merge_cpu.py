"""CPU: the per-file merge entry points are declared, bound and exported, and the scalable CPU greedy of
tests/merge_cpu_ref.py agrees with oracle.nets_ref.greedy_nms_keep."""
import ctypes
import os

import numpy as np
import pytest
import torch

from birdsoundclassif_amd import _lib, ops
from merge_cpu_ref import greedy_keep, make_boxes, ulp_pairs
from oracle import nets_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MERGE_SYMBOLS = ('nbm_merge_collect', 'nbm_merge_nms_workspace', 'nbm_merge_nms', 'nbm_merge_gather')


def test_merge_symbols_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'nbm_hip.h')).read()
    assert '#define NBM_MERGE_MAX_N 131072' in header and ops.MERGE_MAX_N == 131072
    if not os.path.isfile(_lib.LIB_PATH):
        _lib.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in MERGE_SYMBOLS:
        assert f'{s}(' in header, s
        assert s in _lib.SIGNATURES, s
        assert hasattr(lib, s), s
    for s in ('merge_collect', 'merge_nms', 'merge_gather', 'merge_nms_workspace_bytes'):
        assert callable(getattr(ops, s))


def test_workspace_query_and_limit():
    # the query needs no device: dense triangle of 64 x 64-bit tiles + the block ranges
    nb = 131072 // 64
    assert ops.merge_nms_workspace_bytes(131072) >= nb * (nb + 1) // 2 * 512
    assert ops.merge_nms_workspace_bytes(0) > 0
    with pytest.raises(ValueError):
        ops.merge_nms_workspace_bytes(131073)
    nbytes = ctypes.c_int64()
    assert _lib.load().nbm_merge_nms_workspace(131073, ctypes.byref(nbytes)) == -1
    # a null workspace / over-limit capacity is refused before any launch
    assert _lib.load().nbm_merge_nms(None, None, 131073, ctypes.c_float(0.3), None, 0, None, None, None) == -1


@pytest.mark.parametrize('layout', ['realistic', 'dense', 'scattered'])
@pytest.mark.parametrize('n', [0, 1, 2, 63, 64, 65, 300, 1500])
def test_cpu_greedy_matches_oracle(layout, n):
    b = make_boxes(layout, n, seed=n + 7)
    assert greedy_keep(b, 0.3) == O.greedy_nms_keep(torch.from_numpy(b), 0.3)


def test_cpu_greedy_matches_oracle_random_and_ulp_pairs():
    rng = np.random.default_rng(5)
    for _ in range(20):
        n = int(rng.integers(1, 600))
        b = (rng.uniform(0, 3000, (n, 4)) + np.array([0, 0, 0, 0])).astype(np.float32)
        b[:, 2] = b[:, 0] + rng.uniform(0, 300, n).astype(np.float32)
        b[:, 3] = b[:, 1] + rng.uniform(0, 300, n).astype(np.float32)
        assert greedy_keep(b, 0.3) == O.greedy_nms_keep(torch.from_numpy(b), 0.3)
    # one ulp below float32(0.3) keeps the second box, exactly float32(0.3) and one ulp above remove it
    got = [greedy_keep(np.stack([a, b]), 0.3) for a, b in ulp_pairs()]
    assert got == [[0, 1], [0], [0]]
    assert got == [O.greedy_nms_keep(torch.from_numpy(np.stack([a, b])), 0.3) for a, b in ulp_pairs()]
