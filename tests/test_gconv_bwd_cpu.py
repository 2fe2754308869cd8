"""CPU (no GPU needed): the host-only parts of the grouped convolution's gradients -- the prepared weights of the data gradient
(`_prep.gconv_dgrad`) and the planner / workspace query of the weight gradient (`ops.gconv_wgrad_plan`,
`nbm_gconv3x3_wgrad_workspace`)."""
import ctypes as C

import pytest
import torch

from birdsoundclassif_amd import _lib, ops
from birdsoundclassif_amd.nets import _prep

GROUPS = [(32, 4), (32, 8), (32, 16), (32, 32), (32, 64), (64, 4)]          # (G, Cg) of tests/test_gpu_gconv.py

# the 14 distinct grouped launches of DESIGN 4k's table on a 375 x 1024 image: (input H, W, C, Cg, stride)
LAUNCHES = [(94, 256, 128, 4, 1), (94, 256, 256, 8, 2), (47, 128, 256, 8, 1), (47, 128, 512, 16, 2), (24, 64, 512, 16, 1),
            (24, 64, 1024, 32, 2), (12, 32, 1024, 32, 1),
            (94, 256, 256, 8, 1), (94, 256, 512, 16, 2), (47, 128, 512, 16, 1), (47, 128, 1024, 32, 2), (24, 64, 1024, 32, 1),
            (24, 64, 2048, 64, 2), (12, 32, 2048, 64, 1)]
CUS = 256


@pytest.mark.parametrize('G,Cg', GROUPS)
def test_dgrad_weights_are_the_fragments_of_the_transposed_rotated_scaled_weight(G, Cg):
    gen = torch.Generator().manual_seed(10 * Cg + G)
    Cn = G * Cg
    w = torch.randn(Cn, Cg, 3, 3, generator=gen)
    scale = torch.randn(Cn, generator=gen)
    for sc in (None, scale):
        # W'[g Cg + c][n][r][s] = scale[g Cg + n] * W[g Cg + n][c][2 - r][2 - s], element by element
        wx = torch.empty_like(w)
        w5 = w.view(G, Cg, Cg, 3, 3)
        for r in range(3):
            for s in range(3):
                t = w5[:, :, :, 2 - r, 2 - s]                                   # [g][n][c]
                if sc is not None:
                    t = t * sc.view(G, Cg, 1)
                wx.view(G, Cg, Cg, 3, 3)[:, :, :, r, s] = t.transpose(1, 2)     # [g][c][n]
        got = _prep.gconv_dgrad(w, G, sc)
        assert tuple(got.shape) == (Cn // 16, 9, max(Cg, 16) // 16, 64, 4)
        assert torch.equal(got, _prep.gconv(wx, G)), (G, Cg, sc is not None)
    # a new scale tensor replaces the entry instead of adding one
    assert not torch.equal(_prep.gconv_dgrad(w, G, scale * 2), _prep.gconv_dgrad(w, G, scale))
    with pytest.raises(ValueError):
        _prep.gconv_dgrad(torch.zeros(32 * 12, 12, 3, 3), 32)


def _query(B, H, W, groups, Cg, stride, splits=0):
    d = ops._gconv_bwd_desc(B, H, W, groups, Cg, stride, splits=splits)
    n = C.c_longlong(-1)
    return _lib.load().nbm_gconv3x3_wgrad_workspace(C.byref(d), C.byref(n)), n.value


@pytest.mark.parametrize('B', [64, 128])
@pytest.mark.parametrize('H,W,Cn,Cg,stride', LAUNCHES)
def test_plan_of_the_backbone_launches(B, H, W, Cn, Cg, stride):
    G = Cn // Cg
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    splits, nbytes = ops.gconv_wgrad_plan(B, Ho, Wo, G, Cg, stride)
    assert splits >= 1
    rc, through_ctypes = _query(B, H, W, G, Cg, stride)
    assert rc == 0 and through_ctypes == nbytes
    # linear in the split count: one split holds C x 9 x max(Cg, 16) floats
    per_split = Cn * 9 * max(Cg, 16) * 4
    assert nbytes == splits * per_split
    for s in (1, 3, splits):
        assert _query(B, H, W, G, Cg, stride, splits=s) == (0, s * per_split)
    # the reduce pass stays a minor share of the traffic: no more than the two operands the launch reads
    assert nbytes <= 4 * B * Cn * (Ho * Wo + H * W)
    # at least one workgroup per CU wherever the pixels allow it (a workgroup = one split of 64 channels; a split needs at least one
    # pixel tile of 4 x 16 (stride 1) / 2 x 16 (stride 2) gradient pixels, and the workspace bound above caps the splits too)
    TH = 4 if stride == 1 else 2
    n_tiles = B * ((Ho + TH - 1) // TH) * ((Wo + 15) // 16)
    possible = min(n_tiles, 4 * B * Cn * 2 * Ho * Wo // per_split)      # (the planner counts x with the pixels of g: H W >= Ho Wo)
    workgroups = splits * (Cn // 64)
    print(f'B={B} {H}x{W} C={Cn} Cg={Cg} stride={stride}: splits {splits}, {workgroups} workgroups, workspace {nbytes / 2 ** 20:.1f} MiB')
    if possible * (Cn // 64) >= CUS:
        assert workgroups >= CUS
    assert splits <= n_tiles


def test_unsupported_geometry_is_refused_by_the_workspace_query():
    assert _query(2, 8, 8, 32, 4, 1)[0] == 0
    assert _query(2, 8, 8, 32, 12, 1) == (-3, -1)                    # Cg = 12
    assert _query(2, 8, 8, 32, 4, 3) == (-3, -1)                     # stride 3
    assert _query(2, 8, 8, 24, 4, 1) == (-3, -1)                     # C = 96: no multiple of 64
    with pytest.raises(_lib.NbmHipError, match='NBM_EUNSUPPORTED'):
        ops.gconv_wgrad_plan(2, 8, 8, 32, 12, 1)


def test_the_gradient_ops_refuse_cpu_tensors():
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.gconv3x3_dgrad(torch.zeros(1, 4, 4, 128), torch.zeros(8, 9, 1, 64, 4), 32, 4, 4)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.gconv3x3_wgrad(torch.zeros(1, 4, 4, 128), torch.zeros(1, 4, 4, 128), 32)
