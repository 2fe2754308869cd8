"""GPU: every GEMM-type launch of a B = 128 training step (positive and negative), checked at the size it runs at.

The table below lists each distinct launch: the backward ones as their `ops.PROFILE_BWD` keys (kind, B, H, W, Cin, N, k, stride,
groups), the forward ones as their `ops.PROFILE` keys (Cin, N, kh, H, W, B, groups, stride, label), each with the epilogue operands and
pitches the model passes there (nets/functional.py, ondemand.py) and the steps it occurs in ('p' positive, 'n' negative).  `S(v)` marks
a dimension that depends on the step's data (RoI tile lists, device-side counts): the census matches it as a wildcard and the exact
check runs it at v, the size this step recorded.  FWD_OTHER: launches that are not plain implicit GEMMs (the fused Winograd kernels,
the stem, whole-op brackets, the listed-pixel lateral): census only here; their GEMM parts have their own entries.

`test_census_*` runs one positive and one negative B = 128 step with both profile lists on and asserts that the recorded key set is
the table's.  The exact checks then run every entry as one raw launch at its real geometry with small-integer operands (one operand
in {-1, 0, 1}, the other in {-2, ..., 2}, dyadic scales): every product and partial sum is an integer multiple of the smallest scale
well below 2^24 of it, so fp32 gives the same bits in any summation order and the kernel must equal the float64 reference
(tests/conv_ref.py) bit for bit on every output element, under NBM_SPLIT_BF16=0 and =1.  Outputs are allocated with guard rows and
a pitch above the width, NaN-filled: what the launch must not write stays NaN.  The precision cases use randn operands."""
import math
import os

import numpy as np
import pytest
import torch

import conv_ref as R

pytestmark = pytest.mark.gpu


class S(int):
    """A dimension that depends on the step's data; the value is what the census step recorded."""

    def __repr__(self):
        return f'S({int(self)})'


T = 'T'        # the launch passes this operand (a tensor)


# ------------------------------------------------------------------------------------------------------------ the launch table
# (kind, B, H, W, Cin, N, k, stride, groups), steps, epilogue operands / pitches
BWD = [
    (('dgrad', 128, 94, 256, 64, 64, 1, 1, 1), 'np', dict(a_scale=T, g_ld=64, residual=T, w_ld=64)),
    (('dgrad', 128, 94, 256, 64, 64, 3, 1, 1), 'np', dict(a_scale=T, g_ld=64, mask=T, w_ld=576)),
    (('dgrad', 128, 94, 256, 64, 256, 1, 1, 1), 'np', dict(a_scale=T, g_ld=256, mask=T, mask_bits=T, w_ld=64)),
    (('dgrad', 128, 94, 256, 64, 256, 1, 1, 1), 'np', dict(a_scale=T, g_ld=256, w_ld=64)),
    (('dgrad', 128, 94, 256, 128, 128, 3, 2, 1), 'np', dict(a_scale=T, g_ld=128, mask=T, w_ld=1152)),
    (('dgrad', 128, 94, 256, 256, 64, 1, 1, 1), 'np', dict(a_scale=T, g_ld=64, mask=T, mask_bits=T, residual=T, w_ld=256)),
    (('dgrad', 128, 94, 256, 256, 128, 1, 1, 1), 'np', dict(a_scale=T, g_ld=128, mask=T, mask_bits=T, residual=T, residual2=T, w_ld=256)),
    (('dgrad', 128, 94, 256, 256, 384, 1, 1, 1), 'np', dict(alpha=2.0, g_ld=384, w_ld=256)),
    (('dgrad', 1, S(1284096), 1, 64, 384, 1, 1, 1), 'n', dict(alpha=2.0, g_ld=384, w_ld=64)),
    (('dgrad', 128, 47, 128, 128, 512, 1, 1, 1), 'np', dict(a_scale=T, g_ld=512, mask=T, w_ld=128)),
    (('dgrad', 128, 47, 128, 128, 512, 1, 1, 1), 'np', dict(a_scale=T, g_ld=512, mask=T, mask_bits=T, w_ld=128)),
    (('dgrad', 128, 47, 128, 256, 256, 3, 2, 1), 'np', dict(a_scale=T, g_ld=256, mask=T, w_ld=2304)),
    (('dgrad', 128, 47, 128, 256, 512, 1, 1, 1), 'np', dict(a_scale=T, g_ld=512, w_ld=256)),
    (('dgrad', 128, 47, 128, 512, 128, 1, 1, 1), 'np', dict(a_scale=T, g_ld=128, mask=T, mask_bits=T, residual=T, w_ld=512)),
    (('dgrad', 128, 47, 128, 512, 256, 1, 1, 1), 'np', dict(a_scale=T, g_ld=256, mask=T, mask_bits=T, residual=T, residual2=T, w_ld=512)),
    (('dgrad', 128, 47, 128, 512, 384, 1, 1, 1), 'np', dict(alpha=2.0, g_ld=384, w_ld=512)),
    (('dgrad', 1, S(624640), 1, 64, 384, 1, 1, 1), 'n', dict(alpha=2.0, g_ld=384, w_ld=64)),
    (('dgrad', 128000, 2, 2, 256, 2048, 1, 1, 1), 'n', dict(g_ld=2048, w_ld=256)),
    (('dgrad', 128000, 2, 2, 1024, 256, 1, 1, 1), 'n', dict(g_ld=256, w_ld=1024)),
    (('dgrad', 1, 196608, 1, 1024, 384, 1, 1, 1), 'np', dict()),
    (('dgrad', 1, 196608, 1, 1024, 1408, 1, 1, 1), 'np', dict(residual=T)),
    (('dgrad', 128, 24, 64, 256, 18, 1, 1, 1), 'np', dict(g_ld=32, w_ld=256)),
    (('dgrad', 128, 24, 64, 256, 1024, 1, 1, 1), 'np', dict(a_scale=T, g_ld=1024, mask=T, w_ld=256)),
    (('dgrad', 128, 24, 64, 256, 1024, 1, 1, 1), 'np', dict(a_scale=T, g_ld=1024, mask=T, mask_bits=T, w_ld=256)),
    (('dgrad', 128, 24, 64, 512, 256, 1, 1, 1), 'np', dict(g_ld=256, w_ld=512)),
    (('dgrad', 128, 24, 64, 512, 512, 3, 2, 1), 'np', dict(a_scale=T, g_ld=512, mask=T, w_ld=4608)),
    (('dgrad', 128, 24, 64, 512, 1024, 1, 1, 1), 'np', dict(a_scale=T, g_ld=1024, w_ld=512)),
    (('dgrad', 128, 24, 64, 1024, 256, 1, 1, 1), 'np', dict(a_scale=T, g_ld=256, mask=T, mask_bits=T, residual=T, w_ld=1024)),
    (('dgrad', 128, 24, 64, 1024, 512, 1, 1, 1), 'np', dict(a_scale=T, g_ld=512, mask=T, mask_bits=T, residual=T, residual2=T, w_ld=1024)),
    (('dgrad', 1, 128000, 1, 1024, 151, 1, 1, 1), 'n', dict(g_ld=160, w_ld=1024)),
    (('dgrad', 1, 49152, 1, 2048, 384, 1, 1, 1), 'np', dict()),
    (('dgrad', 1, 49152, 1, 2048, 2432, 1, 1, 1), 'np', dict(residual=T)),
    (('dgrad', 128, 12, 32, 512, 2048, 1, 1, 1), 'np', dict(a_scale=T, g_ld=2048, mask=T, w_ld=512)),
    (('dgrad', 128, 12, 32, 512, 2048, 1, 1, 1), 'np', dict(a_scale=T, g_ld=2048, mask=T, mask_bits=T, w_ld=512)),
    (('dgrad', 128, 12, 32, 1024, 2048, 1, 1, 1), 'np', dict(a_scale=T, g_ld=2048, w_ld=1024)),
    (('dgrad', 128, 12, 32, 2048, 512, 1, 1, 1), 'np', dict(a_scale=T, g_ld=512, mask=T, mask_bits=T, residual=T, w_ld=2048)),
    (('dgrad', 1, S(15360), 1, 64, 384, 1, 1, 1), 'p', dict(alpha=2.0, g_ld=384, w_ld=64)),
    (('dgrad', 1, S(9216), 1, 64, 384, 1, 1, 1), 'p', dict(alpha=2.0, g_ld=384, w_ld=64)),
    (('dgrad', 2048, 2, 2, 256, 2048, 1, 1, 1), 'p', dict(g_ld=2048, w_ld=256)),
    (('dgrad', 2048, 2, 2, 1024, 256, 1, 1, 1), 'p', dict(g_ld=256, w_ld=1024)),
    (('dgrad', 1, 2048, 1, 1024, 151, 1, 1, 1), 'p', dict(g_ld=160, w_ld=1024)),
    (('dgrad', 1, 2048, 1, 1024, 604, 1, 1, 1), 'p', dict(g_ld=608, w_ld=1024)),
    (('dgrad', 1, 1536, 1, 384, 1536, 1, 1, 128), 'np', dict(g_gs=2359296, g_ld=1536, out_gs=589824, out_ld=384, w_gs=2162688, w_ld=1408)),
    (('dgrad', 1, 1536, 1, 512, 1536, 1, 1, 128), 'np', dict(g_gs=2359296, g_ld=1536, out_gs=2162688, out_ld=1408, w_gs=2162688, w_ld=1408)),
    (('dgrad', 1, 384, 1, 384, 384, 1, 1, 128), 'np', dict(g_gs=147456, g_ld=384, out_gs=147456, out_ld=384, w_gs=933888, w_ld=2432)),
    (('dgrad', 1, 384, 1, 1024, 384, 1, 1, 128), 'np', dict(g_gs=147456, g_ld=384, out_gs=933888, out_ld=2432, w_gs=933888, w_ld=2432)),
    (('wgrad', 128, 94, 256, 64, 64, 1, 1, 1), 'np', dict(g_ld=64, out_ld=64, row_scale=T)),
    (('wgrad', 128, 94, 256, 64, 64, 3, 1, 1), 'np', dict(g_ld=64, out_ld=576, row_scale=T)),
    (('wgrad', 128, 94, 256, 64, 256, 1, 1, 1), 'np', dict(g_ld=256, out_ld=64, row_scale=T)),
    (('wgrad', 128, 94, 256, 128, 128, 3, 2, 1), 'np', dict(g_ld=128, out_ld=1152, row_scale=T)),
    (('wgrad', 128, 94, 256, 256, 64, 1, 1, 1), 'np', dict(g_ld=64, out_ld=256, row_scale=T)),
    (('wgrad', 128, 94, 256, 256, 128, 1, 1, 1), 'np', dict(g_ld=128, out_ld=256, row_scale=T)),
    (('wgrad', 128, 94, 256, 256, 384, 1, 1, 1), 'np', dict(alpha=2.0, bias_grad=T, g_ld=384, out_ld=256)),
    (('wgrad', 128, 94, 256, 256, 512, 1, 2, 1), 'np', dict(g_ld=512, out_ld=256, row_scale=T)),
    (('wgrad', 1, S(1284096), 1, 64, 384, 1, 1, 1), 'n', dict(alpha=2.0, bias_grad=T)),
    (('wgrad', 128, 47, 128, 128, 512, 1, 1, 1), 'np', dict(g_ld=512, out_ld=128, row_scale=T)),
    (('wgrad', 128, 47, 128, 256, 256, 3, 2, 1), 'np', dict(g_ld=256, out_ld=2304, row_scale=T)),
    (('wgrad', 128, 47, 128, 512, 128, 1, 1, 1), 'np', dict(g_ld=128, out_ld=512, row_scale=T)),
    (('wgrad', 128, 47, 128, 512, 256, 1, 1, 1), 'np', dict(g_ld=256, out_ld=512, row_scale=T)),
    (('wgrad', 128, 47, 128, 512, 384, 1, 1, 1), 'np', dict(alpha=2.0, bias_grad=T, g_ld=384, out_ld=512)),
    (('wgrad', 128, 47, 128, 512, 1024, 1, 2, 1), 'np', dict(g_ld=1024, out_ld=512, row_scale=T)),
    (('wgrad', 1, S(624640), 1, 64, 384, 1, 1, 1), 'n', dict(alpha=2.0, bias_grad=T)),
    (('wgrad', 128000, 2, 2, 256, 256, 1, 1, 1), 'n', dict(bias_grad=T, g_ld=256, out_ld=256)),
    (('wgrad', 128000, 2, 2, 256, 2048, 1, 1, 1), 'n', dict(bias_grad=T, g_ld=2048, out_ld=256)),
    (('wgrad', 128000, 2, 2, 1024, 256, 1, 1, 1), 'n', dict(bias_grad=T, g_ld=256, out_ld=1024)),
    (('wgrad', 1, S(292096), 1, 384, 256, 1, 1, 16), 'n', dict(g_gs=74776576, out_gs=98304, x_gs=112164864)),
    (('wgrad', 1, S(210944), 1, 384, 256, 1, 1, 16), 'n', dict(g_gs=54001664, out_gs=98304, x_gs=81002496)),
    (('wgrad', 1, 196608, 1, 384, 256, 1, 1, 25), 'np', dict(g_gs=0, out_gs=384, out_ld=9600, x_gs=75497472)),
    (('wgrad', 1, 196608, 1, 1024, 384, 1, 1, 1), 'np', dict()),
    (('wgrad', 1, 196608, 1, 1024, 1408, 1, 1, 1), 'np', dict()),
    (('wgrad', 128, 24, 64, 256, 18, 1, 1, 1), 'np', dict(bias_grad=T, g_ld=32, out_ld=256)),
    (('wgrad', 128, 24, 64, 256, 1024, 1, 1, 1), 'np', dict(g_ld=1024, out_ld=256, row_scale=T)),
    (('wgrad', 128, 24, 64, 512, 256, 1, 1, 1), 'np', dict(bias_grad=T, g_ld=256, out_ld=512)),
    (('wgrad', 128, 24, 64, 512, 512, 3, 2, 1), 'np', dict(g_ld=512, out_ld=4608, row_scale=T)),
    (('wgrad', 128, 24, 64, 1024, 256, 1, 1, 1), 'np', dict(g_ld=256, out_ld=1024, row_scale=T)),
    (('wgrad', 128, 24, 64, 1024, 512, 1, 1, 1), 'np', dict(g_ld=512, out_ld=1024, row_scale=T)),
    (('wgrad', 128, 24, 64, 1024, 2048, 1, 2, 1), 'np', dict(g_ld=2048, out_ld=1024, row_scale=T)),
    (('wgrad', 1, S(142080), 1, 384, 256, 1, 1, 16), 'n', dict(g_gs=36372480, out_gs=98304, x_gs=54558720)),
    (('wgrad', 1, 132096, 1, 448, 256, 1, 1, 25), 'np', dict(g_gs=0, out_gs=448, out_ld=11200, x_gs=59179008)),
    (('wgrad', 1, 128000, 1, 1024, 151, 1, 1, 1), 'n', dict(bias_grad=T, g_ld=160, out_ld=1024)),
    (('wgrad', 1, 64512, 1, 448, 256, 1, 1, 25), 'np', dict(g_gs=0, out_gs=448, out_ld=11200, x_gs=28901376)),
    (('wgrad', 1, 49152, 1, 128, 128, 1, 1, 36), 'np', dict(g_gs=6291456, out_gs=16384, x_gs=6291456)),
    (('wgrad', 1, 49152, 1, 384, 256, 1, 1, 36), 'np', dict(g_gs=12582912, out_gs=98304, x_gs=18874368)),
    (('wgrad', 1, 49152, 1, 2048, 384, 1, 1, 1), 'np', dict()),
    (('wgrad', 1, 49152, 1, 2048, 2432, 1, 1, 1), 'np', dict()),
    (('wgrad', 128, 12, 32, 512, 2048, 1, 1, 1), 'np', dict(g_ld=2048, out_ld=512, row_scale=T)),
    (('wgrad', 128, 12, 32, 2048, 512, 1, 1, 1), 'np', dict(g_ld=512, out_ld=2048, row_scale=T)),
    (('wgrad', 1, S(16896), 1, 384, 256, 1, 1, 16), 'p', dict(g_gs=4325376, out_gs=98304, x_gs=6488064)),
    (('wgrad', 1, S(15360), 1, 64, 384, 1, 1, 1), 'p', dict(alpha=2.0, bias_grad=T)),
    (('wgrad', 1, 12288, 1, 256, 256, 1, 1, 36), 'np', dict(g_gs=3145728, out_gs=65536, x_gs=3145728)),
    (('wgrad', 1, 12288, 1, 384, 256, 1, 1, 36), 'np', dict(g_gs=3145728, out_gs=98304, x_gs=4718592)),
    (('wgrad', 1, S(9216), 1, 64, 384, 1, 1, 1), 'p', dict(alpha=2.0, bias_grad=T)),
    (('wgrad', 2048, 2, 2, 256, 256, 1, 1, 1), 'p', dict(bias_grad=T, g_ld=256, out_ld=256)),
    (('wgrad', 2048, 2, 2, 256, 2048, 1, 1, 1), 'p', dict(bias_grad=T, g_ld=2048, out_ld=256)),
    (('wgrad', 2048, 2, 2, 1024, 256, 1, 1, 1), 'p', dict(bias_grad=T, g_ld=256, out_ld=1024)),
    (('wgrad', 1, 8064, 1, 384, 256, 1, 1, 25), 'np', dict(g_gs=0, out_gs=384, out_ld=9600, x_gs=3096576)),
    (('wgrad', 1, 6400, 1, 64, 384, 1, 1, 1), 'np', dict(alpha=2.0, g_ld=448, x_ld=448)),
    (('wgrad', 1, 5418, 1, 448, 256, 1, 1, 25), 'np', dict(g_gs=0, out_gs=448, out_ld=11200, x_gs=2427264)),
    (('wgrad', 1, S(3584), 1, 384, 256, 1, 1, 16), 'p', dict(g_gs=917504, out_gs=98304, x_gs=1376256)),
    (('wgrad', 1, 3072, 1, 384, 256, 1, 1, 36), 'np', dict(g_gs=786432, out_gs=98304, x_gs=1179648)),
    (('wgrad', 1, 3072, 1, 512, 512, 1, 1, 36), 'np', dict(g_gs=1572864, out_gs=262144, x_gs=1572864)),
    (('wgrad', 1, 2944, 1, 384, 256, 1, 1, 25), 'np', dict(g_gs=0, out_gs=384, out_ld=9600, x_gs=1130496)),
    (('wgrad', 1, 2646, 1, 448, 256, 1, 1, 25), 'np', dict(g_gs=0, out_gs=448, out_ld=11200, x_gs=1185408)),
    (('wgrad', 1, S(2176), 1, 384, 256, 1, 1, 16), 'p', dict(g_gs=557056, out_gs=98304, x_gs=835584)),
    (('wgrad', 1, 2048, 1, 1024, 151, 1, 1, 1), 'p', dict(bias_grad=T, g_ld=160, out_ld=1024)),
    (('wgrad', 1, 2048, 1, 1024, 604, 1, 1, 1), 'p', dict(bias_grad=T, g_ld=608, out_ld=1024)),
    (('wgrad', 1, 1978, 1, 448, 256, 1, 1, 25), 'np', dict(g_gs=0, out_gs=448, out_ld=11200, x_gs=886144)),
    (('wgrad', 1, 1536, 1, 384, 1536, 1, 1, 128), 'np', dict(g_gs=2359296, g_ld=1536, out_gs=2162688, out_ld=1408, x_gs=589824, x_ld=384)),
    (('wgrad', 1, 1536, 1, 512, 1536, 1, 1, 128), 'np', dict(g_gs=2359296, g_ld=1536, out_gs=2162688, out_ld=1408, x_gs=2162688, x_ld=1408)),
    (('wgrad', 1, 966, 1, 448, 256, 1, 1, 25), 'np', dict(g_gs=0, out_gs=448, out_ld=11200, x_gs=432768)),
    (('wgrad', 1, 384, 1, 384, 384, 1, 1, 128), 'np', dict(g_gs=147456, g_ld=384, out_gs=933888, out_ld=2432, x_gs=147456, x_ld=384)),
    (('wgrad', 1, 384, 1, 1024, 384, 1, 1, 128), 'np', dict(g_gs=147456, g_ld=384, out_gs=933888, out_ld=2432, x_gs=933888, x_ld=2432)),
    (('wgrad', 1, 256, 1, 384, 256, 1, 1, 25), 'np', dict(g_gs=65536, out_gs=98304, x_gs=384, x_ld=9600)),
    (('wgrad', 1, 256, 1, 448, 256, 1, 1, 25), 'np', dict(g_gs=65536, out_gs=114688, x_gs=448, x_ld=11200)),
    (('wgrad', 1, 128, 1, 384, 256, 1, 1, 25), 'np', dict(g_gs=0, out_gs=384, out_ld=9600, x_gs=49152)),
    (('wgrad', 1, 86, 1, 448, 256, 1, 1, 25), 'np', dict(g_gs=0, out_gs=448, out_ld=11200, x_gs=38528)),
    (('wgrad', 1, 42, 1, 448, 256, 1, 1, 25), 'np', dict(g_gs=0, out_gs=448, out_ld=11200, x_gs=18816)),
]
# (Cin, N, kh, H, W, B, groups, stride, label), steps, epilogue operands / pitches
FWD = [
    ((64, 64, 1, 94, 256, 128, 1, 1, None), 'np', dict(act=1, scale=T, shift=T, w_ld=64)),
    ((64, 64, 3, 94, 256, 128, 1, 1, None), 'np', dict(act=1, bits_out=T, scale=T, shift=T, w_ld=576)),
    ((64, 256, 1, 94, 256, 128, 1, 1, None), 'np', dict(scale=T, shift=T, w_ld=64)),
    ((64, 256, 1, 94, 256, 128, 1, 1, None), 'np', dict(act=1, bits_out=T, residual=T, scale=T, shift=T, w_ld=64)),
    ((128, 128, 3, 94, 256, 128, 1, 2, None), 'np', dict(act=1, bits_out=T, scale=T, shift=T, w_ld=1152)),
    ((256, 64, 1, 94, 256, 128, 1, 1, None), 'np', dict(act=1, scale=T, shift=T, w_ld=256)),
    ((256, 128, 1, 94, 256, 128, 1, 1, None), 'np', dict(act=1, scale=T, shift=T, w_ld=256)),
    ((256, 384, 1, 94, 256, 128, 1, 1, None), 'np', dict(alpha=2.0, shift=T, up=T, w_ld=256)),
    ((256, 512, 1, 94, 256, 128, 1, 2, None), 'np', dict(scale=T, shift=T, w_ld=256)),
    ((384, 256, 5, 5, 196608, 1, 5, 1, ('rpn-composite-train', 94, 256)), 'np', dict(w_gs=1920, w_ld=9600, x_gs=377487360, x_ld=384, y_gs=50331648)),
    ((128, 512, 1, 47, 128, 128, 1, 1, None), 'np', dict(act=1, bits_out=T, residual=T, scale=T, shift=T, w_ld=128)),
    ((256, 256, 3, 47, 128, 128, 1, 2, None), 'np', dict(act=1, bits_out=T, scale=T, shift=T, w_ld=2304)),
    ((512, 128, 1, 47, 128, 128, 1, 1, None), 'np', dict(act=1, scale=T, shift=T, w_ld=512)),
    ((512, 256, 1, 47, 128, 128, 1, 1, None), 'np', dict(act=1, scale=T, shift=T, w_ld=512)),
    ((512, 384, 1, 47, 128, 128, 1, 1, None), 'np', dict(alpha=2.0, shift=T, up=T, w_ld=512)),
    ((512, 1024, 1, 47, 128, 128, 1, 2, None), 'np', dict(scale=T, shift=T, w_ld=512)),
    ((448, 256, 5, 5, 132096, 1, 5, 1, ('rpn-composite-train', 188, 512)), 'np', dict(w_gs=2240, w_ld=11200, x_gs=295895040, x_ld=448, y_gs=33816576)),
    ((256, 256, 1, 2, 2, 128000, 1, 1, None), 'n', dict(shift=T, w_ld=256)),
    ((256, 2048, 1, 2, 2, 128000, 1, 1, None), 'n', dict(shift=T, w_ld=256)),
    ((1024, 256, 1, 2, 2, 128000, 1, 1, None), 'n', dict(shift=T, w_ld=1024)),
    ((448, 256, 5, 5, 64512, 1, 5, 1, ('rpn-composite-train', 188, 512)), 'np', dict(w_gs=2240, w_ld=11200, x_gs=144506880, x_ld=448, y_gs=16515072)),
    ((256, 18, 1, 24, 64, 128, 1, 1, None), 'np', dict(shift=T, w_ld=256)),
    ((256, 384, 1, 196608, 1, 1, 25, 1, ('cell-dgrad', 94, 256)), 'np', dict(w_gs=98304, x_gs=0, y_gs=75497472)),
    ((256, 1024, 1, 24, 64, 128, 1, 1, None), 'np', dict(act=1, bits_out=T, residual=T, scale=T, shift=T, w_ld=256)),
    ((512, 256, 1, 24, 64, 128, 1, 1, None), 'np', dict(shift=T, w_ld=512)),
    ((512, 512, 3, 24, 64, 128, 1, 2, None), 'np', dict(act=1, bits_out=T, scale=T, shift=T, w_ld=4608)),
    ((1024, 256, 1, 24, 64, 128, 1, 1, None), 'np', dict(act=1, scale=T, shift=T, w_ld=1024)),
    ((1024, 384, 1, 24, 64, 128, 1, 1, None), 'np', dict(residual=T, shift=T, up=T, w_ld=1024)),
    ((1024, 512, 1, 24, 64, 128, 1, 1, None), 'np', dict(act=1, scale=T, shift=T, w_ld=1024)),
    ((1024, 1408, 1, 196608, 1, 1, 1, 1, None), 'np', dict(shift=T, w_ld=1024)),
    ((1024, 2048, 1, 24, 64, 128, 1, 2, None), 'np', dict(scale=T, shift=T, w_ld=1024)),
    ((256, 448, 1, 132096, 1, 1, 25, 1, ('cell-dgrad', 188, 512)), 'np', dict(w_gs=114688, x_gs=0, y_gs=59179008)),
    ((1024, 151, 1, 128000, 1, 1, 1, 1, None), 'n', dict(shift=T, w_ld=1024)),
    ((1024, 604, 1, 128000, 1, 1, 1, 1, None), 'n', dict(shift=T, w_ld=1024)),
    ((256, 448, 1, 64512, 1, 1, 25, 1, ('cell-dgrad', 188, 512)), 'np', dict(w_gs=114688, x_gs=0, y_gs=28901376)),
    ((128, 128, 1, 49152, 1, 1, 36, 1, ('wino23', 47, 128)), 'np', dict(w_gs=16384, x_gs=6291456, y_gs=6291456)),
    ((256, 384, 1, 49152, 1, 1, 36, 1, ('wino23', 47, 128)), 'np', dict(w_gs=98304, x_gs=12582912, y_gs=18874368)),
    ((512, 2048, 1, 12, 32, 128, 1, 1, None), 'np', dict(act=1, bits_out=T, residual=T, scale=T, shift=T, w_ld=512)),
    ((2048, 384, 1, 12, 32, 128, 1, 1, None), 'np', dict(residual=T, shift=T, w_ld=2048)),
    ((2048, 512, 1, 12, 32, 128, 1, 1, None), 'np', dict(act=1, scale=T, shift=T, w_ld=2048)),
    ((2048, 2432, 1, 49152, 1, 1, 1, 1, None), 'np', dict(shift=T, w_ld=2048)),
    ((256, 256, 1, 12288, 1, 1, 36, 1, ('wino23', 24, 64)), 'np', dict(w_gs=65536, x_gs=3145728, y_gs=3145728)),
    ((256, 384, 1, 12288, 1, 1, 36, 1, ('wino23', 24, 64)), 'np', dict(w_gs=98304, x_gs=3145728, y_gs=4718592)),
    ((256, 256, 1, 2, 2, 2048, 1, 1, None), 'p', dict(shift=T, w_ld=256)),
    ((256, 2048, 1, 2, 2, 2048, 1, 1, None), 'p', dict(shift=T, w_ld=256)),
    ((1024, 256, 1, 2, 2, 2048, 1, 1, None), 'p', dict(shift=T, w_ld=1024)),
    ((256, 384, 1, 8064, 1, 1, 25, 1, ('cell-dgrad', 94, 256)), 'np', dict(w_gs=98304, x_gs=0, y_gs=3096576)),
    ((384, 256, 1, 8064, 1, 1, 25, 1, ('rpn-composite-train', 94, 256)), 'np', dict(w_gs=384, w_ld=9600, x_gs=3096576, y_gs=2064384)),
    ((64, 384, 1, 6400, 1, 1, 1, 1, None), 'np', dict(alpha=2.0, res_ld=448, residual=T, w_ld=64, x_ld=448)),
    ((256, 448, 1, 5418, 1, 1, 25, 1, ('cell-dgrad', 188, 512)), 'np', dict(w_gs=114688, x_gs=0, y_gs=2427264)),
    ((448, 256, 1, 5418, 1, 1, 25, 1, ('rpn-composite-train', 188, 512)), 'np', dict(w_gs=448, w_ld=11200, x_gs=2427264, y_gs=1387008)),
    ((256, 384, 1, 3072, 1, 1, 36, 1, ('wino23', 12, 32)), 'np', dict(w_gs=98304, x_gs=786432, y_gs=1179648)),
    ((512, 512, 1, 3072, 1, 1, 36, 1, ('wino23', 12, 32)), 'np', dict(w_gs=262144, x_gs=1572864, y_gs=1572864)),
    ((256, 384, 1, 2944, 1, 1, 25, 1, ('cell-dgrad', 94, 256)), 'np', dict(w_gs=98304, x_gs=0, y_gs=1130496)),
    ((384, 256, 1, 2944, 1, 1, 25, 1, ('rpn-composite-train', 94, 256)), 'np', dict(w_gs=384, w_ld=9600, x_gs=1130496, y_gs=753664)),
    ((256, 448, 1, 2646, 1, 1, 25, 1, ('cell-dgrad', 188, 512)), 'np', dict(w_gs=114688, x_gs=0, y_gs=1185408)),
    ((448, 256, 1, 2646, 1, 1, 25, 1, ('rpn-composite-train', 188, 512)), 'np', dict(w_gs=448, w_ld=11200, x_gs=1185408, y_gs=677376)),
    ((384, 1, 1, 2048, 1, 1, 1, 1, None), 'np', dict(w_ld=384)),
    ((384, 1024, 1, 2048, 1, 1, 1, 1, None), 'np', dict(w_ld=384)),
    ((1024, 151, 1, 2048, 1, 1, 1, 1, None), 'p', dict(shift=T, w_ld=1024)),
    ((1024, 604, 1, 2048, 1, 1, 1, 1, None), 'p', dict(shift=T, w_ld=1024)),
    ((256, 448, 1, 1978, 1, 1, 25, 1, ('cell-dgrad', 188, 512)), 'np', dict(w_gs=114688, x_gs=0, y_gs=886144)),
    ((448, 256, 1, 1978, 1, 1, 25, 1, ('rpn-composite-train', 188, 512)), 'np', dict(w_gs=448, w_ld=11200, x_gs=886144, y_gs=506368)),
    ((384, 1536, 1, 1536, 1, 1, 128, 1, None), 'np', dict(w_gs=2162688, w_ld=1408, x_gs=589824, x_ld=384, y_gs=2359296)),
    ((512, 1536, 1, 1536, 1, 1, 128, 1, None), 'np', dict(alpha=0.04418913275003433, w_gs=2162688, w_ld=1408, x_gs=2162688, x_ld=1408, y_gs=2359296)),
    ((384, 1, 1, 1024, 1, 1, 1, 1, None), 'np', dict(w_ld=384)),
    ((384, 512, 1, 1024, 1, 1, 1, 1, None), 'np', dict(w_ld=384)),
    ((384, 2048, 1, 1024, 1, 1, 1, 1, None), 'np', dict(w_ld=384)),
    ((256, 448, 1, 966, 1, 1, 25, 1, ('cell-dgrad', 188, 512)), 'np', dict(w_gs=114688, x_gs=0, y_gs=432768)),
    ((448, 256, 1, 966, 1, 1, 25, 1, ('rpn-composite-train', 188, 512)), 'np', dict(w_gs=448, w_ld=11200, x_gs=432768, y_gs=247296)),
    ((384, 1, 1, 512, 1, 1, 1, 1, None), 'np', dict(w_ld=384)),
    ((384, 1024, 1, 512, 1, 1, 1, 1, None), 'np', dict(w_ld=384)),
    ((256, 256, 1, 448, 1, 1, 25, 1, None), 'np', dict(w_gs=65536, x_gs=114688, y_gs=114688)),
    ((256, 256, 1, 384, 1, 1, 25, 1, None), 'np', dict(w_gs=65536, x_gs=98304, y_gs=98304)),
    ((384, 384, 1, 384, 1, 1, 128, 1, None), 'np', dict(w_gs=933888, w_ld=2432, x_gs=147456, x_ld=384, y_gs=147456)),
    ((512, 1, 1, 384, 1, 1, 1, 1, None), 'np', dict(w_ld=512)),
    ((512, 1024, 1, 384, 1, 1, 1, 1, None), 'np', dict(w_ld=512)),
    ((1024, 1, 1, 384, 1, 1, 1, 1, None), 'np', dict(w_ld=1024)),
    ((1024, 1, 1, 384, 1, 1, 1, 1, None), 'np', dict(shift=T, shift_per_row=True)),
    ((1024, 384, 1, 384, 1, 1, 128, 1, None), 'np', dict(alpha=0.03125, w_gs=933888, w_ld=2432, x_gs=933888, x_ld=2432, y_gs=147456)),
    ((1024, 512, 1, 384, 1, 1, 1, 1, None), 'np', dict(w_ld=1024)),
    ((1024, 2048, 1, 384, 1, 1, 1, 1, None), 'np', dict(w_ld=1024)),
    ((2048, 1, 1, 384, 1, 1, 1, 1, None), 'np', dict(shift=T, shift_per_row=True)),
    ((2048, 1024, 1, 384, 1, 1, 1, 1, None), 'np', dict(w_ld=2048)),
    ((256, 384, 1, 256, 1, 1, 25, 1, None), 'np', dict(w_gs=98304, x_gs=65536, y_gs=384, y_ld=9600)),
    ((256, 448, 1, 256, 1, 1, 25, 1, None), 'np', dict(w_gs=114688, x_gs=65536, y_gs=448, y_ld=11200)),
    ((384, 256, 1, 256, 1, 1, 25, 1, None), 'np', dict(w_gs=98304, x_gs=384, x_ld=9600, y_gs=65536)),
    ((448, 256, 1, 256, 1, 1, 25, 1, None), 'np', dict(w_gs=114688, x_gs=448, x_ld=11200, y_gs=65536)),
    ((256, 384, 1, 128, 1, 1, 25, 1, ('cell-dgrad', 94, 256)), 'np', dict(w_gs=98304, x_gs=0, y_gs=49152)),
    ((384, 256, 1, 128, 1, 1, 25, 1, ('rpn-composite-train', 94, 256)), 'np', dict(w_gs=384, w_ld=9600, x_gs=49152, y_gs=32768)),
    ((256, 448, 1, 86, 1, 1, 25, 1, ('cell-dgrad', 188, 512)), 'np', dict(w_gs=114688, x_gs=0, y_gs=38528)),
    ((448, 256, 1, 86, 1, 1, 25, 1, ('rpn-composite-train', 188, 512)), 'np', dict(w_gs=448, w_ld=11200, x_gs=38528, y_gs=22016)),
    ((256, 448, 1, 42, 1, 1, 25, 1, ('cell-dgrad', 188, 512)), 'np', dict(w_gs=114688, x_gs=0, y_gs=18816)),
    ((448, 256, 1, 42, 1, 1, 25, 1, ('rpn-composite-train', 188, 512)), 'np', dict(w_gs=448, w_ld=11200, x_gs=18816, y_gs=10752)),
]
# launches of other kernels in ops.PROFILE (fused Winograd, stem, whole-op brackets, listed pixels): census only
FWD_OTHER = [
    (('wino23', 128, 128, 47, 128, 128), 'np'),
    (('wino23', 256, 256, 24, 64, 128), 'np'),
    (('wino23', 256, 384, 12, 32, 128), 'np'),
    (('wino23', 256, 384, 24, 64, 128), 'np'),
    (('wino23', 256, 384, 47, 128, 128), 'np'),
    (('wino23', 384, 256, 12, 32, 128), 'np'),
    (('wino23', 384, 256, 24, 64, 128), 'np'),
    (('wino23', 384, 256, 47, 128, 128), 'np'),
    (('wino23', 512, 512, 12, 32, 128), 'np'),
    (('wino23-dgrad-rois', 256, 384, 188, 512, 42), 'np'),
    (('wino23-dgrad-rois', 256, 384, 188, 512, 86), 'np'),
    (('wino23-dgrad-rois', 256, 384, 94, 256, 128), 'np'),
    (('wino23-rois', 384, 256, 188, 512, 42), 'np'),
    (('wino23-rois', 384, 256, 188, 512, 86), 'np'),
    (('wino23-rois', 384, 256, 94, 256, 128), 'np'),
    ((1, 64, 7, 375, 1024, 128, 1, 2, None), 'np'),
    ((128, 128, 1, 196608, 1, 1, 16, 1, ('wino23', 47, 128)), 'np'),
    ((256, 256, 1, 49152, 1, 1, 16, 1, ('wino23', 24, 64)), 'np'),
    ((256, 384, 1, S(148), 1, 1, 16, 1, ('wino23-dgrad-rois', 94, 256)), 'p'),
    ((256, 384, 1, S(156160), 1, 1, 16, 1, ('wino23-dgrad-rois', 188, 512)), 'n'),
    ((256, 384, 1, S(1952), 1, 1, 16, 1, ('wino23-dgrad-rois', 94, 256)), 'n'),
    ((256, 384, 1, S(2304), 1, 1, 16, 1, ('wino23-dgrad-rois', 188, 512)), 'p'),
    ((256, 384, 1, S(321024), 1, 1, 16, 1, ('wino23-dgrad-rois', 188, 512)), 'n'),
    ((256, 384, 1, S(3840), 1, 1, 16, 1, ('wino23-dgrad-rois', 188, 512)), 'p'),
    ((384, 256, 1, S(1110), 1, 1, 16, 1, ('wino23-rois', 188, 512)), 'n'),
    ((384, 256, 1, 12288, 1, 1, 16, 1, ('wino23', 12, 32)), 'np'),
    ((384, 256, 1, S(132), 1, 1, 16, 1, ('wino23-rois', 94, 256)), 'p'),
    ((384, 256, 1, S(1648), 1, 1, 16, 1, ('wino23-rois', 94, 256)), 'n'),
    ((384, 256, 1, S(17), 1, 1, 16, 1, ('wino23-rois', 188, 512)), 'p'),
    ((384, 256, 1, 196608, 1, 1, 16, 1, ('wino23', 47, 128)), 'np'),
    ((384, 256, 1, S(2282), 1, 1, 16, 1, ('wino23-rois', 188, 512)), 'n'),
    ((384, 256, 1, S(28), 1, 1, 16, 1, ('wino23-rois', 188, 512)), 'p'),
    ((384, 256, 1, 49152, 1, 1, 16, 1, ('wino23', 24, 64)), 'np'),
    ((512, 512, 1, 12288, 1, 1, 16, 1, ('wino23', 12, 32)), 'np'),
    ((64, 384, 1, 0, 1, 1, 1, 1, ('rows-rois', 188, 512)), 'np'),
]


# ------------------------------------------------------------------------------------------------------- exact-check machinery
GUARD_ROWS = 64                       # NaN rows behind every output
DY = (-0.5, 0.5, 1.0, 2.0)            # dyadic scales
LIMIT = 2 ** 22                       # worst-case |partial sum| in units of the finest term, asserted per entry (fp32: exact below 2^24)


def _gen(seed):
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    return g


def _ints(n, lo, hi, gen):
    return torch.randint(lo, hi + 1, (n,), generator=gen, device='cuda', dtype=torch.int8).float()


def _pick(n, vals, gen):
    return torch.tensor(vals, device='cuda', dtype=torch.float32)[torch.randint(0, len(vals), (n,), generator=gen, device='cuda')]


def _operand(n, amax, gen, randn):
    """`amax` = 1: {-1, 0, 1}; 2: {-2, ..., 2}; randn: standard normal (the precision cases)."""
    if randn:
        return torch.randn((n,), generator=gen, device='cuda', dtype=torch.float32)
    return _ints(n, -amax, amax, gen)


def _span(G, gs, rows, ld, width):
    """Floats an operand of G groups (stride gs) x rows (pitch ld) x width occupies."""
    return (G - 1) * gs + (rows - 1) * ld + width


def _nhwc(flat, G, gs, B, H, W, ld, C):
    return flat.as_strided((G, B, H, W, C), (gs, H * W * ld, W * ld, ld, 1))


def _nan(n):
    return torch.full((n,), float('nan'), device='cuda', dtype=torch.float32)


def _assert_buffer(got, exp, what, bound=None, rms=None):
    """Whole-buffer comparison: NaN exactly where nothing may be written, and every written element equal to the reference
    (bit for bit; with `bound`: |got - ref| <= bound per element)."""
    torch.cuda.synchronize()
    nan_g, nan_e = got.isnan(), exp.isnan()
    if not torch.equal(nan_g, nan_e):
        bad = (nan_g != nan_e).nonzero()
        pytest.fail(f'{what}: {bad.numel()} elements written outside / missing inside the output region, first at flat index '
                    f'{int(bad[0])} (got {float(got[bad[0]])}, expected {float(exp[bad[0]])})')
    if bound is None:
        if not torch.equal(got.nan_to_num(0.0), exp.nan_to_num(0.0)):
            bad = ((got != exp) & ~nan_e).nonzero()
            i = int(bad[0])
            pytest.fail(f'{what}: torch.equal fails, {bad.numel()} of {int((~nan_e).sum())} elements differ, first at flat index {i}: '
                        f'got {float(got[i])}, reference {float(exp[i])}')
    else:
        viol = ((got.double() - exp).abs() > bound) & ~nan_e
        if bool(viol.any()):
            bad = viol.nonzero()
            i = int(bad[0])
            pytest.fail(f'{what}: {bad.numel()} elements outside the rounding bound, first at {i}: got {float(got[i])}, reference '
                        f'{float(exp[i])}, bound {float(bound[i])}')
    if rms is not None:
        K, l2 = rms
        sel = ~nan_e
        e = (got.double() - exp)[sel]
        e_rms = float(e.square().mean().sqrt())
        del e
        lim = _rms_limit(K, float(l2[sel].square().mean().sqrt()), float(exp[sel].square().mean().sqrt()))
        assert e_rms <= lim, f'{what}: rms error {e_rms:.3e} above the fp32 limit {lim:.3e}'


def _bound_ok(what, K, amax, bmax, smax, unit, extra=0.0):
    """Precondition of exactness: worst-case |partial sum| K max|a| max|b| max scale (+ the pre-filled / added terms), in units of the
    finest representable term, below 2^22."""
    worst = (K * amax * bmax * smax + extra) / unit
    assert worst < LIMIT, f'{what}: worst case {worst:.3g} units >= 2^22, the integer operands would not be exact'
    return worst


# Precision bound (randn operands): both kernels sum K products in fp32.  The products are exact in the fma (fp32 kernel) or carry
# <= 3 dropped split terms below 2^-24 of them (split-bf16: x = hi + mid + lo, six of nine products kept); every addition
# rounds to nearest with an error <= 2^-24 of the running |sum| <= abs_ref.  At most K + (pixel splits) + 3 (epilogue: scale, shift,
# residual) roundings reach an element; as independent zero-mean errors, each of variance <= (2^-24 abs_ref)^2 / 3, they sum to a
# standard deviation <= sqrt(K) 2^-24 abs_ref / sqrt(3) (K >= 64 here, so sqrt(K) covers the few extra roundings twice over).  6.5
# standard deviations for ~1e9 elements, doubled for the split form's second error source: c = 2 * 6.5 / sqrt(3) ~ 7.5 -> 8.
PREC_C = 8.0
TINY = 1e-30


def _prec_bound(K, absref):
    return PREC_C * math.sqrt(K) * 2.0 ** -24 * absref + TINY


# The per-element bound above scales with abs_ref ~ K E|ab|: at K = 3 M it admits errors close to |ref| ~ sqrt(K) itself, so on its own it
# only catches bf16-level loss (2^-9 per product) at short K.  The companion is an rms bound in the l2 norm of the products,
# l2 = sqrt(sum_k (a_k b_k)^2) (conv_ref.sq_ref): a sequential fp32 sum whose partial sums s_k have rms ~ sqrt(k / K) l2 rounds with
# errors of rms <= 2^-24 |s_k| / sqrt(3), so the rms error is <= 2^-24 l2 sqrt(sum_k k / K / 3) = 2^-24 l2 sqrt((K + 1) / 6); pixel splits
# and several accumulators only shorten the chains.  Factor 2 for the split form's dropped terms, + 2 roundings of |ref| for the
# epilogue.  A product truncated to bf16 errs by ~2^-9 l2 / sqrt(3): 2^10 times this at K = 64, still ~5 times it at K = 3 M.
def _rms_limit(K, l2_rms, ref_rms):
    return 2.0 ** -24 * (2.0 * math.sqrt((K + 1) / 6.0) * l2_rms + 2.0 * ref_rms)


def _routes(monkeypatch, run):
    """run(route) under NBM_SPLIT_BF16=0 (fp32 matrix instruction) and =1 (split-bf16 where the dispatch takes it)."""
    for route in ('0', '1'):
        monkeypatch.setenv('NBM_SPLIT_BF16', route)
        run(route)
    monkeypatch.delenv('NBM_SPLIT_BF16')


def _free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _expected_bits(y):
    """nbm_gemm_desc.bits_out of y [M, N] (N % 32 == 0): word m * N / 32 + n / 32, bit 8 (n % 4) + (n % 32) / 4, set where y > 0."""
    M, N = y.shape
    b = (y > 0).view(M, N // 32, 8, 4).long()
    w = torch.tensor([[1 << (8 * e + j) for e in range(4)] for j in range(8)], device=y.device, dtype=torch.int64)
    words = (b * w).sum((-1, -2))
    return (words - (words >= 2 ** 31).long() * 2 ** 32).to(torch.int32).reshape(-1)


def _bits_from_forward(mask2d):
    """The ReLU bits of `mask` [M, C] as the forward kernel writes them: a 1x1 launch with identity weights reproduces mask exactly."""
    from birdsoundclassif_amd import ops
    M, C_ = mask2d.shape
    y = torch.empty((M, C_), device='cuda', dtype=torch.float32)
    bits = torch.empty((M * C_ // 32,), device='cuda', dtype=torch.int32)
    ops.gemm_conv(mask2d, torch.eye(C_, device='cuda'), y, B=1, H=M, W=1, Cin=C_, N=C_, bits_out=bits)
    assert torch.equal(y, mask2d)
    assert torch.equal(bits, _expected_bits(mask2d)), 'bits_out of the forward kernel'
    del y
    return bits


# ------------------------------------------------------------------------------------------------------------------ data gradient
def run_dgrad(key, ep, monkeypatch, seed, randn=False):
    from birdsoundclassif_amd import ops
    _, B, H, W, Cin, N, k, stride, G = (int(v) if not isinstance(v, str) else v for v in key)
    pad = (k - 1) // 2
    Ho, Wo = R.out_size(H, W, k, k, stride, pad)
    Mo, Mi = B * Ho * Wo, B * H * W
    g_ld, w_ld, out_ld = ep.get('g_ld', N), ep.get('w_ld', k * k * Cin), ep.get('out_ld', Cin)
    g_gs, w_gs, out_gs = ep.get('g_gs', 0), ep.get('w_gs', 0), ep.get('out_gs', 0)
    if G == 1 and out_ld == Cin:
        out_ld = Cin + 4                                       # a pitch above the width: the 4 columns between rows are guards
    alpha = ep.get('alpha', 1.0)
    gen = _gen(seed)
    g = _operand(_span(G, g_gs, Mo, g_ld, g_ld), 1, gen, randn)
    if g_ld > N:                                              # the zero padding the kernel reads up to ceil(N / 32) * 32
        assert G == 1
        g.view(Mo, g_ld)[:, N:] = 0
    w = _operand(_span(G, w_gs, N, w_ld, w_ld), 2, gen, randn)
    a_scale = _pick(N, DY, gen) if 'a_scale' in ep else None
    mask = _ints(Mi * Cin, -1, 1, gen) if 'mask' in ep else None              # exact zeros and negatives: the `mask <= 0` ties
    residual = _operand(Mi * Cin, 2, gen, randn) if 'residual' in ep else None
    r2 = None
    if 'residual2' in ep:
        r2 = _operand(B * ((H + 1) // 2) * ((W + 1) // 2) * Cin, 2, gen, randn).view(B, (H + 1) // 2, (W + 1) // 2, Cin)
    smin, smax = (0.5, 2.0) if a_scale is not None else (1.0, 1.0)
    K = N * k * k
    if not randn:
        _bound_ok(key, K, 1, 2, smax * abs(alpha), min(1.0, smin * abs(alpha)), extra=4.0)
    gv = _nhwc(g, G, g_gs, B, Ho, Wo, g_ld, N)
    wv = w.as_strided((G, N, k * k * Cin), (w_gs, w_ld, 1))
    kw = dict(H=H, W=W, kh=k, kw=k, stride=stride, pad=pad, a_scale=a_scale, alpha=alpha,
              residual=None if residual is None else residual.view(B, H, W, Cin), residual2=r2,
              mask=None if mask is None else mask.view(B, H, W, Cin))
    ref = R.dgrad(gv, wv, **kw)
    n_out = _span(G, out_gs, Mi, out_ld, out_ld) + GUARD_ROWS * out_ld
    if randn:
        exp = torch.full((n_out,), float('nan'), device='cuda', dtype=torch.float64)
        bnd = torch.zeros((n_out,), device='cuda', dtype=torch.float64)
        _nhwc(exp, G, out_gs, B, H, W, out_ld, Cin).copy_(ref)
        del ref
        _nhwc(bnd, G, out_gs, B, H, W, out_ld, Cin).copy_(_prec_bound(K, R.abs_ref(R.dgrad, gv, wv, **kw)))
        l2 = torch.zeros((n_out,), device='cuda', dtype=torch.float64)
        _nhwc(l2, G, out_gs, B, H, W, out_ld, Cin).copy_(R.sq_ref(R.dgrad, gv, wv, **kw).sqrt())
        rms = (K, l2)
    else:
        exp = _nan(n_out)
        _nhwc(exp, G, out_gs, B, H, W, out_ld, Cin).copy_(ref)
        bnd = rms = None
        del ref
    _free()
    bits = _bits_from_forward(mask.view(Mi, Cin)) if 'mask_bits' in ep else None
    out = _nan(n_out)

    def launch(route, use_bits):
        out.fill_(float('nan'))
        ops.conv_dgrad(g, w, out, B=B, H=H, W=W, Cin=Cin, N=N, kh=k, kw=k, stride=stride, pad=pad, g_ld=g_ld, w_ld=w_ld, out_ld=out_ld,
                       a_scale=a_scale, residual=residual, mask=mask, alpha=alpha, groups=G, g_gs=g_gs, w_gs=w_gs, out_gs=out_gs,
                       residual2=r2, mask_bits=bits if use_bits else None)
        _assert_buffer(out, exp, f'{key} {ep} NBM_SPLIT_BF16={route}{" mask_bits" if use_bits else ""}', bnd, rms)

    def run(route):
        launch(route, False)
        if bits is not None:                                  # the bits and the float mask give the same d/dx, bit for bit
            launch(route, True)
    _routes(monkeypatch, run)
    del g, w, out, exp, bnd, mask, residual, r2, bits, rms
    _free()


# ---------------------------------------------------------------------------------------------------------------- weight gradient
def run_wgrad(key, ep, monkeypatch, seed, randn=False):
    from birdsoundclassif_amd import ops
    _, B, H, W, Cin, N, k, stride, G = (int(v) if not isinstance(v, str) else v for v in key)
    pad = (k - 1) // 2
    Ho, Wo = R.out_size(H, W, k, k, stride, pad)
    Mo, Mi = B * Ho * Wo, B * H * W
    KC = k * k * Cin
    g_ld, x_ld, out_ld = ep.get('g_ld', N), ep.get('x_ld', Cin), ep.get('out_ld', KC)
    g_gs, x_gs, out_gs = ep.get('g_gs', 0), ep.get('x_gs', 0), ep.get('out_gs', 0)
    if G == 1 and out_ld == KC:
        out_ld = KC + 4
    alpha = ep.get('alpha', 1.0)
    K = Mo                                                    # the reduction runs over the output pixels
    # operand ranges: the widest of these whose worst case stays below 2^22 units
    # (alpha and row_scale multiply each chunk's sum before the atomics: the pre-filled partial sum is drawn in units of the finest such
    # product, u = min|row_scale| |alpha|, so that every value the atomics add is an integer multiple of u)
    for xa, scales in ((2, DY), (1, DY), (1, (-1.0, 1.0))):
        smin, smax = (min(abs(s) for s in scales), max(abs(s) for s in scales)) if 'row_scale' in ep else (1.0, 1.0)
        u = smin * abs(alpha)
        if (K * xa * smax * abs(alpha) + 4 * u) / u < LIMIT:
            break
    gen = _gen(seed)
    g = _operand(_span(G, g_gs, Mo, g_ld, g_ld), 1, gen, randn)
    x = _operand(_span(G, x_gs, Mi, x_ld, x_ld), xa, gen, randn)
    row_scale = _pick(N, scales, gen) if 'row_scale' in ep else None
    if not randn:
        _bound_ok(key, K, 1, xa, smax * abs(alpha), u, extra=4.0 * u)
    n_out = _span(G, out_gs, N, out_ld, out_ld) + GUARD_ROWS * out_ld
    dt = torch.float64 if randn else torch.float32
    exp = torch.full((n_out,), float('nan'), device='cuda', dtype=dt)
    ov = exp.as_strided((G, N, KC), (out_gs, out_ld, 1))
    ov.copy_(_operand(G * N * KC, 4, gen, randn).view(G, N, KC) * (1.0 if randn else u))   # pre-filled partial sum: the launch adds
    pre = exp.float().clone()
    bias = _operand(N, 4, gen, randn) if 'bias_grad' in ep else None
    gv = _nhwc(g, G, g_gs, B, Ho, Wo, g_ld, N)
    xv = _nhwc(x, G, x_gs, B, H, W, x_ld, Cin)
    kw = dict(kh=k, kw=k, stride=stride, pad=pad, row_scale=row_scale, alpha=alpha)
    ref, gb_ref = R.wgrad(gv, xv, out=ov.clone(), bias_grad=bias, **kw)
    bnd = gbb = rms = None
    if randn:
        absr, absb = R.wgrad(gv.abs(), xv.abs(), out=ov.abs(), bias_grad=None if bias is None else bias.abs(),
                             **dict(kw, row_scale=None if row_scale is None else row_scale.abs(), alpha=abs(alpha)))
        bnd = torch.zeros((n_out,), device='cuda', dtype=torch.float64)
        bnd.as_strided((G, N, KC), (out_gs, out_ld, 1)).copy_(_prec_bound(K, absr))
        gbb = None if absb is None else _prec_bound(K, absb.reshape(-1))
        del absr
        sq, _ = R.wgrad(gv.square(), xv.square(), out=ov.square(), **dict(kw, row_scale=None if row_scale is None else row_scale.square(),
                                                                         alpha=alpha * alpha))
        l2 = torch.zeros((n_out,), device='cuda', dtype=torch.float64)
        l2.as_strided((G, N, KC), (out_gs, out_ld, 1)).copy_(sq.sqrt())
        rms = (K, l2)
        del sq
    ov.copy_(ref)
    del ref
    _free()
    out = pre.clone()

    def run(route):
        out.copy_(pre)
        bg = None if bias is None else bias.clone()
        ops.conv_wgrad(g, x, out, B=B, H=H, W=W, Cin=Cin, N=N, kh=k, kw=k, stride=stride, pad=pad, g_ld=g_ld, x_ld=x_ld, out_ld=out_ld,
                       row_scale=row_scale, alpha=alpha, groups=G, g_gs=g_gs, x_gs=x_gs, out_gs=out_gs, bias_grad=bg)
        what = f'{key} {ep} NBM_SPLIT_BF16={route}'
        _assert_buffer(out, exp, what, bnd, rms)
        if bias is not None:
            _assert_buffer(bg, gb_ref.reshape(-1).to(dt), what + ' bias_grad', gbb)
    _routes(monkeypatch, run)
    del g, x, out, exp, pre, bnd, rms
    _free()


# -------------------------------------------------------------------------------------------------------------------- forward
def run_fwd(key, ep, monkeypatch, seed, randn=False):
    from birdsoundclassif_amd import ops
    Cin, N, kh, H, W, B, G, stride = (int(v) for v in key[:8])
    label = key[8]
    kw_ = 1 if (label is not None and label[0] == 'rpn-composite-train' and kh == 5) else kh   # the 5-plane composite: a kh x 1 filter
    pad = 0 if kw_ != kh else (kh - 1) // 2
    Ho, Wo = R.out_size(H, W, kh, kw_, stride, pad)
    Mo, Mi = B * Ho * Wo, B * H * W
    KC = kh * kw_ * Cin
    x_ld, w_ld, y_ld = ep.get('x_ld', Cin), ep.get('w_ld', KC), ep.get('y_ld', N)
    x_gs, w_gs, y_gs = ep.get('x_gs', 0), ep.get('w_gs', 0), ep.get('y_gs', 0)
    if G == 1 and y_ld == N:
        y_ld = N + 4
    alpha = ep.get('alpha', 1.0)
    if alpha != 2.0 ** round(math.log2(abs(alpha))):
        alpha = 0.5                                           # the attention's 1 / sqrt(d): not dyadic, the launch is the same
    per_row = ep.get('shift_per_row', False)
    relu = ep.get('act', 0) == 1
    gen = _gen(seed)
    x = _operand(_span(G, x_gs, Mi, x_ld, x_ld), 1, gen, randn)
    w = _operand(_span(G, w_gs, N, w_ld, w_ld), 2, gen, randn)
    scale = _pick(N, DY, gen) if 'scale' in ep else None
    shift = _operand(Mo if per_row else N, 2, gen, randn) if 'shift' in ep else None
    res_ld = ep.get('res_ld', N)
    residual = _operand(Mo * res_ld, 2, gen, randn) if 'residual' in ep else None
    smin, smax = (0.5, 2.0) if scale is not None else (1.0, 1.0)
    if not randn:
        _bound_ok(key, KC, 1, 2, smax * abs(alpha), min(1.0, smin * abs(alpha)), extra=4.0)
    xv = _nhwc(x, G, x_gs, B, H, W, x_ld, Cin)
    wv = w.as_strided((G, N, KC), (w_gs, w_ld, 1))
    kw = dict(kh=kh, kw=kw_, stride=stride, pad=pad, Ho=Ho, Wo=Wo, scale=scale, alpha=alpha,
              shift=None if shift is None else (shift.view(B, Ho, Wo, 1) if per_row else shift),
              residual=None if residual is None else residual.view(B, Ho, Wo, res_ld)[..., :N])
    up = None
    if 'up' in ep and randn:                                   # the top-down merge: a coarse map of half the size, bilinear
        uh, uw = (Ho + 1) // 2, (Wo + 1) // 2
        up = _operand(B * uh * uw * N, 2, gen, randn).view(B, uh, uw, N)
        assert not relu and G == 1
        bil = lambda u: torch.nn.functional.interpolate(u.double().permute(0, 3, 1, 2), size=(Ho, Wo), mode='bilinear',
                                                        align_corners=True).permute(0, 2, 3, 1)
        kw['residual'] = bil(up) + (0 if kw['residual'] is None else kw['residual'].double())
    ref = R.conv(xv, wv, relu=relu, **kw)
    n_out = _span(G, y_gs, Mo, y_ld, y_ld) + GUARD_ROWS * y_ld
    want_bits = 'bits_out' in ep and not randn
    ebits = _expected_bits(ref.reshape(Mo, N).float()) if want_bits else None
    if randn:
        exp = torch.full((n_out,), float('nan'), device='cuda', dtype=torch.float64)
        bnd = torch.zeros((n_out,), device='cuda', dtype=torch.float64)
        _nhwc(exp, G, y_gs, B, Ho, Wo, y_ld, N).copy_(ref)
        del ref
        if up is not None:
            kw['residual'] = bil(up.abs()) + (0 if residual is None else residual.view(B, Ho, Wo, res_ld)[..., :N].abs())
        _nhwc(bnd, G, y_gs, B, Ho, Wo, y_ld, N).copy_(_prec_bound(KC, R.abs_ref(R.conv, xv, wv, **kw)))
        if up is not None:
            kw['residual'] = bil(up.square()).sqrt() + (0 if residual is None else residual.view(B, Ho, Wo, res_ld)[..., :N].abs())
        l2 = torch.zeros((n_out,), device='cuda', dtype=torch.float64)
        _nhwc(l2, G, y_gs, B, Ho, Wo, y_ld, N).copy_(R.sq_ref(R.conv, xv, wv, **kw).sqrt())
        rms = (KC, l2)
    else:
        exp = _nan(n_out)
        _nhwc(exp, G, y_gs, B, Ho, Wo, y_ld, N).copy_(ref)
        bnd = rms = None
        del ref
    _free()
    y = _nan(n_out)
    bits = torch.empty((Mo * N // 32,), device='cuda', dtype=torch.int32) if want_bits else None

    def run(route):
        y.fill_(float('nan'))
        ops.gemm_conv(x, w, y, B=B, H=H, W=W, Cin=Cin, N=N, kh=kh, kw=kw_, stride=stride, pad=pad, Ho=Ho, Wo=Wo, x_ld=x_ld, w_ld=w_ld,
                      y_ld=y_ld, scale=scale, shift=shift, residual=residual, res_ld=res_ld, groups=G, x_gs=x_gs, w_gs=w_gs, y_gs=y_gs,
                      alpha=alpha, act=ops.ACT_RELU if relu else ops.ACT_NONE, shift_per_row=per_row, bits_out=bits, up=up)
        what = f'{key} {ep} NBM_SPLIT_BF16={route}'
        _assert_buffer(y, exp, what, bnd, rms)
        if want_bits:
            assert torch.equal(bits, ebits), what + ': bits_out'
    _routes(monkeypatch, run)
    del x, w, y, exp, bnd, residual, bits, ebits, rms, up
    _free()


# ------------------------------------------------------------------------------------------------------------------------ census
def _norm(key):
    return tuple(int(v) if torch.is_tensor(v) else v for v in key)


def _match(table_key, key):
    return len(table_key) == len(key) and all(isinstance(t, S) or t == v for t, v in zip(table_key, key))


CENSUS = {}        # table key with S(.) dimensions -> the key the census step recorded (the exact checks run that size)


def _resolved(key):
    return CENSUS.get(key, key)


def _census_diff(table, recorded):
    missing = [t for t in table if not any(_match(t, r) for r in recorded)]
    extra = [r for r in recorded if not any(_match(t, r) for t in table)]
    return missing, extra


def test_census_of_a_b128_step_equals_the_table():
    """One positive and one negative B = 128 step (built as test_gpu_fullsize / scripts/trainlayers.py do) with ops.PROFILE and
    ops.PROFILE_BWD on: the recorded launch keys of each step are the table's, no more, no fewer."""
    from birdsoundclassif_amd import ops, synth, train as TR
    from birdsoundclassif_amd.nets import build_model
    from helpers import filler_state_dict
    args = TR.default_args(device='cuda')
    model, crit = build_model(args)
    model.load_state_dict(filler_state_dict())
    model = model.cuda().train()
    crit.train()
    opt, _ = TR.build_optimizer(model, args)
    img8, neg8 = torch.from_numpy(synth.image_batch(0, 8)), torch.from_numpy(synth.image_batch(100, 8))
    bb8, ids8, len8 = synth.label_batch(0, 8)
    tile = lambda t, k: torch.cat([t] * k, 0) if torch.is_tensor(t) else list(t) * k
    batch = [tile(img8, 16), tile(neg8, 16), tile(bb8, 16), tile(ids8, 16), tile(len8, 16)]
    problems = []
    try:
        for step, neg in (('p', False), ('n', True)):
            ops.PROFILE, ops.PROFILE_BWD = [], []
            np.random.seed(77)
            TR.train_one_step(model, crit, opt, batch, args.clip_max_norm, 'cuda', negative_sample=neg)
            torch.cuda.synchronize()
            fwd = {_norm(e[0]) for e in ops.PROFILE}
            bwd = {_norm(e[0]) for e in ops.PROFILE_BWD}
            ops.PROFILE, ops.PROFILE_BWD = None, None
            for name, table, rec in (('backward', [k for k, st, _ in BWD if step in st], bwd),
                                     ('forward', [k for k, st, _ in FWD if step in st] + [k for k, st in FWD_OTHER if step in st], fwd)):
                missing, extra = _census_diff(table, rec)
                for t in table:
                    if any(isinstance(v, S) for v in t):
                        hit = [r for r in rec if _match(t, r)]
                        if len(hit) == 1:
                            CENSUS[t] = hit[0]
                if missing or extra:
                    problems.append(f'{"positive" if step == "p" else "negative"} step, {name}: in the table but not launched {missing}; '
                                    f'launched but not in the table {extra}')
    finally:
        ops.PROFILE, ops.PROFILE_BWD = None, None
        del model, crit, opt
        _free()
    assert not problems, '\n'.join(problems)


# --------------------------------------------------------------------------------------------------------------------- exact
def _ids(entries):
    return [f'{k}-{"+".join(sorted(e))}' if e else f'{k}' for k, _, e in entries]


@pytest.mark.parametrize('i', range(len(BWD)), ids=_ids(BWD))
def test_exact_backward_launch(i, monkeypatch):
    key, _, ep = BWD[i]
    key = _resolved(key)
    (run_dgrad if key[0] == 'dgrad' else run_wgrad)(key, ep, monkeypatch, seed=1000 + i)


@pytest.mark.parametrize('i', range(len(FWD)), ids=_ids(FWD))
def test_exact_forward_launch(i, monkeypatch):
    """The forward implicit-GEMM launches.  The top-down merge operand `up` of the FPN laterals is left out here (its bilinear
    weights are not dyadic; tests/test_gpu_split.py checks it); the attention's 1 / sqrt(d) alpha is replaced by 0.5."""
    key, _, ep = FWD[i]
    key = _resolved(key)
    run_fwd(key, ep, monkeypatch, seed=2000 + i)


# ----------------------------------------------------------------------------------------------------------------- precision
def _entry(table, key, **need):
    for k, _, ep in table:
        if k == key and all((n in ep) == v for n, v in need.items()):
            return k, ep
    raise KeyError(key)


PRECISION = [   # one case per kernel family at its largest table shape: (table, key, required epilogue operands)
    ('fwd', (64, 256, 1, 94, 256, 128, 1, 1, None), dict(residual=True)),           # short-K forward, residual + ReLU epilogue
    ('fwd', (64, 64, 3, 94, 256, 128, 1, 1, None), {}),                             # 3x3 forward
    ('fwd', (2048, 2432, 1, 49152, 1, 1, 1, 1, None), {}),                          # deep-K forward (the split-bf16 instantiation)
    ('fwd', (256, 448, 1, 132096, 1, 1, 25, 1, ('cell-dgrad', 188, 512)), {}),      # grouped cell-domain product
    ('bwd', ('dgrad', 128, 94, 256, 256, 384, 1, 1, 1), {}),                        # deep-K 1x1 data gradient
    ('bwd', ('dgrad', 128, 94, 256, 64, 64, 3, 1, 1), {}),                          # 3x3 data gradient
    ('bwd', ('dgrad', 128, 94, 256, 128, 128, 3, 2, 1), {}),                        # stride-2 data gradient (parity classes)
    ('bwd', ('wgrad', 128, 94, 256, 256, 384, 1, 1, 1), {}),                        # 1x1 weight gradient at 3.08 M rows
    ('bwd', ('wgrad', 128, 94, 256, 64, 64, 3, 1, 1), {}),                          # 3x3 weight gradient
    ('bwd', ('wgrad', 1, 132096, 1, 448, 256, 1, 1, 25), {}),                       # the 448-column split of the fp32 weight gradient
]


@pytest.mark.parametrize('i', range(len(PRECISION)), ids=[repr(p[1]) for p in PRECISION])
def test_precision_at_the_real_shape(i, monkeypatch):
    """randn operands: |got - ref| <= 8 sqrt(K) 2^-24 abs_ref + 1e-30 per element (PREC_C above), for the fp32 and the split-bf16
    route alike (DESIGN 4e claims fp32 accuracy for the latter)."""
    which, key, need = PRECISION[i]
    if which == 'fwd':
        k, ep = _entry(FWD, key, **need)
        run_fwd(k, ep, monkeypatch, seed=3000 + i, randn=True)
    else:
        k, ep = _entry(BWD, key, **need)
        (run_dgrad if k[0] == 'dgrad' else run_wgrad)(k, ep, monkeypatch, seed=3000 + i, randn=True)


# ------------------------------------------------------------------------------------- Winograd, stem and max-pool at B = 128
# The F(2x2, 3x3) forward is exact on integer operands: its constants (WG2 in csrc/winograd.hip and the integer input / output
# transforms of csrc/wino_fused.hip) are dyadic.  F(4x4, 3x3) (the backward convolutions, WINO_BWD_TILE = 4) is not: its input
# transform W43_BT holds 1/3, 1/6, 5/6, 16/15, 1/30, so those paths get the precision check against a float64 run of the same
# transforms.  The cell-domain planes (csrc/cellwino.hip) likewise: CE is integer but CV holds 2/3, 1/12, 1/24; their 25 grouped
# GEMMs are table entries above.
WINO_FWD = [(128, 128, 47, 128), (256, 256, 24, 64), (512, 512, 12, 32)]        # ('wino23', C, N, H, W, B = 128) of the table


def _krsc(w):
    N, C_ = w.shape[:2]
    return w.permute(0, 2, 3, 1).reshape(N, 9 * C_)


@pytest.mark.parametrize('C_,N,H,W', WINO_FWD)
def test_exact_winograd_f2_forward(C_, N, H, W, monkeypatch):
    """conv3x3_winograd(m = 2) as the bottleneck's conv2 calls it (scale, bias, ReLU) at B = 128, and once more with the batch cut
    into three chunks (WINO_CHUNK_BYTES), the last one short: bit for bit the direct convolution."""
    from birdsoundclassif_amd import ops
    B = 128
    gen = _gen(4000 + C_)
    x = _ints(B * H * W * C_, -1, 1, gen).view(B, H, W, C_)
    w = _ints(N * C_ * 9, -2, 2, gen).view(N, C_, 3, 3)
    scale, bias = _pick(N, DY, gen), _ints(N, -2, 2, gen)
    # |V| <= 2 * 2 max|x|, |U| <= 1.5 * 1.5 max|w| in units of 1/4, output transform rows sum to <= 3 in magnitude
    _bound_ok(('wino23', C_, N, H, W), C_, 4, 4.5, 9 * 2.0, 0.25 * 0.5, extra=2.0)
    ref = R.conv(x, _krsc(w), kh=3, kw=3, pad=1, scale=scale, shift=bias, relu=True).float()
    U = ops.wino_weight(w, m=2)
    y = ops.conv3x3_winograd(x, U, bias, m=2, scale=scale, relu=True)
    torch.cuda.synchronize()
    assert torch.equal(y, ref), f'{int((y != ref).sum())} elements differ'
    per_img = 4 * (-(-H // 2)) * (2 * (-(-W // 2)) + 2) * C_ * 4
    monkeypatch.setattr(ops, 'WINO_CHUNK_BYTES', per_img * 47)                # chunks of 47, 47, 34 images
    y = ops.conv3x3_winograd(x, U, bias, m=2, scale=scale, relu=True)
    torch.cuda.synchronize()
    assert torch.equal(y, ref), f'chunked: {int((y != ref).sum())} elements differ'
    del x, y, ref, U
    _free()


_W43_BT = [[1, -1.5, -2, 1.5, 1, 0], [0, -1 / 3, 1 / 6, 5 / 6, 1 / 3, 0], [0, -1 / 3, 5 / 6, -1 / 6, -1 / 3, 0],
           [0, 32 / 15, 16 / 15, -32 / 15, -16 / 15, 0], [0, 1 / 30, -1 / 15, -1 / 30, 1 / 15, 0], [0, 1, -1.5, -2, 1.5, 1]]
_W43_AT = [[1, 1, 1, 1, 1, 0], [0, 1, -1, 0.5, -2, 0], [0, 1, 1, 0.25, 4, 0], [0, 1, -1, 0.125, -8, 1]]
_WG4 = [[1, 0, 0], [1, 1, 1], [1, -1, 1], [1, 0.5, 0.25], [1, -2, 4], [0, 0, 1]]


def _f43(device):
    t = lambda m: torch.tensor(m, device=device, dtype=torch.float64)
    return t(_W43_BT), t(_W43_AT), t(_WG4)


def _tiles43(x):
    """x [B, H, W, C] -> the 6 x 6 patches at rows 4 ty - 1 .. 4 ty + 4 (zero padded): [B, TH, TW, C, 6, 6]."""
    B, H, W, C_ = x.shape
    TH, TW = -(-H // 4), -(-W // 4)
    xp = x.new_zeros((B, 4 * TH + 2, 4 * TW + 2, C_))
    xp[:, 1:H + 1, 1:W + 1] = x
    return xp.unfold(1, 6, 4).unfold(2, 6, 4)


def _wino43_input(x, BT):
    """V [36, T, C] = BT d BT^T per tile, float64."""
    d = _tiles43(x.double())
    V = torch.einsum('ij,bywcjk,lk->ilbywc', BT, d, BT)
    return V.reshape(36, -1, x.shape[-1])


def _wino43_conv(x, U, BT, AT, H, W):
    """Float64 F(4x4, 3x3): x [B, H, W, C], U [36, N, C] -> [B, H, W, N] (same transforms as csrc/winograd.hip)."""
    B = x.shape[0]
    TH, TW = -(-H // 4), -(-W // 4)
    M = torch.matmul(_wino43_input(x, BT), U.transpose(1, 2))                   # [36, T, N]
    N = M.shape[-1]
    Y = torch.einsum('ij,jktn,lk->iltn', AT, M.view(6, 6, -1, N), AT)          # [4, 4, T, N]
    Y = Y.view(4, 4, B, TH, TW, N).permute(2, 3, 0, 4, 1, 5).reshape(B, 4 * TH, 4 * TW, N)
    return Y[:, :H, :W]


@pytest.mark.parametrize('C_,N,H,W', WINO_FWD)
def test_precision_winograd_f4_data_gradient(C_, N, H, W):
    """conv3x3_winograd(m = 4) with transposed weights (FrozenBN scale folded) and the producer's ReLU mask, as the bottleneck's
    backward runs it at B = 128: against float64 of the same transforms on the same fp32 weights U, per element within
    8 sqrt(36 C) 2^-24 times the transforms' magnitude sum |AT| (|U| |BT| |g| |BT|^T) |AT|^T; and the float64 direct data gradient
    within the same bound plus the rounding of U (one fp32 rounding: 2^-24 |U|)."""
    from birdsoundclassif_amd import ops
    B = 128
    gen = _gen(5000 + C_)
    g = torch.randn((B, H, W, N), generator=gen, device='cuda')
    w = torch.randn((N, C_, 3, 3), generator=gen, device='cuda')
    scale = _pick(N, DY, gen)
    mask = _ints(B * H * W * C_, -1, 1, gen).view(B, H, W, C_)
    U = ops.wino_weight(w, transposed=True, m=4, scale=scale)                  # [36, C, N]
    gx = ops.conv3x3_winograd(g, U, None, m=4, mask=mask)
    torch.cuda.synchronize()
    BT, AT, _ = _f43('cuda')
    ref = _wino43_conv(g, U.double(), BT, AT, H, W)
    absr = _wino43_conv(g.abs(), U.double().abs(), BT.abs(), AT.abs(), H, W)
    ref = torch.where(mask > 0, ref, ref.new_zeros(()))
    bound = _prec_bound(36 * N, absr) * (mask > 0)
    err = (gx.double() - ref).abs()
    assert bool((err <= bound).all()), f'max err / bound {float((err / (bound + 1e-300)).max()):.3g}'
    assert bool((gx[mask <= 0] == 0).all())
    direct = R.dgrad(g, _krsc(w), H=H, W=W, kh=3, kw=3, pad=1, a_scale=scale, mask=mask)
    assert bool(((gx.double() - direct).abs() <= 2 * bound + 2.0 ** -22 * absr).all()), 'against the direct data gradient'
    del g, w, mask, U, gx, ref, absr, bound, err, direct
    _free()


@pytest.mark.parametrize('C_,N,H,W', WINO_FWD)
def test_precision_winograd_f4_weight_gradient(C_, N, H, W, monkeypatch):
    """conv3x3_winograd_wgrad(m = WINO_BWD_TILE = 4) at B = 128, whole and cut into three batch chunks: dU [36][N][C] against float64
    of the same transforms, per element within 8 sqrt(T) 2^-24 sum_t |dM| |V| (T tiles) + the transforms' own rounding."""
    from birdsoundclassif_amd import ops
    B = 128
    gen = _gen(6000 + C_)
    x = torch.randn((B, H, W, C_), generator=gen, device='cuda')
    g = torch.randn((B, H, W, N), generator=gen, device='cuda')
    BT, AT, _ = _f43('cuda')
    V, Va = _wino43_input(x, BT), _wino43_input(x.abs(), BT.abs())
    A6 = AT.t()                                                                 # dM = AT^T g_tile AT (6 x 6 from 4 x 4)
    TH, TW = -(-H // 4), -(-W // 4)
    gp = g.new_zeros((B, 4 * TH, 4 * TW, N), dtype=torch.float64)
    gp[:, :H, :W] = g
    gt = gp.view(B, TH, 4, TW, 4, N).permute(0, 1, 3, 5, 2, 4)                # [B, TH, TW, N, 4, 4]
    dM = torch.einsum('ij,bywnjk,lk->ilbywn', A6, gt, A6).reshape(36, -1, N)
    dMa = torch.einsum('ij,bywnjk,lk->ilbywn', A6.abs(), gt.abs(), A6.abs()).reshape(36, -1, N)
    ref = torch.matmul(dM.transpose(1, 2), V)
    bound = _prec_bound(36 * V.shape[1], torch.matmul(dMa.transpose(1, 2), Va))
    del V, Va, dM, dMa, gp, gt
    _free()
    for chunks in (1, 3):
        if chunks == 3:
            per_img = 36 * TH * TW * (C_ + N) * 4
            monkeypatch.setattr(ops, 'WINO_CHUNK_BYTES', per_img * 47)          # 47, 47, 34 images
        dU, _ = ops.conv3x3_winograd_wgrad(x, g, m=4)
        torch.cuda.synchronize()
        err = (dU.double() - ref).abs()
        assert bool((err <= bound).all()), f'{chunks} chunk(s): max err / bound {float((err / bound).max()):.3g}'
    del x, g, ref, bound, dU, err
    _free()


def test_stem_weight_gradient_at_b128(monkeypatch):
    """stem7x7_wgrad at B = 128 on 375 x 1024 images (g [128, 188, 512, 64]: 3.15 GB): U = sum g x under every 7x7 / stride-2 / pad-3 tap and
    V = the same over the inside-the-image indicator, exact on integers.  g has a quarter of its elements non-zero: the worst case is the
    number of non-zeros (counted, not estimated), below 2^22."""
    from birdsoundclassif_amd import ops
    B, H, W = 128, 375, 1024
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    gen = _gen(7000)
    img = _ints(B * H * W, -1, 1, gen).view(B, H, W, 1)
    g = _ints(B * Ho * Wo * 64, -1, 1, gen)
    g *= (torch.rand(g.shape, generator=gen, device='cuda') < 0.25)
    g = g.view(B, Ho, Wo, 64)
    nnz = int((g != 0).sum(dim=(0, 1, 2)).max())
    _bound_ok('stem7x7_wgrad', nnz, 1, 1, 1, 1)
    U, V = ops.stem7x7_wgrad(img, g)
    torch.cuda.synchronize()
    Ur, _ = R.wgrad(g, img, kh=7, kw=7, stride=2, pad=3)
    Vr, _ = R.wgrad(g, torch.ones_like(img), kh=7, kw=7, stride=2, pad=3)
    assert torch.equal(U.reshape(64, 49), Ur.float()), f'U: {int((U.reshape(64, 49) != Ur.float()).sum())} of 3136 differ'
    assert torch.equal(V.reshape(64, 49), Vr.float()), f'V: {int((V.reshape(64, 49) != Vr.float()).sum())} of 3136 differ'
    # precision: randn image and gradient, the same two sums (K = 4.9 M pixels per channel)
    img = torch.randn((B, H, W, 1), generator=gen, device='cuda')
    g = torch.randn((B, Ho, Wo, 64), generator=gen, device='cuda')
    U, V = ops.stem7x7_wgrad(img, g)
    torch.cuda.synchronize()
    K = B * Ho * Wo
    for got, x in ((U, img), (V, torch.ones_like(img))):
        ref, _ = R.wgrad(g, x, kh=7, kw=7, stride=2, pad=3)
        absr, _ = R.wgrad(g.abs(), x.abs(), kh=7, kw=7, stride=2, pad=3)
        l2, _ = R.wgrad(g.double().square(), x.double().square(), kh=7, kw=7, stride=2, pad=3)
        e = (got.reshape(64, 49).double() - ref)
        assert bool((e.abs() <= _prec_bound(K, absr)).all())
        assert float(e.square().mean().sqrt()) <= _rms_limit(K, float(l2.mean().sqrt()), float(ref.square().mean().sqrt()))
    del img, g, U, V
    _free()


def test_maxpool_backward_at_b128():
    """maxpool3x3s2_bwd with `residual` and `mask` at the stem's size (x [128, 188, 512, 64]): gx = scatter of gy to the argmax of every
    window (the forward's index) + residual, zeroed where mask <= 0 -- exact on integers (each pixel sums <= 4 windows)."""
    from birdsoundclassif_amd import ops
    B, H, W, C_ = 128, 188, 512, 64
    gen = _gen(8000)
    x = torch.randn((B, H, W, C_), generator=gen, device='cuda')
    y, idx = ops.maxpool3x3s2(x, with_index=True)
    Ho, Wo = y.shape[1:3]
    gy = _ints(B * Ho * Wo * C_, -2, 2, gen).view(B, Ho, Wo, C_)
    res = _ints(B * H * W * C_, -2, 2, gen).view(B, H, W, C_)
    mask = _ints(B * H * W * C_, -1, 1, gen).view(B, H, W, C_)
    gx = ops.maxpool3x3s2_bwd(idx, gy, H, W, residual=res, mask=mask)
    torch.cuda.synchronize()
    bb = torch.arange(B, device='cuda').view(B, 1, 1, 1)
    oy = torch.arange(Ho, device='cuda').view(1, Ho, 1, 1)
    ox = torch.arange(Wo, device='cuda').view(1, 1, Wo, 1)
    cc = torch.arange(C_, device='cuda').view(1, 1, 1, C_)
    il = idx.long()
    iy, ix = 2 * oy - 1 + il // 3, 2 * ox - 1 + il % 3
    assert bool(((iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)).all()), 'window index outside the image'
    flat = ((bb * H + iy) * W + ix) * C_ + cc
    del iy, ix, il
    assert torch.equal(x.reshape(-1)[flat.reshape(-1)].view_as(y), y), 'idx does not point at the maximum'
    ref = res.double().reshape(-1).index_put_((flat.reshape(-1),), gy.double().reshape(-1), accumulate=True).view(B, H, W, C_)
    ref = torch.where(mask > 0, ref, ref.new_zeros(()))
    assert torch.equal(gx, ref.float()), f'{int((gx != ref.float()).sum())} elements differ'
    del x, y, idx, gy, res, mask, gx, ref, flat
    _free()


@pytest.mark.parametrize('key', [(256, 384, 1, 94, 256, 128, 1, 1, None), (1024, 384, 1, 24, 64, 128, 1, 1, None)])
def test_precision_lateral_with_topdown_merge(key, monkeypatch):
    """The FPN lateral launches with the `up` operand at their real shape (randn; the bilinear weights are not dyadic, so no exact
    case): y = alpha conv + shift (+ residual) + bilinear(up) (align corners), per element and rms as the other precision cases."""
    k, ep = _entry(FWD, key)
    run_fwd(k, ep, monkeypatch, seed=9000 + key[0], randn=True)
