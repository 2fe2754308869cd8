"""CPU: the host side of deterministic mode (ops.set_deterministic / train.py --deterministic) -- the allowlist of atomic
sites, the workspace of the weight gradient's twin against the plan, the args round trip, the refusals and the loud guard."""
import argparse
import ctypes as C
import glob
import json
import os
import re

import pytest

from birdsoundclassif_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ('integer, order-free', 'default path only')


def atomic_sites():
    """{(file, kernel): number of atomicAdd( / unsafeAtomicAdd( calls} over csrc/*.hip."""
    hits = {}
    for path in sorted(glob.glob(os.path.join(ROOT, 'birdsoundclassif_amd', 'csrc', '*.hip'))):
        kernel = None
        for line in open(path):
            m = re.search(r'__global__.*?void\s+(\w+)\s*\(', line)
            if m:
                kernel = m.group(1)
            n = len(re.findall(r'\b(?:unsafeAtomicAdd|atomicAdd)\(', line))
            if n:
                key = (os.path.basename(path), kernel)
                hits[key] = hits.get(key, 0) + n
    return hits


def test_every_atomic_add_of_the_sources_is_in_the_allowlist():
    listed = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'atomic_sites.json')))
    table = {(r['file'], r['kernel']): r for r in listed}
    assert len(table) == len(listed)
    found = atomic_sites()
    assert len(found) > 20
    unlisted = sorted(k for k in found if k not in table)
    assert not unlisted, f'atomicAdd in a kernel that tests/golden/atomic_sites.json does not list: {unlisted}'
    stale = sorted(k for k in table if k not in found)
    assert not stale, f'listed kernels without an atomicAdd: {stale}'
    for key, n in found.items():
        row = table[key]
        assert row['count'] == n, (key, n, row['count'])
        assert row['class'] in CLASSES, row
        if row['class'] == 'default path only':
            assert row['twin'], row                                  # the name of its twin, or why there is none and who refuses
            for name in re.findall(r'\bnbm_\w+_det\b', row['twin']):
                assert name in _lib.SIGNATURES, name
        else:
            assert row['twin'] is None, row


def test_guard_table_names_real_entry_points_and_real_twins():
    for name, twin in ops.ATOMIC_ENTRY_POINTS.items():
        assert name in _lib.SIGNATURES, name
        assert twin in (None, 'desc') or twin in _lib.SIGNATURES, twin
    # every twin the allowlist names is reachable through the table
    listed = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'atomic_sites.json')))
    named = {n for r in listed if r['twin'] for n in re.findall(r'\bnbm_\w+_det\b', r['twin'])}
    assert named <= set(ops.ATOMIC_ENTRY_POINTS.values())


def wgrad_desc(B, H, W, Cin, N, k=1, stride=1, pad=0, groups=1, bias=False, out_ld=None, g_gs=0, x_gs=0, out_gs=0):
    d = _lib.BwdDesc()
    d.g = d.x = d.out = 4096                     # any aligned non-null address: nothing is launched
    d.groups = groups
    d.B, d.H, d.W, d.Cin, d.N = B, H, W, Cin, N
    d.kh = d.kw = k
    d.stride, d.pad = stride, pad
    d.Ho, d.Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    d.g_ld, d.x_ld, d.out_ld = (N + 3) // 4 * 4, Cin, out_ld or k * k * Cin
    d.g_gs, d.x_gs, d.out_gs = g_gs, x_gs, out_gs
    d.alpha = 1.0
    if bias:
        d.bias_grad = 4096
    return d


# the shapes of tests/test_gpu_deterministic_kernels.py
WGRAD_SHAPES = {
    '1x1': dict(B=2, H=47, W=128, Cin=64, N=64),
    '3x3-s2-odd': dict(B=2, H=23, W=31, Cin=32, N=32, k=3, stride=2, pad=1),
    'generic-cin3': dict(B=2, H=47, W=128, Cin=3, N=32, k=3, pad=1),
    'n17-bias': dict(B=2, H=47, W=128, Cin=64, N=17, bias=True),
    'groups2': dict(B=1, H=2 * 47 * 128, W=1, Cin=32, N=32, groups=2, g_gs=2 * 47 * 128 * 32, x_gs=2 * 47 * 128 * 32, out_gs=32 * 32),
}


@pytest.mark.parametrize('name', list(WGRAD_SHAPES))
def test_wgrad_workspace_is_splits_times_the_slice(name):
    kw = WGRAD_SHAPES[name]
    d = wgrad_desc(**kw)
    plan = ops.gemm_plan(2, d)
    assert plan.rc == 0 and plan.splits >= 2, plan
    nbytes, stride = ops.wgrad_workspace(d)
    # the rows at their own pitch (taps * Cin, rounded up to 4 floats; = out_ld for these shapes but the 27 columns of the Cin = 3 one)
    ld = (d.kh * d.kw * d.Cin + 3) // 4 * 4
    assert ld == (d.out_ld + 3) // 4 * 4
    assert stride == d.groups * d.N * ld + ((d.groups * d.N + 3) // 4 * 4 if kw.get('bias') else 0)
    assert nbytes == plan.splits * stride * 4
    # the plan with the twin selected is the default plan here (the 1 GiB ceiling is far away): same kernel, grid and splits
    d.workspace, d.ws_split_stride, d.workspace_bytes = 4096, stride, nbytes
    assert ops.gemm_plan(2, d) == plan


def test_wgrad_workspace_is_zero_for_one_split_and_reports_the_entry_points_error():
    d = wgrad_desc(1, 8, 8, 64, 64)
    assert ops.gemm_plan(2, d).splits == 1
    assert ops.wgrad_workspace(d)[0] == 0
    d = wgrad_desc(1, 8, 8, 64, 64, bias=True)                 # a riding bias gradient is summed by several threads: it needs its slice
    assert ops.wgrad_workspace(d)[0] == 1 * (64 * 64 + 64) * 4
    bad = wgrad_desc(2, 47, 128, 64, 64)
    bad.g_ld = 62                                                # not a multiple of 4
    nbytes, stride = C.c_int64(0), C.c_int64(0)
    rc = ops.lib().nbm_conv_wgrad_workspace(C.byref(bad), C.byref(nbytes), C.byref(stride))
    assert rc == ops.gemm_plan(2, bad).rc == -2
    bad = wgrad_desc(2, 47, 128, 64, 64)
    bad.x = None
    assert ops.lib().nbm_conv_wgrad_workspace(C.byref(bad), C.byref(nbytes), C.byref(stride)) == ops.gemm_plan(2, bad).rc == -1


def test_wgrad_slices_do_not_depend_on_the_pitch_of_out():
    """`out` as a column slice of a much wider matrix (the attention's dV' inside the fused projection's gradient, one group per image):
    the slices hold the rows at their own pitch, so the workspace is that of the same GEMM into a matrix of its own."""
    wide = wgrad_desc(1, 1536, 1, 384, 1536, groups=128, out_ld=1408, g_gs=1536 * 1536, x_gs=1536 * 384, out_gs=1536 * 1408)
    own = wgrad_desc(1, 1536, 1, 384, 1536, groups=128, g_gs=1536 * 1536, x_gs=1536 * 384, out_gs=1536 * 384)
    assert ops.wgrad_workspace(wide) == ops.wgrad_workspace(own)
    nbytes, stride = ops.wgrad_workspace(wide)
    assert stride == 128 * 1536 * 384 and nbytes in (0, ops.gemm_plan(2, wide).splits * stride * 4) and nbytes <= 1 << 30


def test_det_workspace_sizes_and_errors():
    assert ops._det_bytes(ops.DET_COLSUM, 100003, 18) == 1024 * 18 * 8
    assert ops._det_bytes(ops.DET_COLSUM, 5, 18) == 2 * 18 * 8
    assert ops._det_bytes(ops.DET_SQNORM, 1000003) == 2048 * 8
    assert ops._det_bytes(ops.DET_BN, 4099, 12) == 1024 * 12 * 16
    assert ops._det_bytes(ops.DET_DWCONV, 2 * 13 * 17, 16) == 111 * 16 * 40
    n = C.c_int64(0)
    assert ops.lib().nbm_det_workspace(9, 10, 10, C.byref(n)) == -1
    assert ops.lib().nbm_det_workspace(0, 0, 10, C.byref(n)) == -1
    assert ops.lib().nbm_stem7x7_wgrad_workspace(2, 64, 96, C.byref(n)) == 0 and n.value == (2 * 32 * 4096 + 8 * 2 * 64 * 49) * 4


def test_args_round_trip_and_old_args_files_load_as_off():
    from birdsoundclassif_amd import train as T
    assert T.get_args_parser().parse_args([]).deterministic is False
    args = T.get_args_parser().parse_args(['--deterministic'])
    assert args.deterministic is True and T.wants_deterministic(args)
    stored = json.loads(json.dumps({k: v for k, v in args.__dict__.items() if isinstance(v, (int, float, str, bool, type(None)))}))
    assert T.wants_deterministic(argparse.Namespace(**stored))
    del stored['deterministic']                                 # an `args` file from before the flag
    assert not T.wants_deterministic(argparse.Namespace(**stored))
    assert T.default_args(device='cpu').deterministic is False


def test_state_functions_context_manager_and_torch_state():
    import torch
    assert not ops.deterministic()
    before = torch.are_deterministic_algorithms_enabled()
    from birdsoundclassif_amd import ondemand
    split = ondemand.UPBWD_SPLIT
    with ops.set_deterministic(True):
        assert ops.deterministic() and torch.are_deterministic_algorithms_enabled() and ondemand.UPBWD_SPLIT is False
        with ops.set_deterministic(True):                       # nested: a no-op that leaves the mode on
            assert ops.deterministic()
        assert ops.deterministic()
    assert not ops.deterministic() and torch.are_deterministic_algorithms_enabled() == before and ondemand.UPBWD_SPLIT == split
    ops.set_deterministic(True)
    ops.set_deterministic(False)
    assert not ops.deterministic() and torch.are_deterministic_algorithms_enabled() == before


def test_split_bf16_is_refused_by_name(monkeypatch):
    monkeypatch.setenv('NBM_SPLIT_BF16', '1')
    with pytest.raises(ValueError, match='NBM_SPLIT_BF16=1'):
        ops.set_deterministic(True)
    assert not ops.deterministic()
    # and the twin's plan never takes the split-bf16 kernel, whatever the switch says
    d = wgrad_desc(1, 4096, 1, 256, 256)
    assert ops.gemm_plan(2, d).kernel.startswith('igemm_split_tn_kernel')
    d.workspace, d.ws_split_stride, d.workspace_bytes = 4096, 256 * 256, 1 << 30
    assert ops.gemm_plan(2, d).kernel.startswith('igemm_tn_kernel')


def test_an_entry_point_without_a_twin_raises_before_anything_is_launched():
    with ops.set_deterministic(True):
        for name, twin in ops.ATOMIC_ENTRY_POINTS.items():
            if twin is None:
                with pytest.raises(RuntimeError, match=f'{name} is not reproducible under --deterministic'):
                    ops._reduction(name, ())
            elif twin == 'desc':                                # covered, but through descriptor fields: not a `_reduction` call
                with pytest.raises(TypeError, match='descriptor fields'):
                    ops._reduction(name, ())


def test_atomic_entry_points_are_only_called_through_the_guarded_wrappers():
    """A direct `lib().nbm_colsum(...)` somewhere in the package would be silently non-reproducible: every call of an entry point of the
    table (and of its twin) sits in ops.py, inside `_reduction`, `roi_tiles`, `conv_wgrad`, `layernorm_bwd` (which routes) or `layernorm_bwd_det`."""
    names = set(ops.ATOMIC_ENTRY_POINTS) | {t for t in ops.ATOMIC_ENTRY_POINTS.values() if t not in (None, 'desc')}
    call = re.compile(r'\.(' + '|'.join(sorted(names, key=len, reverse=True)) + r')\(')
    pkg = os.path.join(ROOT, 'birdsoundclassif_amd')
    direct = {}
    for path in glob.glob(os.path.join(pkg, '**', '*.py'), recursive=True):
        for no, line in enumerate(open(path), 1):
            for m in call.finditer(line):
                direct.setdefault(os.path.relpath(path, pkg), []).append((no, m.group(1)))
    assert set(direct) <= {'ops.py'}, direct
    src = open(os.path.join(pkg, 'ops.py')).read().split('\n')
    allowed = {'nbm_conv_wgrad': 'conv_wgrad', 'nbm_roi_tiles': 'roi_tiles', 'nbm_roi_tiles_det': 'roi_tiles',
               'nbm_layernorm_bwd_det': 'layernorm_bwd_det', 'nbm_layernorm_bwd': 'layernorm_bwd',       # (routes to the twin)
               'nbm_tiles_upsample_bilinear_bwd_add': 'upsample_bilinear_bwd'}     # (raises in deterministic mode before the call)
    for no, name in direct.get('ops.py', []):
        fn = next(l for l in reversed(src[:no]) if l.startswith('def '))
        assert name in allowed and fn.startswith(f'def {allowed[name]}('), (no, name, fn)


def test_a_slice_beyond_the_workspace_ceiling_is_refused_not_run_on_atomics():
    d = wgrad_desc(2, 47, 128, 65536, 4352)                      # 4352 x 65536 floats = 1.06 GiB for one slice
    assert ops.gemm_plan(2, d).rc == 0                           # the default plan is unaffected
    with pytest.raises(_lib.NbmHipError, match='NBM_EUNSUPPORTED'):
        ops.wgrad_workspace(d)
    d.workspace, d.ws_split_stride, d.workspace_bytes = 4096, 4352 * 65536, 1 << 40
    assert ops.gemm_plan(2, d).rc == -3
