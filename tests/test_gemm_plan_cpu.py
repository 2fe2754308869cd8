"""CPU: the launch plan of the three GEMM entry points (csrc/igemm_plan.h through nbm_gemm_plan / ops.gemm_plan) against a recorded table.

tests/golden/gemm_plan.json was recorded from the entry points as they were BEFORE the planner existed (host-only build, every kernel
launch replaced by a recorder): per row a descriptor, the five switches (`sw`: -1 = all unset, else bit i = value of SWITCHES[i]), the
return code and the launches (instantiation, grid, block and the tiling fields of the parameter struct).  It holds every distinct outcome
of a census of a few thousand descriptors -- every kernel instantiation, every NBM_E* return -- and the network's own layers at B = 2 and
64.  A change that moves a layer to another kernel or another grid fails here, without a GPU."""
import json
import os

import pytest

from birdsoundclassif_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ('NBM_STREAM1X1', 'NBM_SPLIT_BF16', 'NBM_H16', 'NBM_NN_H16', 'NBM_SPLIT_TN')
TWO_STAGE = 'igemm_kernel<128,128,64,64,0,0,2,false>'
ROWS = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'gemm_plan.json')))


@pytest.fixture
def switches():
    """set(sw) puts the five switches into the state a row was recorded under; the environment is restored afterwards."""
    was = {n: os.environ.get(n) for n in SWITCHES}

    def set_(sw):
        for i, n in enumerate(SWITCHES):
            if sw < 0:
                os.environ.pop(n, None)
            else:
                os.environ[n] = str((sw >> i) & 1)
    yield set_
    for n, v in was.items():
        if v is None:
            os.environ.pop(n, None)
        else:
            os.environ[n] = v


def descriptor(row):
    d = _lib.GemmDesc() if row['kind'] == 0 else _lib.BwdDesc()
    d.alpha = 1.0
    for k, v in row['desc'].items():
        setattr(d, k, v)
    return d


def test_table_reaches_every_kernel_and_every_error():
    names = {l['name'] for r in ROWS for l in r['launches']}
    assert len(names) == 35                                       # 36 kernel ids; two stream1x1 ids share an instantiation (below)
    assert {(r['kind'], r['rc']) for r in ROWS} == {(0, 0), (0, -1), (0, -2), (0, -3), (1, 0), (1, -1), (1, -2), (1, -3), (2, 0), (2, -1), (2, -2)}
    # the sliced and unsliced forms of stream1x1_kernel<8,2,2,8>
    assert {l['grid'][1] > 1 for r in ROWS for l in r['launches'] if l['name'] == 'stream1x1_kernel<8,2,2,8>'} == {False, True}
    assert any(len(r['launches']) == 2 for r in ROWS if r['kind'] == 0) and any(len(r['launches']) == 2 for r in ROWS if r['kind'] == 2)


def test_plan_equals_the_recorded_launch(switches):
    for i, row in enumerate(ROWS):
        switches(row['sw'])
        p = ops.gemm_plan(row['kind'], descriptor(row))
        what = f'row {i}: kind {row["kind"]} sw {row["sw"]} {row["desc"]}'
        assert p.rc == row['rc'], what
        if p.rc:
            continue
        first = row['launches'][0]                                    # (a width 64 past a multiple of 128: the first of the two calls)
        assert p.halves == (len(row['launches']) == 2), what
        assert (p.kernel, list(p.grid), p.block) == (first['name'], first['grid'], first['block']), what
        for f in ('m_tiles', 'n_tiles', 'vec_epi', 'k_chunk', 'phased', 'plain', 'b_generic'):
            if f in first and not (f == 'n_tiles' and first['name'].startswith('stream1x1')):
                assert getattr(p, f) == first[f], f'{f}: {what}'
        if 'ph_tiles' in first:
            assert list(p.ph_tiles) == first['ph_tiles'], what
        if first['name'].startswith('stream1x1'):
            assert p.slices == first['grid'][1], what
        if row['kind'] == 2:
            assert p.splits == first['grid'][1], what


def test_best_split_against_the_recorded_weight_gradient_splits(switches):
    """Both uses of best_split (512 slots / 8 K-steps per split on the fp32 kernels, 256 slots / 16 x 32 pixels on the split-bf16 kernel):
    splits and k_chunk of every weight-gradient row, and the table must hold rows of both with more than one split."""
    seen = set()
    for row in ROWS:
        if row['kind'] != 2 or row['rc']:
            continue
        switches(row['sw'])
        p = ops.gemm_plan(2, descriptor(row))
        first = row['launches'][0]
        assert (p.splits, p.k_chunk) == (first['grid'][1], first['k_chunk']), row['desc']
        assert p.k_chunk % 32 == 0 and (p.splits - 1) * p.k_chunk < first['M'] <= p.splits * p.k_chunk
        if p.splits > 1:
            seen.add(first['name'].startswith('igemm_split_tn'))
    assert seen == {False, True}


def _aligned(desc):
    return (all(desc.get(k, 0) % 16 == 0 for k in ('x', 'w', 'y', 'scale', 'shift', 'residual', 'up', 'mask')) and
            all(v % 4 == 0 for k, v in desc.items() if k.endswith(('_ld', '_gs'))) and desc['N'] % 4 == 0)


def test_is_deepk_is_the_planners_deep_k_rule(switches):
    """ops.is_deepk (bench.py filters its per-launch timings with it) restates a shape rule; pin it to the planner.  With aligned operands
    and NBM_H16=0 it is exactly "the plan is the two-stage 128 x 128 fast kernel"; under the default switches those launches run on that
    kernel's half-step twin (igemm_h16_kernel: same products, same order) unless the filter has 63 taps or more."""
    n = 0
    for row in ROWS:
        d = row['desc']
        if row['kind'] != 0 or row['rc'] or row['sw'] != -1 or 'rows' in d or not _aligned(d):
            continue
        deep = ops.is_deepk(d['Cin'], d['N'], d['kh'], d['kw'])
        switches(-1)
        assert row['launches'][0]['name'] in (TWO_STAGE, 'igemm_h16_kernel') if deep else row['launches'][0]['name'] not in (TWO_STAGE, 'igemm_h16_kernel'), d
        assert (ops.gemm_plan(0, descriptor(row)).kernel in (TWO_STAGE, 'igemm_h16_kernel')) == deep, d
        os.environ['NBM_H16'] = '0'
        assert (ops.gemm_plan(0, descriptor(row)).kernel == TWO_STAGE) == deep, d
        n += deep
    assert n >= 20


def test_switch_parsing_is_one_rule(switches):
    """A default-on switch is off iff its value begins with '0'; a default-off switch is on iff its value begins with '1'."""
    deep = next(r for r in ROWS if r['kind'] == 0 and r['sw'] == -1 and r['launches'] and r['launches'][0]['name'] == 'igemm_h16_kernel')
    switches(-1)
    for v, kernel in (('0', TWO_STAGE), ('1', 'igemm_h16_kernel'), ('00', TWO_STAGE), ('abc', 'igemm_h16_kernel'), ('', 'igemm_h16_kernel')):
        os.environ['NBM_H16'] = v
        assert ops.gemm_plan(0, descriptor(deep)).kernel == kernel, v
    os.environ.pop('NBM_H16')
    for v, split in (('1', True), ('0', False), ('', False), ('yes', False), ('10', True)):
        os.environ['NBM_SPLIT_BF16'] = v
        assert ops.gemm_plan(0, descriptor(deep)).kernel.startswith('igemm_split_kernel') == split, v
