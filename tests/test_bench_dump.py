"""CPU: `bench.py --dump-outputs DIR` -- the per-clip detection dictionaries of the timed path's last step as float rows, the
64 MB cap (a fixed, seeded sample of the rows), and the arguments that reach the timed loop."""
import numpy as np
import pytest
import torch

import bench


def _dets():
    empty = dict(bbox_coord=torch.Tensor(), scores=torch.Tensor())
    d0 = {'1': dict(bbox_coord=torch.tensor([[1., 2., 30., 40.], [5., 6., 70., 80.]]), scores=torch.tensor([[0.9, 0.4]])),
          '2': empty,
          '3': dict(bbox_coord=torch.tensor([[0., 0., 1023., 374.]]), scores=torch.tensor([[0.25]]))}
    return [d0, {'1': empty, '2': empty, '3': empty}]


def test_detection_rows():
    rows = bench.detection_rows(_dets())
    assert rows.dtype == np.float64 and rows.shape == (3, 7)
    assert rows[:, :2].tolist() == [[0, 1], [0, 1], [0, 3]]
    assert rows[1, 2:6].tolist() == [5, 6, 70, 80] and rows[2, 6] == np.float32(0.25)
    assert bench.detection_rows([{'1': dict(bbox_coord=torch.Tensor(), scores=torch.Tensor())}]).shape == (0, 7)


def test_dump_outputs_writes_and_caps(tmp_path):
    rows = bench.detection_rows(_dets())
    bench.dump_outputs(str(tmp_path / 'a'), {'detections': rows})
    assert np.array_equal(np.load(tmp_path / 'a' / 'detections.npy'), rows)
    big = np.arange(4000 * 7, dtype=np.float64).reshape(4000, 7)
    small = np.arange(10, dtype=np.float32)
    limit = 8 * 7 * 1000
    for d in ('b', 'c'):
        bench.dump_outputs(str(tmp_path / d), {'big': big, 'small': small}, limit=limit)
    got = np.load(tmp_path / 'b' / 'big.npy')
    assert np.array_equal(got, np.load(tmp_path / 'c' / 'big.npy'))             # the same sample on every run
    assert sum((tmp_path / 'b' / f).stat().st_size - 128 for f in ('big.npy', 'small.npy')) <= limit
    assert len(got) > 0 and np.all(np.diff(got[:, 0]) > 0) and np.isin(got, big).all()
    with pytest.raises(TypeError):
        bench.dump_outputs(str(tmp_path / 'd'), {'n': np.arange(3)})


def test_dump_and_steps_arguments():
    a = bench.parse_args(['--steps', '7', '--dump-outputs', 'out'])
    assert a.steps == 7 and a.dump_outputs == 'out'
    assert bench.parse_args([]).dump_outputs is None
    with pytest.raises(SystemExit):
        bench.parse_args(['--steps', '0'])


def test_full_is_opt_in():
    assert bench.parse_args([]).full is False
    assert bench.parse_args(['--full', '--steps', '3']).full is True
