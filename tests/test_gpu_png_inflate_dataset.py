"""GPU: `Img_dataset(device_inflate=True)` -- workers ship the PNG files' zlib streams and `nbm_png_inflate` inflates
them -- gives bit for bit the batches of the host-inflate route, refuses a damaged file, and drives `train.py`."""
import json
import os
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from birdsoundclassif_amd import synth                                       # noqa: E402
from deflate_writer import H, W, write_png                                    # noqa: E402
from helpers import filler_state_dict                                         # noqa: E402


def write_small_dataset(root):
    """4 positives (two recordings), 3 negatives, 2 hard negatives at 70 x 1024; one file split over several IDAT chunks,
    one written at level 0 (stored blocks)."""
    def u8(i):
        return np.round(synth.image_batch(i, 1, H, W)[0] * 255.0).astype(np.uint8)
    plan = {'recA': [(0, [[40, 5, 160, 40], [500, 20, 620, 60]], [7, 113]), (1, [[300, 12, 420, 50]], [42]),
                     (2, [[10, 10, 60, 30], [700, 8, 800, 66]], [0, 9])],
            'rec__B': [(0, [[100, 20, 230, 60]], [150])]}
    k = 0
    for rec, rows in plan.items():
        d = os.path.join(root, 'positive_files', rec)
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, 'annotations.csv'), 'w') as f:
            f.write('index;coord;bird_id\n')
            for idx, boxes, ids in rows:
                f.write(f'{idx};{boxes};{ids}\n')
                write_png(os.path.join(d, f'{rec}__{idx}.png'), u8(800 + k), idat_split=4096 if k == 1 else None)
                k += 1
    for sub, rec, n, level0 in (('negative_files', 'negA', 2, 1), ('negative_files', 'negB', 1, None), ('hard_neg', 'hardA', 2, None)):
        d = os.path.join(root, sub, rec)
        os.makedirs(d, exist_ok=True)
        for i in range(n):
            write_png(os.path.join(d, f'{rec}__{i}.png'), u8(800 + k), level=0 if i == level0 else 6)
            k += 1


@pytest.fixture(scope='module')
def dataset_root(tmp_path_factory):
    root = tmp_path_factory.mktemp('inflate_dataset')
    write_small_dataset(str(root))
    return str(root)


def _batch(root, order, seed, **kw):
    from birdsoundclassif_amd.nbm_datasets.image_dataset import Img_dataset
    ds = Img_dataset(root, **kw)
    assert len(ds) == 4 and len(ds.negative_files) == 3 and len(ds.hard_negative_files) == 2
    np.random.seed(seed), torch.manual_seed(seed)
    items = [ds.raw_item(i) for i in order]
    return ds.collate(items), items


@pytest.mark.parametrize('kw', [dict(transform=True, host_noise=True), dict(transform=True, host_noise=False),
                                dict(transform=False)], ids=['host_noise', 'device_noise', 'no_transform'])
def test_device_inflate_batches_equal_host_inflate_batches(dataset_root, kw):
    order = (0, 1, 2, 3, 1, 0, 2)
    (img_h, neg_h, bb_h, ids_h, len_h), items_h = _batch(dataset_root, order, 21, **kw)
    (img_d, neg_d, bb_d, ids_d, len_d), items_d = _batch(dataset_root, order, 21, device_inflate=True, **kw)
    assert isinstance(items_h[0]['pos'], np.ndarray) and isinstance(items_d[0]['pos'], tuple)
    assert isinstance(items_d[0]['pos'][0], bytes) and items_d[0]['pos'][1:] == (H, W) and isinstance(items_d[0]['neg'], tuple)
    if kw['transform']:
        assert any('hard' in it for it in items_d) and [it['flags'] for it in items_d] == [it['flags'] for it in items_h]
    assert img_d.is_cuda and img_d.shape == (len(order), H, W)
    assert torch.equal(img_d, img_h) and torch.equal(neg_d, neg_h)
    assert torch.equal(bb_d, bb_h) and torch.equal(ids_d, ids_h) and len_d == len_h


def test_damaged_idat_is_refused_on_both_routes(dataset_root, tmp_path):
    import shutil
    from birdsoundclassif_amd.nbm_datasets.image_dataset import Img_dataset
    root = str(tmp_path / 'damaged')
    shutil.copytree(dataset_root, root)
    victim = os.path.join(root, 'positive_files', 'recA', 'recA__0.png')
    data = bytearray(open(victim, 'rb').read())
    at = data.index(b'IDAT') + 4 + 3000                                       # well inside the zlib stream
    data[at] ^= 0x10
    open(victim, 'wb').write(bytes(data))
    ds = Img_dataset(root, transform=True, device_inflate=True)
    idx = ds.positive_files.index('recA__0.png')
    np.random.seed(1), torch.manual_seed(1)
    items = [ds.raw_item(i) for i in ((idx + 1) % 4, idx)]
    with pytest.raises(ValueError, match='corrupt PNG: positive image of item 1'):
        ds.collate(items)
    with pytest.raises(zlib.error):
        Img_dataset(root, transform=True).raw_item(idx)


def test_train_driver_step_with_device_inflate(tmp_path, monkeypatch):
    """One driver step on the smallest configuration of tests/test_gpu_train_driver.py: the same losses on both routes."""
    from birdsoundclassif_amd import train as T
    from birdsoundclassif_amd.nbm_datasets.prepare_dataset import encode_png_gray8
    data = tmp_path / 'dataset'
    synth.write_image_dataset(str(data), encode_png_gray8)
    monkeypatch.chdir(tmp_path)
    real_build = T.build_optimizer

    def build_with_filler(model, a):
        model.load_state_dict(filler_state_dict())
        from birdsoundclassif_amd.nets import _prep
        _prep.bump()
        return real_build(model, a)
    monkeypatch.setattr(T, 'build_optimizer', build_with_filler)

    def losses(device_inflate, name):
        args = T.default_args(device='cuda', data_path=str(data), save_dir=str(tmp_path / 'models'), model_name=name,
                              batch_size=1, num_workers=0, validation_prop=0.67, max_steps=1, neg_step_freq=2,
                              first_neg_step=0, seed=3)
        assert args.device_inflate is False
        args.val_freq, args.log_freq, args.host_noise, args.device_inflate = 1000, 1, False, device_inflate
        assert T.main(args) == 1
        rows = [json.loads(l) for l in open(tmp_path / 'models' / name / 'scalars.jsonl')]
        return {r['tag']: r['value'] for r in rows if r['tag'].startswith('Training_Loss/')}
    # the first driver run of a process draws another noise seed than the later ones do (on the host route alike: its
    # result is `first`), so the two runs that are compared both come after it
    first, on, off = losses(False, 'first'), losses(True, 'on'), losses(False, 'off')
    print('losses, first run (host inflate):', first, '\nlosses, device inflate:', on, '\nlosses, host inflate:', off)
    assert 'Training_Loss/first_class_loss' in off and all(np.isfinite(v) for v in off.values())
    assert on == off
    assert T.get_args_parser().parse_args(['--device_inflate']).device_inflate is True
