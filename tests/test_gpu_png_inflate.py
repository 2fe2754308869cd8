"""GPU: `nbm_png_inflate` (ops.png_inflate) against `zlib.decompress`, byte for byte.  Every image is 70 x 1024
(71 750 scanline bytes: past one 65 535-byte stored block and two 32 KiB windows).  The streams come from
tests/deflate_writer.py; tests/test_png_inflate_cpu.py proves them on the host."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import deflate_writer as DW                                                  # noqa: E402


def _inflate(streams, **kw):
    from birdsoundclassif_amd import ops
    packed, table = ops.png_payload_pack(list(streams))
    raw, status = ops.png_inflate(torch.from_numpy(packed).cuda(), table, DW.H, DW.W, **kw)
    assert raw.shape == (len(streams), DW.EXPECT) and raw.dtype == torch.uint8 and status.dtype == torch.int32
    return raw, status


def _expected(datas):
    return torch.from_numpy(np.stack([np.frombuffer(d, dtype=np.uint8) for d in datas]))


def _check(named):
    """named: name -> (stream, expected bytes, ...): one batch, every stream status 0 and equal to its bytes."""
    names = list(named)
    raw, status = _inflate([named[n][0] for n in names])
    status = status.cpu().tolist()
    assert status == [0] * len(names), {n: s for n, s in zip(names, status) if s}
    got, ref = raw.cpu(), _expected([named[n][1] for n in names])
    for i, n in enumerate(names):
        assert torch.equal(got[i], ref[i]), n


def test_zlib_made_streams_in_one_batch():
    _check(DW.zlib_streams())


def test_handwritten_streams():
    _check(DW.handwritten_streams())


def test_single_stream_and_mixed_lengths():
    z = DW.zlib_streams()
    _check({'gradient-level9': z['gradient-level9']})
    three = {n: z[n] for n in ('random-level0', 'zeros-level9', 'gradient-level6')}       # ~71.8 KB, ~0.1 KB, tens of KB
    sizes = [len(v[0]) for v in three.values()]
    assert sizes[1] < 200 < sizes[2] < sizes[0]
    _check(three)


def test_payload_that_ends_with_the_buffer():
    """No padding behind the last stream: its last byte is the allocation's last byte."""
    from birdsoundclassif_amd import ops
    z = DW.zlib_streams()
    names = ['zeros-level6', 'gradient-level1']
    packed, table = ops.png_payload_pack([z[n][0] for n in names])
    end = int(table[-1].sum())
    assert end % 16 != 0 and end < packed.size
    raw, status = ops.png_inflate(torch.from_numpy(packed[:end].copy()).cuda(), table, DW.H, DW.W)
    assert status.cpu().tolist() == [0, 0] and torch.equal(raw.cpu(), _expected([z[n][1] for n in names]))


def test_stale_buffers_and_two_runs_identical():
    z = DW.zlib_streams()
    names = ['gradient-level6', 'random-rle', 'zeros-fixed', 'gradient-huffman']
    pitch = (DW.EXPECT + 15) // 16 * 16
    outs = []
    for fill in (0xA5, 0x5A):
        out = torch.full((len(names), pitch), fill, dtype=torch.uint8, device='cuda')
        status = torch.full((len(names),), -0x5A5A5A5B, dtype=torch.int32, device='cuda')
        raw, st = _inflate([z[n][0] for n in names], out=out, status=status)
        assert st.data_ptr() == status.data_ptr() and raw.data_ptr() == out.data_ptr()
        assert status.cpu().tolist() == [0] * len(names)
        assert bool((out[:, DW.EXPECT:] == fill).all())              # nothing written behind a row's bytes
        outs.append(raw.cpu())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], _expected([z[n][1] for n in names]))


@pytest.mark.parametrize('name', sorted(DW.corrupt_streams()))
def test_corrupt_stream_beside_two_good_ones(name):
    stream, code, _ = DW.corrupt_streams()[name]
    z = DW.zlib_streams()
    good = ['gradient-level6', 'random-level1']
    raw, status = _inflate([z[good[0]][0], stream, z[good[1]][0]])
    assert status.cpu().tolist() == [0, code, 0]
    got = raw.cpu()
    assert torch.equal(got[0], _expected([z[good[0]][1]])[0]) and torch.equal(got[2], _expected([z[good[1]][1]])[0])


def test_bad_arguments_are_refused():
    from birdsoundclassif_amd import ops
    stream = DW.zlib_streams()['zeros-level6'][0]
    packed, table = ops.png_payload_pack([stream, stream])
    payload = torch.from_numpy(packed).cuda()
    outside = table.copy()
    outside[1, 1] = packed.size - outside[1, 0] + 1
    with pytest.raises(ValueError, match='outside the payload'):
        ops.png_inflate(payload, outside, DW.H, DW.W)
    unaligned = table.copy()
    unaligned[1, 0] += 4
    with pytest.raises(ValueError, match='16-byte boundary'):
        ops.png_inflate(payload, unaligned, DW.H, DW.W)
    with pytest.raises(ValueError):
        ops.png_inflate(payload, table[:0], DW.H, DW.W)
    with pytest.raises(ValueError):
        ops.png_inflate(payload, table.astype(np.int32), DW.H, DW.W)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.png_inflate(torch.from_numpy(packed), table, DW.H, DW.W)
