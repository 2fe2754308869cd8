"""CPU: the fixtures of the PNG inflate tests are what they claim to be (every good stream inflates to its intended
bytes under `zlib.decompress`, every corrupt one is refused on the host), plus the host-only pieces of the device
inflate route: `ops.png_payload_pack` and `image_dataset.read_png_payload`."""
import struct
import zlib

import numpy as np
import pytest

import deflate_writer as DW
from deflate_writer import write_png


def test_zlib_made_streams_round_trip():
    streams = DW.zlib_streams()
    assert len(streams) == 24
    for name, (stream, data) in streams.items():
        assert len(data) == DW.EXPECT and zlib.decompress(stream) == data, name
    # what the names promise: stored blocks inside the image, a small-window header, stored fall-back on noise
    assert len(streams['random-level0'][0]) > DW.EXPECT and streams['gradient-wbits9'][0][0] >> 4 == 1
    assert len(streams['random-level6'][0]) > DW.EXPECT and len(streams['zeros-level9'][0]) < 200


def test_handwritten_streams_round_trip():
    streams = DW.handwritten_streams()
    for name, (stream, data, end_bits) in streams.items():
        assert len(data) == DW.EXPECT, name
        assert zlib.decompress(stream) == data, name
    assert streams['ends_on_byte'][2] % 8 == 0 and streams['ends_mid_byte'][2] % 8 != 0
    d = streams['dist32768_len258'][1]
    assert d[32768:32768 + 258] == d[:258]
    d = streams['dist1_len258'][1]
    assert d[:259] == bytes([7]) * 259
    d = streams['match_over_ring_wrap'][1]
    assert d[32668:32668 + 258] == d[32368:32368 + 258] and d[65436:65436 + 258] == d[32668:32668 + 258]


def test_writer_blocks_and_bfinal():
    w = DW.DeflateWriter().fixed([65, 66, (4, 2)]).stored(b'xyz').fixed([67])
    stream = w.finish()
    assert zlib.decompress(stream) == b'ABABABxyzC' == bytes(w.expected)
    d = zlib.decompressobj()
    assert d.decompress(stream) == b'ABABABxyzC' and d.eof and d.unused_data == b''
    assert stream[2] & 1 == 0                                       # first block: BFINAL clear


def test_corrupt_streams_are_refused_on_the_host(tmp_path):
    for name, (stream, code, host_raises) in DW.corrupt_streams().items():
        assert 1 <= code <= 10, name
        if host_raises:
            with pytest.raises(zlib.error):
                zlib.decompress(stream)
        else:                                                       # inflates cleanly to another size: refused by the size
            assert len(zlib.decompress(stream)) != DW.EXPECT, name
    assert {c for _, c, _ in DW.corrupt_streams().values()} >= {1, 2, 3, 5, 7, 8, 9, 10}


def test_png_payload_pack():
    from birdsoundclassif_amd import ops
    streams = [b'a' * 5, b'b' * 16, b'c' * 33, b'd']
    packed, table = ops.png_payload_pack(streams)
    assert packed.dtype == np.uint8 and packed.ndim == 1 and table.dtype == np.int64 and table.shape == (4, 2)
    assert table.tolist() == [[0, 5], [16, 16], [32, 33], [80, 1]]
    assert packed.size % 16 == 0 and packed.size >= 81 + 8
    for (o, n), s in zip(table, streams):
        assert o % 16 == 0 and packed[o:o + n].tobytes() == s
    keep = np.ones(packed.size, bool)
    for o, n in table:
        keep[o:o + n] = False
    assert not packed[keep].any()                                   # padding is zeros
    # a stream that ends on a 16-byte boundary still has 8 bytes behind it
    packed, table = ops.png_payload_pack([b'e' * 32])
    assert table.tolist() == [[0, 32]] and packed.size >= 40 and packed.size % 16 == 0
    packed, table = ops.png_payload_pack([])
    assert table.shape == (0, 2) and table.dtype == np.int64 and packed.dtype == np.uint8 and packed.size % 16 == 0


def test_read_png_payload_matches_read_png_scanlines(tmp_path):
    from birdsoundclassif_amd.nbm_datasets.image_dataset import read_png_payload, read_png_scanlines
    img = np.random.RandomState(0).randint(0, 256, size=(37, 129), dtype=np.uint8)
    for name, kw in (('one.png', {}), ('multi.png', dict(idat_split=100)), ('stored.png', dict(level=0, idat_split=1000))):
        raw, stream = write_png(tmp_path / name, img, **kw)
        payload, h, w = read_png_payload(str(tmp_path / name))
        lines = read_png_scanlines(str(tmp_path / name))
        assert isinstance(payload, bytes) and payload == stream and (h, w) == (37, 129)
        assert lines.shape == (h, w + 1) and zlib.decompress(payload) == lines.tobytes() == raw


def test_read_png_payload_keeps_the_refusals(tmp_path):
    from birdsoundclassif_amd.nbm_datasets.image_dataset import read_png_payload, read_png_scanlines
    img = np.zeros((4, 6), np.uint8)
    write_png(tmp_path / 'nosig.png', img, signature=b'\x89PNX\r\n\x1a\n')
    write_png(tmp_path / 'sixteen.png', img, ihdr_tail=(16, 0, 0, 0, 0))
    write_png(tmp_path / 'colour.png', img, ihdr_tail=(8, 2, 0, 0, 0))
    write_png(tmp_path / 'interlaced.png', img, ihdr_tail=(8, 0, 0, 0, 1))
    for read in (read_png_payload, read_png_scanlines):
        with pytest.raises(ValueError, match='not a PNG file'):
            read(str(tmp_path / 'nosig.png'))
        for name in ('sixteen.png', 'colour.png', 'interlaced.png'):
            with pytest.raises(NotImplementedError, match='only 8-bit greyscale non-interlaced PNG is supported'):
                read(str(tmp_path / name))


def test_wrong_size_streams_are_refused_by_the_host_route(tmp_path):
    """The two corrupt streams that zlib inflates cleanly: `read_png_scanlines` refuses them by their size."""
    from birdsoundclassif_amd.nbm_datasets.image_dataset import read_png_scanlines
    chunk = DW.png_chunk
    for name in ('output_longer', 'output_shorter'):
        stream = DW.corrupt_streams()[name][0]
        p = tmp_path / (name + '.png')
        p.write_bytes(b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', DW.W, DW.H, 8, 0, 0, 0, 0)) +
                      chunk(b'IDAT', stream) + chunk(b'IEND', b''))
        with pytest.raises(ValueError, match='inflated size'):
            read_png_scanlines(str(p))
