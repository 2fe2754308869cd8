"""Test-side writer of zlib streams (RFC 1950 / 1951) with caller-chosen content, and the streams the PNG inflate tests
share.  zlib's own compressor never emits a distance above 32 506 and never puts a match straight behind a stored
block; `DeflateWriter` writes stored blocks and fixed-Huffman blocks of any literals and (length, distance) pairs, sets
BFINAL on the last block only, and keeps the bytes the stream must inflate to (`expected`).  `raw_bits` and the
`header` / `adler` overrides are for streams that are wrong on purpose.

tests/test_png_inflate_cpu.py proves every stream below against `zlib.decompress` before a GPU sees it."""
import functools
import struct
import zlib

import numpy as np

H, W = 70, 1024
EXPECT = H * (W + 1)           # 71 750: just past one 65 535-byte stored block and two 32 KiB windows

_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
          8193, 12289, 16385, 24577]
_DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


class DeflateWriter:
    def __init__(self, header=(0x78, 0x01)):
        self.head = bytes(header)
        self.blocks = []            # ('stored', bytes) | ('fixed', items) | ('raw', [(value, nbits)])
        self.expected = bytearray()

    # ---- content
    def stored(self, data):
        assert len(data) <= 65535
        self.blocks.append(('stored', bytes(data)))
        self.expected += data
        return self

    def fixed(self, items):
        """items: ints (literals) and (length, distance) pairs."""
        for it in items:
            if isinstance(it, tuple):
                n, d = it
                assert 3 <= n <= 258 and 1 <= d <= 32768 and d <= len(self.expected)
                for _ in range(n):
                    self.expected.append(self.expected[-d])
            else:
                self.expected.append(it)
        self.blocks.append(('fixed', list(items)))
        return self

    def fixed_unchecked(self, items):
        """A fixed block whose matches are not simulated (for distances that reach too far back)."""
        self.blocks.append(('fixed', list(items)))
        return self

    def raw_bits(self, fields):
        """A 'block' of literal bit fields [(value, nbits)], least significant bit first, BFINAL included."""
        self.blocks.append(('raw', list(fields)))
        return self

    def filler(self, n, seed=1):
        """n pseudo-random bytes as stored blocks."""
        data = np.random.RandomState(seed).randint(0, 256, size=n, dtype=np.uint8).tobytes()
        for o in range(0, n, 65535):
            self.stored(data[o:o + 65535])
        return self

    def fill_to(self, total=EXPECT, seed=1):
        return self.filler(total - len(self.expected), seed)

    # ---- encoding
    def finish(self, adler=None, with_bit_length=False):
        acc, nacc, out = 0, 0, bytearray(self.head)

        def put(value, n):                       # n bits, least significant first
            nonlocal acc, nacc
            acc |= value << nacc
            nacc += n
            while nacc >= 8:
                out.append(acc & 0xFF)
                acc >>= 8
                nacc -= 8

        def code(value, n):                      # a Huffman code: most significant bit first
            put(int(format(value, f'0{n}b')[::-1], 2), n)

        def lit(sym):
            if sym < 144:
                code(0x30 + sym, 8)
            elif sym < 256:
                code(0x190 + sym - 144, 9)
            elif sym < 280:
                code(sym - 256, 7)
            else:
                code(0xC0 + sym - 280, 8)

        end_bits = None
        for i, (kind, body) in enumerate(self.blocks):
            last = int(i == len(self.blocks) - 1)
            if kind == 'raw':
                for value, n in body:
                    put(value, n)
            elif kind == 'stored':
                put(last, 1), put(0, 2)
                if nacc:
                    put(0, 8 - nacc)
                put(len(body), 16), put(len(body) ^ 0xFFFF, 16)
                out += body
            else:
                put(last, 1), put(1, 2)
                for it in body:
                    if isinstance(it, tuple):
                        n, d = it
                        li = max(k for k in range(29) if _LBASE[k] <= n) if n < 258 else 28
                        lit(257 + li), put(n - _LBASE[li], _LEXT[li])
                        di = max(k for k in range(30) if _DBASE[k] <= d)
                        code(di, 5), put(d - _DBASE[di], _DEXT[di])
                    else:
                        lit(it)
                lit(256)
            end_bits = 8 * len(out) + nacc
        if nacc:
            put(0, 8 - nacc)
        a = zlib.adler32(bytes(self.expected)) if adler is None else adler
        out += a.to_bytes(4, 'big')
        return (bytes(out), end_bits) if with_bit_length else bytes(out)


def png_chunk(kind, body):
    return struct.pack('>I', len(body)) + kind + body + struct.pack('>I', zlib.crc32(kind + body))


def write_png(path, img, level=6, idat_split=None, ihdr_tail=(8, 0, 0, 0, 0), signature=b'\x89PNG\r\n\x1a\n'):
    """uint8 [H, W] -> an 8-bit greyscale PNG file (filter 0); idat_split: payload bytes per IDAT chunk.  Returns
    (scanline bytes, zlib stream)."""
    h, w = img.shape
    raw = b''.join(b'\x00' + img[r].tobytes() for r in range(h))
    payload = zlib.compress(raw, level)
    parts = [payload] if idat_split is None else [payload[o:o + idat_split] for o in range(0, len(payload), idat_split)]
    with open(path, 'wb') as f:
        f.write(signature + png_chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, *ihdr_tail)) +
                b''.join(png_chunk(b'IDAT', p) for p in parts) + png_chunk(b'IEND', b''))
    return raw, payload


# --------------------------------------------------------------------------- the shared streams
def _contents():
    rs = np.random.RandomState(7)
    ramp = np.add.outer(np.arange(H) * 2.0, np.arange(W + 1) * 0.2)
    gradient = np.clip(ramp + rs.normal(0, 6, size=(H, W + 1)), 0, 255).astype(np.uint8)
    gradient[:, 0] = 0                                           # a filter byte per scanline, like a PNG's
    return {'gradient': gradient.tobytes(), 'zeros': bytes(EXPECT),
            'random': rs.randint(0, 256, size=EXPECT, dtype=np.uint8).tobytes()}


def _deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, mem=8):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, mem, strategy)
    return c.compress(data) + c.flush()


@functools.lru_cache(None)
def zlib_streams():
    """name -> (stream, expected bytes): what zlib itself writes, every block type and strategy."""
    out = {}
    for cname, data in _contents().items():
        for tag, kw in (('level0', dict(level=0)), ('level1', dict(level=1)), ('level6', dict(level=6)),
                        ('level9', dict(level=9)), ('fixed', dict(strategy=zlib.Z_FIXED)), ('rle', dict(strategy=zlib.Z_RLE)),
                        ('huffman', dict(strategy=zlib.Z_HUFFMAN_ONLY)), ('wbits9', dict(wbits=9, mem=1))):
            out[f'{cname}-{tag}'] = (_deflate(data, **kw), data)
    return out


def _rand(n, seed):
    return np.random.RandomState(seed).randint(0, 256, size=n, dtype=np.uint8).tobytes()


@functools.lru_cache(None)
def handwritten_streams():
    """name -> (stream, expected bytes, bit position at which the last block ends): the edges zlib never writes.
    Every stream inflates to EXPECT bytes."""
    w = {}
    w['dist32768_len258'] = DeflateWriter().stored(_rand(32768, 2)).fixed([(258, 32768)]).fill_to()
    w['dist1_len258'] = DeflateWriter().fixed([7, (258, 1)]).fill_to()
    around = [(n, d) for d in (63, 64, 65) for n in (3, 64, 65, 258)]
    w['wave_width'] = DeflateWriter().fixed(list(_rand(100, 3)) + around).fill_to()
    w['match_at_position_1'] = DeflateWriter().fixed([0x55, (10, 1)]).fill_to()
    w['match_after_stored'] = DeflateWriter().stored(_rand(500, 4)).fixed([(50, 500)]).fill_to()
    w['match_over_ring_wrap'] = (DeflateWriter().stored(_rand(32668, 5)).fixed([(258, 300)]).filler(32510, 6)
                                 .fixed([(258, 32768), (200, 1)]).fill_to())
    w['ends_on_byte'] = DeflateWriter().filler(EXPECT - 8).fixed([200, 201, 202, 203, 204, 205, 1, 2])
    w['ends_mid_byte'] = DeflateWriter().filler(EXPECT - 1).fixed([9])
    w['empty_block_between'] = DeflateWriter().fixed([1, 2, 3]).fixed([]).fixed([4, 5, (5, 5)]).fill_to()
    w['empty_stored_between'] = DeflateWriter().fixed([1, 2, 3]).stored(b'').fixed([(3, 3)]).fill_to()
    out = {}
    for name, dw in w.items():
        stream, end_bits = dw.finish(with_bit_length=True)
        out[name] = (stream, bytes(dw.expected), end_bits)
    stream, data = zlib_streams()['gradient-level6']
    out['bytes_behind_the_trailer'] = (stream + b'\x01\x02\x03', data, None)      # zlib.decompress ignores them
    return out


# NBM_INFLATE_* of include/nbm_hip.h
EHEADER, EBLOCKTYPE, ESTORED, ECODELENGTHS, ECODESET, ECODE, EDISTANCE, EOUTPUT, EINPUT, EADLER = range(1, 11)


@functools.lru_cache(None)
def corrupt_streams():
    """name -> (stream, documented status, host_raises).  host_raises: `zlib.decompress` raises on it; the two streams
    of the wrong size inflate cleanly and are refused by their size (`read_png_scanlines` does the same)."""
    good, data = zlib_streams()['gradient-level6']
    out = {}
    out['truncated'] = (good[:len(good) // 2], EINPUT, True)
    out['wrong_adler'] = (good[:-1] + bytes([good[-1] ^ 0x5A]), EADLER, True)
    fdict = 0x78 * 256 + 0x20
    out['fdict'] = (bytes([0x78, 0x20 + (31 - fdict % 31) % 31]) + good[2:], EHEADER, True)
    cm7 = 0x77 * 256
    out['cm_not_8'] = (bytes([0x77, (31 - cm7 % 31) % 31]) + good[2:], EHEADER, True)
    out['block_type_3'] = (DeflateWriter().raw_bits([(1, 1), (3, 2)]).finish(adler=1), EBLOCKTYPE, True)
    out['stored_len_nlen'] = (DeflateWriter().raw_bits([(1, 1), (0, 2), (0, 5), (100, 16), (100, 16)]).finish(adler=1)
                              + bytes(200), ESTORED, True)
    out['distance_before_start'] = (DeflateWriter().fixed_unchecked([1, 2, (3, 5)]).fill_to(EXPECT - 5).finish(), EDISTANCE,
                                    True)
    # dynamic block whose code-length code gives all 19 symbols one bit
    out['oversubscribed_code_lengths'] = (DeflateWriter().raw_bits([(1, 1), (2, 2), (0, 5), (0, 5), (15, 4)] + [(1, 3)] * 19)
                                          .finish(adler=1) + bytes(64), ECODESET, True)
    # dynamic block: code-length code {1: '0', 2: '1'}, then 257 literal/length codes and 1 distance code of one bit each
    cl = [(0, 3)] * 18
    cl[15] = cl[17] = (1, 3)
    out['oversubscribed_literals'] = (DeflateWriter().raw_bits([(1, 1), (2, 2), (0, 5), (0, 5), (14, 4)] + cl + [(0, 1)] * 258)
                                      .finish(adler=1) + bytes(64), ECODESET, True)
    out['output_longer'] = (_deflate(data + bytes(10)), EOUTPUT, False)
    out['output_shorter'] = (_deflate(data[:-10]), EOUTPUT, False)
    return out
