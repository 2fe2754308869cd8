"""Test helper: RIFF/WAVE files in every sample format `read_wav` reads (and a few it refuses), built byte by byte."""
import struct

import numpy as np

FORMATS = [(1, 8), (1, 16), (1, 24), (1, 32), (3, 32), (3, 64)]


def encode(x, tag, bits):
    """int16 samples [n, channels] -> interleaved payload bytes in the format (tag, bits); the low bits of the wider
    integer formats are filled with a pattern, so that every byte of a sample matters."""
    x = np.asarray(x, dtype=np.int16)
    v = x.astype(np.int64)
    if (tag, bits) == (1, 8):
        return ((v >> 8) + 128).astype(np.uint8).tobytes()
    if (tag, bits) == (1, 16):
        return x.astype('<i2').tobytes()
    if (tag, bits) == (1, 24):
        w = (v << 8) | ((v * 37) & 0xFF)
        return pack24(w)
    if (tag, bits) == (1, 32):
        return ((v << 16) | ((v * 40503) & 0xFFFF)).astype('<i4').tobytes()
    if (tag, bits) == (3, 32):
        return (x.astype(np.float32) / np.float32(32768)).astype('<f4').tobytes()
    if (tag, bits) == (3, 64):
        return (x.astype(np.float64) / 32768.0 + 1e-9).astype('<f8').tobytes()
    raise ValueError((tag, bits))


def pack24(w):
    """int array of values in [-2^23, 2^23) -> little-endian 3-byte samples."""
    u = (np.asarray(w, dtype=np.int64) & 0xFFFFFF).astype('<u4')
    return u.view(np.uint8).reshape(-1, 4)[:, :3].tobytes()


def riff(payload, sr, tag, bits, channels, extensible=False, list_chunk=None, drop_tail=0, declared=None):
    """A wav file as bytes.  `extensible`: a 40-byte WAVE_FORMAT_EXTENSIBLE fmt chunk whose sub-format starts with `tag`;
    `list_chunk`: bytes of a LIST chunk put in front of `data` (odd lengths get their pad byte); `drop_tail`: that many bytes
    of the payload are missing from the file although the header declares them; `declared`: data chunk size to declare."""
    fb = channels * (bits // 8)
    if extensible:
        guid = struct.pack('<H', tag) + bytes.fromhex('000000001000800000aa00389b71')
        fmt = struct.pack('<HHIIHHHHI', 0xFFFE, channels, sr, sr * fb, fb, bits, 22, bits, 0) + guid
    else:
        fmt = struct.pack('<HHIIHH', tag, channels, sr, sr * fb, fb, bits)
    body = b'WAVE' + b'fmt ' + struct.pack('<I', len(fmt)) + fmt
    if list_chunk is not None:
        body += b'LIST' + struct.pack('<I', len(list_chunk)) + list_chunk + (b'\0' if len(list_chunk) & 1 else b'')
    size = len(payload) if declared is None else declared
    body += b'data' + struct.pack('<I', size) + payload[:len(payload) - drop_tail]
    return b'RIFF' + struct.pack('<I', len(body) + drop_tail) + body


def write(path, x, sr, tag, bits, **kw):
    """int16 samples [n] or [n, channels] -> a wav file in the format (tag, bits)."""
    x = np.asarray(x)
    if x.ndim == 1:
        x = x[:, None]
    with open(path, 'wb') as f:
        f.write(riff(encode(x, tag, bits), sr, tag, bits, x.shape[1], **kw))


def channels_of(x, channels):
    """Mono int16 clip -> [n, channels]: channel c is the clip delayed by 7 c samples at a lower level, so that the down-mix
    differs from every single channel."""
    x = np.asarray(x, dtype=np.int16)
    return np.stack([np.roll(x, 7 * c) // (c + 1) for c in range(channels)], 1).astype(np.int16)
