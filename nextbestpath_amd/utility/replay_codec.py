"""The compact replay record ("NBPC", version 1): the DEFINITION of the format, in plain numpy.  Lossless: any fp32 input comes back
bit for bit.  The device kernels (csrc/nbp_replay.hip: hipops.replay_encode / replay_decode) produce and consume exactly these bytes.

One stream holds the C = 6 planes of a replay record -- the five input maps of 'current_model_input' [1,5,S,S], then the obstacle
label 'current_gt_2d_layout' [1,1,S,S] -- little-endian, every section on a 16-byte boundary, padding bytes zero:

    header, 16 + 8 C = 64 bytes
        magic "NBPC" | u16 version = 1 | u16 C | u32 S | u32 total_bytes (header included)
        per channel { u32 nnz, u8 width, 3 zero bytes }
    per channel, in order
        bitmap, S^2 / 8 bytes: bit i of byte j is row-major pixel 8 j + i, set where the pixel's fp32 BIT PATTERN is not 0x00000000
            (-0.0, denormals and NaN count as non-zero)
        the non-zero pixels in row-major order, `width` bytes each, padded to 16

`width` is the smallest that holds every non-zero pixel of the channel:

    0   every non-zero is exactly 1.0f (also nnz == 0)     no value section
    1   every non-zero is an integer in [1, 255]           u8
    2   every non-zero is an integer in [1, 65535]         u16
    4   anything else                                      the raw fp32 bit patterns

Width 4 always applies: there is no lossy path and no fallback.  S % 16 == 0, as NBP.forward requires, so a bitmap is a multiple of
32 bytes.  The worst case is stream_bound(S) = 64 + 6 (S^2 / 8 + 4 S^2) bytes.
"""
from __future__ import annotations

import struct

import numpy as np

MAGIC = b"NBPC"
VERSION = 1
CHANNELS = 6
HEADER_BYTES = 16 + 8 * CHANNELS
WIDTHS = (0, 1, 2, 4)
_ONE = 0x3F800000


def _pad16(n):
    return (int(n) + 15) & ~15


def stream_bound(S):
    """Largest stream of a record of side S (every pixel non-zero at width 4)."""
    S = int(S)
    return HEADER_BYTES + CHANNELS * (S * S // 8 + 4 * S * S)


def _check_side(S):
    if S < 16 or S % 16:
        raise ValueError(f"S: {S} is not a positive multiple of 16")


def select_width(values):
    """Width of a channel from its non-zero pixels (fp32, any shape)."""
    v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
    if np.all(v.view(np.uint32) == _ONE):
        return 0
    with np.errstate(invalid="ignore"):
        whole = (v >= 1.0) & (v <= 65535.0) & (np.floor(v) == v)
    if not whole.all():
        return 4
    return 1 if v.max() <= 255.0 else 2


def encode(model_input, gt) -> bytes:
    """model_input [1,5,S,S] (or [5,S,S]) and gt [1,1,S,S] (or [1,S,S] / [S,S]) fp32 -> the stream."""
    x = np.ascontiguousarray(model_input, dtype=np.float32)
    g = np.ascontiguousarray(gt, dtype=np.float32)
    S = x.shape[-1]
    _check_side(S)
    if x.size != 5 * S * S or x.shape[-2] != S or g.size != S * S:
        raise ValueError(f"encode: model_input [1,5,S,S] and gt [1,1,S,S] expected, got {x.shape} and {g.shape}")
    planes = np.concatenate([x.reshape(5, S * S), g.reshape(1, S * S)]).view(np.uint32)
    entries, sections = [], []
    for c in range(CHANNELS):
        nz = planes[c] != 0
        vals = planes[c][nz]
        width = select_width(vals.view(np.float32))
        entries.append(struct.pack("<IB3x", len(vals), width))
        sections.append(np.packbits(nz, bitorder="little").tobytes())
        if width:
            body = (vals if width == 4 else vals.view(np.float32).astype({1: np.uint8, 2: np.uint16}[width])).astype(
                {1: "<u1", 2: "<u2", 4: "<u4"}[width]).tobytes()
            sections.append(body + bytes(_pad16(len(body)) - len(body)))
    payload = b"".join(sections)
    total = HEADER_BYTES + len(payload)
    return struct.pack("<4sHHII", MAGIC, VERSION, CHANNELS, S, total) + b"".join(entries) + payload


def parse_header(stream, length=None):
    """Validates the header of `stream` (bytes-like, at least the 64 header bytes) without touching the payload.
    length: what total_bytes must equal (default len(stream); None with a longer buffer: pass the slot's size check yourself).
    -> (S, total_bytes, [(nnz, width)] * 6, [(bitmap offset, value offset)] * 6); ValueError names the failing field."""
    buf = memoryview(stream).cast("B") if not isinstance(stream, (bytes, bytearray)) else stream
    if len(buf) < HEADER_BYTES:
        raise ValueError(f"total_bytes: a stream of {len(buf)} bytes is shorter than the {HEADER_BYTES}-byte header")
    magic, version, C, S, total = struct.unpack_from("<4sHHII", buf, 0)
    if magic != MAGIC:
        raise ValueError(f"magic: {bytes(magic)!r} is not {MAGIC!r}")
    if version != VERSION:
        raise ValueError(f"version: {version} (this codec reads version {VERSION})")
    if C != CHANNELS:
        raise ValueError(f"C: {C} channels (a replay record has {CHANNELS})")
    _check_side(S)
    SS = S * S
    chans, offs, pos = [], [], HEADER_BYTES
    for c in range(CHANNELS):
        nnz, width, z0, z1, z2 = struct.unpack_from("<IBBBB", buf, 16 + 8 * c)
        if width not in WIDTHS:
            raise ValueError(f"width: channel {c} has width {width}, not one of {WIDTHS}")
        if nnz > SS:
            raise ValueError(f"nnz: channel {c} claims {nnz} non-zero pixels of {SS}")
        if z0 or z1 or z2:
            raise ValueError(f"padding: channel {c}'s header entry has non-zero padding bytes")
        chans.append((nnz, width))
        offs.append((pos, pos + SS // 8))
        pos += SS // 8 + _pad16(nnz * width)
    if total != pos:
        raise ValueError(f"total_bytes: the header says {total}, its channel table implies {pos}")
    want = len(buf) if length is None else int(length)
    if total != want:
        raise ValueError(f"total_bytes: the header says {total}, the stream has {want} bytes")
    return S, total, chans, offs


def used_bytes(slot) -> int:
    """total_bytes of the stream at the start of a larger buffer (an encoder's arena slot), header validated."""
    buf = memoryview(slot).cast("B")
    if len(buf) < HEADER_BYTES:
        raise ValueError(f"total_bytes: a slot of {len(buf)} bytes is shorter than the {HEADER_BYTES}-byte header")
    total = struct.unpack_from("<I", buf, 12)[0]
    if total > len(buf):
        raise ValueError(f"total_bytes: the header says {total}, the slot has {len(buf)} bytes")
    parse_header(buf[:HEADER_BYTES], length=total)
    return total


def decode(stream):
    """The stream -> (model_input [1,5,S,S], gt [1,1,S,S]) fp32, new arrays.  Validates everything before it expands anything."""
    S, total, chans, offs = parse_header(stream)
    raw = np.frombuffer(stream, dtype=np.uint8)
    SS = S * S
    maps = []
    for c, ((nnz, width), (boff, voff)) in enumerate(zip(chans, offs)):
        bitmap = raw[boff:boff + SS // 8]
        if int(np.bitwise_count(bitmap).sum()) != nnz:
            raise ValueError(f"nnz: channel {c} claims {nnz}, its bitmap has {int(np.bitwise_count(bitmap).sum())} bits set")
        maps.append(np.unpackbits(bitmap, bitorder="little").astype(bool))
    out = np.zeros((CHANNELS, SS), dtype=np.uint32)
    for c, ((nnz, width), (boff, voff)) in enumerate(zip(chans, offs)):
        if width == 0:
            out[c][maps[c]] = _ONE
        elif width == 4:
            out[c][maps[c]] = raw[voff:voff + 4 * nnz].view("<u4")
        else:
            out[c][maps[c]] = raw[voff:voff + width * nnz].view({1: "<u1", 2: "<u2"}[width]).astype(np.float32).view(np.uint32)
    planes = out.view(np.float32).reshape(CHANNELS, S, S)
    return planes[:5].reshape(1, 5, S, S).copy(), planes[5:].reshape(1, 1, S, S).copy()
