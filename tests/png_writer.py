"""A small PNG writer for the decoder tests, beside jpeg_writer.py: samples in, file bytes out, with the colour type, bit
depth, interlacing and the filter of every row chosen by the caller - what Pillow's writer does not offer.  Built on
zlib only.  expected_bgr() applies the conversion rules of cv::imdecode(IMREAD_COLOR) to the same samples: the tests'
expectation comes from the construction, not from a decoder."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
LEGAL = [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16), (6, 8), (6, 16)]
ADAM7 = [(0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)]  # x0, y0, dx, dy


def chunk(kind, data=b"", crc_ok=True):
    crc = zlib.crc32(kind + data) & 0xFFFFFFFF
    if not crc_ok:
        crc ^= 0x5A5A5A5A
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", crc)


def ihdr(width, height, bit_depth, color_type, interlace=0, compression=0, filter_method=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, bit_depth, color_type, compression, filter_method, interlace))


def passes(height, width, interlace):
    """[(x0, y0, dx, dy)] of the passes that hold pixels"""
    if not interlace:
        return [(0, 0, 1, 1)]
    return [p for p in ADAM7 if width > p[0] and height > p[1]]


def pack_rows(samples, bit_depth):
    """(rows, cols, channels) samples -> (rows, rowbytes) uint8, as PNG stores a scanline"""
    rows, cols, ch = samples.shape
    flat = samples.reshape(rows, cols * ch).astype(np.uint16)
    if bit_depth == 8:
        return flat.astype(np.uint8)
    if bit_depth == 16:
        return np.stack([flat >> 8, flat & 0xFF], -1).reshape(rows, -1).astype(np.uint8)
    per = 8 // bit_depth
    pad = (-flat.shape[1]) % per
    flat = np.pad(flat, ((0, 0), (0, pad)))
    out = np.zeros((rows, flat.shape[1] // per), np.uint16)
    for k in range(per):  # most significant bits first
        out |= flat[:, k::per] << ((per - 1 - k) * bit_depth)
    return out.astype(np.uint8)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_row(kind, row, prior, bpp):
    """the filtered bytes of one scanline (PNG specification, section 9); a kind above 4 stores the bytes unfiltered"""
    x = row.astype(np.int32)
    b = prior.astype(np.int32)
    a = np.concatenate([np.zeros(bpp, np.int32), x[:-bpp]]) if len(x) > bpp else np.zeros(len(x), np.int32)
    c = np.concatenate([np.zeros(bpp, np.int32), b[:-bpp]]) if len(x) > bpp else np.zeros(len(x), np.int32)
    pred = {1: a, 2: b, 3: (a + b) >> 1, 4: _paeth(a, b, c)}.get(kind, np.zeros(len(x), np.int32))
    return ((x - pred) & 0xFF).astype(np.uint8)


def scanlines(samples, color_type, bit_depth, interlace=0, filters=0):
    """the stream that IDAT compresses.  filters: one kind for every row, a list used cyclically over the rows of a pass,
    or a function (pass index, row) -> kind."""
    samples = np.asarray(samples)
    if samples.ndim == 2:
        samples = samples[:, :, None]
    height, width, ch = samples.shape
    assert ch == CHANNELS[color_type]
    bits = ch * bit_depth
    bpp = max(1, bits // 8)
    out = []
    for pi, (x0, y0, dx, dy) in enumerate(passes(height, width, interlace)):
        rows = pack_rows(samples[y0::dy, x0::dx], bit_depth)
        prior = np.zeros(rows.shape[1], np.uint8)
        for r in range(rows.shape[0]):
            kind = filters(pi, r) if callable(filters) else filters[r % len(filters)] if isinstance(filters, (list, tuple)) else filters
            out.append(bytes([kind]) + filter_row(kind, rows[r], prior, bpp).tobytes())
            prior = rows[r]
    return b"".join(out)


def write_png(samples, color_type, bit_depth, interlace=0, filters=0, palette=None, ancillary=(), before_idat=(), level=6, idat_pieces=1,
              stream=None, header=None, iend=True):
    """file bytes.  palette: (n, 3) RGB for PLTE (required by colour type 3).  ancillary / before_idat: ready-made chunks placed
    after IHDR / just before IDAT.  stream: replaces the scanline stream (tests of short and surplus data); header:
    replaces the IHDR chunk."""
    samples = np.asarray(samples)
    height, width = samples.shape[:2]
    raw = scanlines(samples, color_type, bit_depth, interlace, filters) if stream is None else stream
    z = zlib.compress(raw, level)
    cut = [len(z) * k // idat_pieces for k in range(idat_pieces + 1)]
    parts = [SIGNATURE, header if header is not None else ihdr(width, height, bit_depth, color_type, interlace)]
    parts += list(ancillary)
    if palette is not None:
        parts.append(chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes()))
    parts += list(before_idat)
    parts += [chunk(b"IDAT", z[cut[k]:cut[k + 1]]) for k in range(idat_pieces)]
    if iend:
        parts.append(chunk(b"IEND"))
    return b"".join(parts)


def expected_bgr(samples, color_type, bit_depth, palette=None):
    """what cv::imdecode(IMREAD_COLOR) makes of these samples: 1 / 2 / 4-bit grey by bit replication, palette indices through
    PLTE (black beyond it), 16-bit samples cut to their high byte, alpha dropped, grey to three channels, BGR order"""
    s = np.asarray(samples).astype(np.int64)
    if s.ndim == 2:
        s = s[:, :, None]
    if color_type == 3:
        table = np.zeros((256, 3), np.uint8)
        table[:len(palette)] = np.asarray(palette, np.uint8)
        return table[s[:, :, 0]][:, :, ::-1].copy()
    if bit_depth == 16:
        s = s >> 8
    elif bit_depth < 8:
        s = s * (255 // ((1 << bit_depth) - 1))
    if color_type in (0, 4):
        return np.repeat(s[:, :, :1], 3, axis=2).astype(np.uint8)
    return s[:, :, 2::-1].astype(np.uint8)


def random_samples(rs, height, width, color_type, bit_depth):
    return rs.randint(0, 1 << bit_depth, (height, width, CHANNELS[color_type])).astype(np.uint16)
