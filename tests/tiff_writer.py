"""TIFF files built tag by tag and sample by sample (the tests' writer: Python's zlib and an LZW and a PackBits encoder of its
own; strips and tiles, both byte orders, predictor, planar, extra-sample and fill-order variants), and the numpy statement
of the pixel rules of host/tiff_decode.h - convert() - which plays the part raw_writer.convert_rows plays for BMP and PNM.

samples: (height, width, samples per pixel) integers below 2 ** bits, as the file stores them (before the predictor)."""
import struct
import zlib

import numpy as np

NONE, LZW, DEFLATE, ADOBE_DEFLATE, PACKBITS = 1, 5, 32946, 8, 32773
COMPRESSIONS = [NONE, PACKBITS, LZW, ADOBE_DEFLATE, DEFLATE]
MINISWHITE, MINISBLACK, RGB, PALETTE, CMYK = 0, 1, 2, 3, 5
BYTE, ASCII, SHORT, LONG, RATIONAL = 1, 2, 3, 4, 5
_REVERSED = np.array([int("{:08b}".format(i)[::-1], 2) for i in range(256)], np.uint8)


def lzw_encode(data):
    """TIFF LZW: codes most significant bit first, 9 bits to begin with, one more once 511 / 1023 / 2047 entries exist (the
    early change), a clear code first and when the table has 4094 entries, the end code last"""
    out, acc, have = bytearray(), 0, 0
    bits = 9

    def put(code):
        nonlocal acc, have
        acc = (acc << bits) | code
        have += bits
        while have >= 8:
            out.append((acc >> (have - 8)) & 0xFF)
            have -= 8
        acc &= (1 << have) - 1

    put(256)
    table, nxt = {}, 258
    if len(data):
        ent = data[0]
        for c in data[1:]:
            key = (ent << 8) | c
            if key in table:
                ent = table[key]
                continue
            put(ent)
            table[key] = nxt
            nxt += 1
            ent = c
            if nxt == 4094:
                put(256)
                table, nxt, bits = {}, 258, 9
            elif nxt == (1 << bits):
                bits += 1
        put(ent)
        nxt += 1
        if nxt == (1 << bits) and bits < 12:
            bits += 1
    put(257)
    if have:
        out.append((acc << (8 - have)) & 0xFF)
    return bytes(out)


def packbits_encode(data, row_bytes):
    """PackBits, row by row as the specification asks: runs of 3 or more as repeats, the rest as literals of at most 128"""
    out = bytearray()
    for r0 in range(0, len(data), row_bytes):
        row = data[r0:r0 + row_bytes]
        i, n = 0, len(row)
        while i < n:
            j = i
            while j + 1 < n and row[j + 1] == row[i] and j + 1 - i < 127:
                j += 1
            if j - i >= 2:
                out += bytes([257 - (j - i + 1), row[i]])
                i = j + 1
                continue
            j = i
            while j < n and j - i < 128 and not (j + 2 < n and row[j] == row[j + 1] == row[j + 2]):
                j += 1
            out += bytes([j - i - 1]) + bytes(row[i:j])
            i = j
    return bytes(out)


def pack_rows(values, bits, big_endian):
    """(rows, samples of a row) -> (rows, bytes of a row): most significant bits first below 8 bits, rows padded to a byte"""
    values = np.asarray(values)
    rows, n = values.shape
    if bits == 8:
        return values.astype(np.uint8)
    if bits == 16:
        return values.astype(">u2" if big_endian else "<u2").view(np.uint8).reshape(rows, 2 * n)
    per = 8 // bits
    padded = np.zeros((rows, (n + per - 1) // per * per), np.int64)
    padded[:, :n] = values
    out = np.zeros((rows, padded.shape[1] // per), np.int64)
    for k in range(per):
        out |= padded[:, k::per] << ((per - 1 - k) * bits)
    return out.astype(np.uint8)


def difference(block, bits, stride):
    """the horizontal-differencing predictor over (rows, samples of a row): each sample minus the one `stride` before it"""
    block = np.asarray(block, np.int64)
    out = block.copy()
    out[:, stride:] = (block[:, stride:] - block[:, :-stride]) & ((1 << bits) - 1)
    return out


def chunk_list(samples, bits, planar=1, predictor=1, tile=None, rows_per_strip=None, big_endian=False, rs=None):
    """The chunks in file order: [(nominal bytes (rows, row bytes), rows the image has in it)].  tile: (width, height) or None
    for strips of rows_per_strip rows (None: one strip).  The part of an edge tile beyond the image holds rs's noise (zeros
    without rs): nothing of it may show."""
    samples = np.asarray(samples, np.int64)
    h, w, spp = samples.shape
    if tile:
        tw, th = tile
    else:
        tw, th = w, min(h, rows_per_strip or h)
    out = []
    for plane in (range(spp) if planar == 2 else [None]):
        src = samples if plane is None else samples[:, :, plane:plane + 1]
        per = src.shape[2]
        for y0 in range(0, h, th):
            for x0 in range(0, w, tw):
                part = src[y0:y0 + th, x0:x0 + tw]
                rows = part.shape[0]
                block = rs.randint(0, 1 << bits, (th if tile else rows, tw, per)) if rs is not None else np.zeros((th if tile else rows, tw, per), np.int64)
                block[:rows, :part.shape[1]] = part
                flat = block.reshape(block.shape[0], tw * per)
                if predictor == 2:
                    flat = difference(flat, bits, per)
                out.append((pack_rows(flat, bits, big_endian), rows))
    return out, (tw, th)


def frame_data(samples, bits, **kw):
    """what tiff::Frame::data / ocr_tiff_frame.data hold: every chunk at its nominal size (a last strip zero-filled), and (tile
    width, tile height)"""
    chunks, (tw, th) = chunk_list(samples, bits, **kw)
    parts = []
    for block, _ in chunks:
        full = np.zeros((th, block.shape[1]), np.uint8)
        full[:block.shape[0]] = block
        parts.append(full.tobytes())
    return b"".join(parts), (tw, th)


def compress(raw, compression, row_bytes):
    if compression == NONE:
        return raw
    if compression == LZW:
        return lzw_encode(raw)
    if compression == PACKBITS:
        return packbits_encode(raw, row_bytes)
    return zlib.compress(raw, 6)


def write_tiff(samples, bits, photometric, big_endian=False, compression=NONE, predictor=1, planar=1, tile=None, rows_per_strip=None,
               extra=None, fill_order=1, colormap=None, predictor_tag=None, more_tags=(), drop=(), rs=None, orientation=None, streams=None):
    """samples -> file bytes.  extra: the ExtraSamples values (one per sample beyond the colour); colormap: (3, 2 ** bits) 16-bit
    values; predictor_tag: the tag's value when it is not to be the predictor applied; more_tags: [(id, type, [values])];
    drop: tag ids to leave out; streams: coded chunks to store instead of the encoder's (the refusal corpus)."""
    samples = np.asarray(samples, np.int64)
    h, w, spp = samples.shape
    e = ">" if big_endian else "<"
    chunks, (tw, th) = chunk_list(samples, bits, planar, predictor, tile, rows_per_strip, big_endian, rs)
    coded = []
    for block, rows in chunks:
        raw = block[:block.shape[0] if tile else rows].tobytes()
        c = compress(raw, compression, block.shape[1])
        coded.append(_REVERSED[np.frombuffer(c, np.uint8)].tobytes() if fill_order == 2 else c)
    if streams is not None:
        coded = list(streams)
    tags = [(256, LONG, [w]), (257, LONG, [h]), (258, SHORT, [bits] * spp), (259, SHORT, [compression]), (262, SHORT, [photometric]),
            (277, SHORT, [spp])]
    if fill_order != 1:
        tags.append((266, SHORT, [fill_order]))
    if orientation is not None:
        tags.append((274, SHORT, [orientation]))
    if planar != 1:
        tags.append((284, SHORT, [planar]))
    if (predictor_tag or predictor) != 1:
        tags.append((317, SHORT, [predictor_tag or predictor]))
    if colormap is not None:
        tags.append((320, SHORT, [int(v) for v in np.asarray(colormap).reshape(-1)]))
    if extra:
        tags.append((338, SHORT, list(extra)))
    if tile:
        tags += [(322, SHORT, [tw]), (323, SHORT, [th]), (324, LONG, None), (325, LONG, [len(c) for c in coded])]
    else:
        if rows_per_strip is not None:
            tags.append((278, LONG, [rows_per_strip]))
        tags += [(273, LONG, None), (279, LONG, [len(c) for c in coded])]
    tags = sorted([t for t in tags if t[0] not in drop] + list(more_tags), key=lambda t: t[0])
    # layout: header, chunks, out-of-line values, IFD
    body = bytearray(b"MM\0*" if big_endian else b"II*\0") + b"\0\0\0\0"
    offsets = []
    for c in coded:
        offsets.append(len(body))
        body += c
        if len(body) & 1:
            body += b"\0"
    size = {BYTE: 1, ASCII: 1, SHORT: 2, LONG: 4, RATIONAL: 8}
    fmt = {BYTE: "B", ASCII: "B", SHORT: "H", LONG: "I"}
    entries = []
    for tid, typ, vals in tags:
        vals = offsets if vals is None else vals
        count = len(vals)
        if typ == RATIONAL:
            blob = b"".join(struct.pack(e + "II", *v) for v in vals)
        else:
            blob = struct.pack(e + fmt[typ] * count, *vals)
        if len(blob) <= 4:
            field = blob + b"\0" * (4 - len(blob))
        else:
            field = struct.pack(e + "I", len(body))
            body += blob
            if len(body) & 1:
                body += b"\0"
        entries.append(struct.pack(e + "HHI", tid, typ, count) + field)
    struct.pack_into(e + "I", body, 4, len(body))
    body += struct.pack(e + "H", len(entries)) + b"".join(entries) + b"\0\0\0\0"
    return bytes(body)


def reduce_colormap(colormap):
    """(3, n) 16-bit -> (n, 3) B,G,R 8-bit the way libtiff's RGBA interface does: >> 8, unless no value is 256 or more"""
    cm = np.asarray(colormap, np.int64)
    if (cm >= 256).any():
        cm = cm >> 8
    return cm[::-1].T.astype(np.uint8)


def convert(samples, bits, photometric, planar=1, extra=None, colormap=None):
    """the pixel rules: stored samples (h, w, spp) -> (h, w, 3) BGR as cv::imdecode(IMREAD_COLOR) returns it (through
    libtiff's RGBA interface, alpha dropped)"""
    s = np.asarray(samples, np.int64)
    h, w, spp = s.shape
    if photometric == PALETTE:
        return reduce_colormap(colormap)[s[:, :, 0]]
    if photometric == CMYK:
        k = 255 - s[:, :, 3]
        return np.stack([k * (255 - s[:, :, c]) // 255 for c in (2, 1, 0)], -1).astype(np.uint8)
    if photometric in (MINISWHITE, MINISBLACK) and (planar == 1 or spp == 1):
        v = s[:, :, 0]
        g = v >> 8 if bits == 16 else v if bits == 8 else v * 255 // ((1 << bits) - 1)
        if photometric == MINISWHITE:
            g = 255 - g
        return np.repeat(g[:, :, None], 3, 2).astype(np.uint8)
    nc = 3 if photometric == RGB else 1
    c = (s + 128) // 257 if bits == 16 else s
    col = c[:, :, :nc]
    if extra and extra[0] == 2:
        col = (col * c[:, :, nc:nc + 1] + 127) // 255
    if nc == 1:
        col = np.repeat(col, 3, 2)
    return col[:, :, ::-1].astype(np.uint8)


def premultiplies(photometric, planar, extra, spp):
    return int(bool(extra) and extra[0] == 2 and (photometric == RGB or (photometric <= 1 and planar == 2 and spp > 1)))


FORMS = [  # (name, photometric, bits, samples per pixel, ExtraSamples): every sample form in scope
    ("white1", MINISWHITE, 1, 1, None), ("black1", MINISBLACK, 1, 1, None), ("black2", MINISBLACK, 2, 1, None), ("white4", MINISWHITE, 4, 1, None),
    ("black4", MINISBLACK, 4, 1, None), ("black8", MINISBLACK, 8, 1, None), ("white8", MINISWHITE, 8, 1, None), ("black16", MINISBLACK, 16, 1, None),
    ("white16", MINISWHITE, 16, 1, None), ("greya8", MINISBLACK, 8, 2, [2]), ("whitea8", MINISWHITE, 8, 2, [2]), ("greya16", MINISBLACK, 16, 2, [1]),
    ("pal1", PALETTE, 1, 1, None), ("pal2", PALETTE, 2, 1, None), ("pal4", PALETTE, 4, 1, None), ("pal8", PALETTE, 8, 1, None),
    ("rgb8", RGB, 8, 3, None), ("rgb16", RGB, 16, 3, None), ("rgba8", RGB, 8, 4, [2]), ("rgbA8", RGB, 8, 4, [1]), ("rgbx8", RGB, 8, 4, [0]),
    ("rgba16", RGB, 16, 4, [2]), ("rgbA16", RGB, 16, 4, [1]), ("rgbxx8", RGB, 8, 5, [0, 0]), ("cmyk8", CMYK, 8, 4, None), ("cmykx8", CMYK, 8, 5, [0]),
]


def random_case(rs, form, h, w):
    """(samples, colormap) of a form of FORMS"""
    _, photometric, bits, spp, _ = form
    samples = rs.randint(0, 1 << bits, (h, w, spp))
    colormap = rs.randint(256, 65536, (3, 1 << bits)) if photometric == PALETTE else None
    return samples, colormap
