"""BMP and PNM files of every form the service reads, written from known arrays, and the BGR image cv::imdecode's rules
give for those arrays - in numpy, independent of host/raw_decode.h (the counterpart of png_writer.py / jpeg_writer.py).

BMP: write_bmp() + expected_bmp(); run-length streams: rle_encode() (encoded runs, absolute runs, end-of-line, moves).
PNM: write_pnm() + expected_pnm().  Stored rows for the C-ABI descriptor (ocr_raw_frame): KINDS, row_bytes(),
random_rows(), convert_rows()."""
import struct

import numpy as np

# ---------------------------------------------------------------------------------------------- BMP


def _pack_rows(arr, bpp):
    """(h, w[, c]) samples -> (h, row bytes) uint8, top row first, without padding"""
    h, w = arr.shape[:2]
    if bpp == 1:
        return np.packbits(arr.astype(np.uint8) & 1, axis=1)
    if bpp == 4:
        a = arr.astype(np.uint8) & 15
        if w % 2:
            a = np.concatenate([a, np.zeros((h, 1), np.uint8)], 1)
        return (a[:, 0::2] << 4) | a[:, 1::2]
    if bpp == 8:
        return arr.astype(np.uint8)
    if bpp == 16:
        return arr.astype("<u2").view(np.uint8).reshape(h, 2 * w)
    return arr.astype(np.uint8).reshape(h, -1)  # 24: B,G,R; 32: B,G,R,A


def write_bmp(arr, bpp, header=40, top_down=False, palette=None, compression=0, masks=None, clr_used=None, stream=None, gap=0,
              drop_last_padding=False):
    """arr: (h, w) indices (bpp <= 8), (h, w) 16-bit words, (h, w, 3) BGR or (h, w, 4) BGRA, top row first.
    palette: (n, 3) B,G,R - n entries are written, biClrUsed = clr_used (default n when n != 1 << bpp, else 0).
    stream: a ready run-length stream (compression 1 / 2) in place of the rows.  gap: bytes between the tables and the data."""
    h, w = arr.shape[:2]
    if stream is None:
        rows = _pack_rows(arr, bpp)
        stride = (w * bpp + 31) // 32 * 4
        rows = np.concatenate([rows, np.zeros((h, stride - rows.shape[1]), np.uint8)], 1)
        if not top_down:
            rows = rows[::-1]
        body = rows.tobytes()
        if drop_last_padding and stride > (w * bpp + 7) // 8:
            body = body[:len(body) - (stride - (w * bpp + 7) // 8)]
    else:
        body = bytes(stream)
    tables = b""
    if masks is not None and header == 40:
        tables += struct.pack("<III", *masks)
    n = 0
    if palette is not None:
        pal = np.asarray(palette, np.uint8).reshape(-1, 3)
        n = len(pal)
        if header == 12:
            tables += pal.tobytes()
        else:
            tables += np.concatenate([pal, np.zeros((n, 1), np.uint8)], 1).tobytes()
    if clr_used is None:
        clr_used = n if (palette is not None and n != (1 << bpp)) else 0
    if header == 12:
        assert not top_down and compression == 0
        info = struct.pack("<IHHHH", 12, w, h, 1, bpp)
    else:
        info = struct.pack("<IiiHHIIiiII", header, w, -h if top_down else h, 1, bpp, compression, len(body), 2835, 2835, clr_used, 0)
        if header > 40:
            m = tuple(masks) if masks is not None else (0, 0, 0)
            info += struct.pack("<III", *m)
            info += b"\0" * (header - len(info))
    off = 14 + len(info) + len(tables) + gap
    return b"BM" + struct.pack("<IHHI", off + len(body), 0, 0, off) + info + tables + b"\0" * gap + body


def lookup(idx, palette):
    """indices through a B,G,R palette of 256 entries, zero beyond the given ones"""
    full = np.zeros((256, 3), np.uint8)
    if palette is not None:
        p = np.asarray(palette, np.uint8).reshape(-1, 3)
        full[:len(p)] = p
    return full[np.asarray(idx).astype(np.int64)]


def expand16(t, is565):
    """5-5-5 / 5-6-5 words -> BGR by shifting: the low bits stay zero"""
    t = np.asarray(t).astype(np.uint32)
    b = (t << 3) & 0xFF
    g = (t >> 3) & 0xFC if is565 else (t >> 2) & 0xF8
    r = (t >> 8) & 0xF8 if is565 else (t >> 7) & 0xF8
    return np.stack([b, g, r], -1).astype(np.uint8)


def expected_bmp(arr, bpp, palette=None, is565=False):
    if bpp <= 8:
        return lookup(arr, palette)
    if bpp == 16:
        return expand16(arr, is565)
    return np.ascontiguousarray(arr[:, :, :3]).astype(np.uint8)


def random_bmp_samples(rs, h, w, bpp):
    if bpp <= 8:
        return rs.randint(0, 1 << bpp, (h, w))
    if bpp == 16:
        return rs.randint(0, 1 << 16, (h, w))
    return rs.randint(0, 256, (h, w, bpp // 8))


def rle_encode(idx, bpp, rs, skip=0.15, truncate_at=None):
    """(stream, expected indices).  idx: (h, w) indices, top row first (8 bpp: RLE8, 4 bpp: RLE4).  The encoder walks the rows
    bottom-up and picks at random between encoded runs, absolute runs (3 .. 255 pixels, padded to 16 bits) and skips - a move
    (00 02 dx 0) inside a row, an early end-of-line, or a move over whole rows (00 02 dx dy); skipped pixels are never
    written: index 0 is expected there.  truncate_at: the stream is cut after that many bytes; the pixels of the operations
    that no longer fit completely are expected as far as their bytes are there."""
    h, w = idx.shape
    want = np.zeros((h, w), np.int64)
    out = bytearray()
    ops = []  # (stream offset after the op, [(y, x, n)] pixels written)
    nib = bpp == 4
    y = h - 1  # top-first row index of the stored row being written
    x = 0
    while y >= 0:
        row = idx[y]
        while x < w:
            left = w - x
            u = rs.rand()
            if u < skip and left > 1:
                dx = int(rs.randint(1, min(left, 255) + 1))
                out += bytes([0, 2, dx, 0])
                x += dx
                ops.append((len(out), []))
            elif u < skip * 1.3:
                break  # early end of line: the rest of the row stays unwritten
            elif u < 0.6 and left >= 3:
                n = int(rs.randint(3, min(left, 255) + 1))
                px = row[x:x + n]
                if nib:
                    p = np.concatenate([px, np.zeros(n % 2, np.int64)])
                    data = bytes(((p[0::2] << 4) | p[1::2]).astype(np.uint8))
                else:
                    data = bytes(px.astype(np.uint8))
                out += bytes([0, n]) + data + b"\0" * (len(data) % 2)
                ops.append((len(out), [(y, x, n, "abs", len(out) - len(data) - len(data) % 2)]))
                x += n
            else:
                a = int(row[x])
                b = int(row[x + 1]) if (nib and left > 1) else a
                n = 1
                while x + n < w and n < 255 and int(row[x + n]) == (a if n % 2 == 0 else b):
                    n += 1
                n = int(rs.randint(1, n + 1))
                out += bytes([n, (a << 4) | b if nib else a])
                ops.append((len(out), [(y, x, n, "run", 0)]))
                x += n
        # to the next stored row (the one above): end of line, or a move over rows now and then
        if y > 1 and rs.rand() < 0.2:
            dy = int(rs.randint(1, min(y, 3) + 1))
            dx = int(rs.randint(0, 3)) if w > 3 else 0
            out += bytes([0, 0])  # x = 0, one row up
            out += bytes([0, 2, dx, dy - 1]) if (dy > 1 or dx) else b""
            ops.append((len(out), []))
            y -= dy
            x = dx
        else:
            out += bytes([0, 0])
            ops.append((len(out), []))
            y -= 1
            x = 0
    out += bytes([0, 1])
    cut = len(out) if truncate_at is None else min(truncate_at, len(out))
    for end, writes in ops:
        for (yy, xx, n, kind, data_at) in writes:
            if end <= cut:
                want[yy, xx:xx + n] = idx[yy, xx:xx + n]
            elif kind == "abs" and data_at - 2 + 2 <= cut:  # the two header bytes are there: the pixels whose bytes are too
                have = max(0, cut - data_at)
                m = min(n, have * 2 if nib else have)
                want[yy, xx:xx + m] = idx[yy, xx:xx + m]
    return bytes(out[:cut]), want


# ---------------------------------------------------------------------------------------------- PNM

def write_pnm(ptype, s, maxval=255, comments=True, rs=None):
    """ptype 1 .. 6; s: (h, w, c) samples (c = 1 for P1 / P2 / P4 / P5, 3 for P3 / P6; P1 / P4: 1 = black).  ASCII values
    are written as given - also above maxval."""
    h, w, c = s.shape
    head = b"P%d\n" % ptype
    if comments:
        head += b"# a comment\n"
    head += b"%d" % w + (b" # another\n" if comments else b" ") + b"%d" % h
    if ptype not in (1, 4):
        head += b"\n#third\n%d" % maxval if comments else b"\n%d" % maxval
    if ptype == 1:
        body = b"\n".join(b"".join(b"%d" % v for v in row) if (i % 2) else b" ".join(b"%d" % v for v in row) for i, row in enumerate(s[:, :, 0]))
        return head + b"\n" + body + b"\n"
    if ptype in (2, 3):
        flat = s.reshape(h, -1)
        body = b"\n".join(b" ".join(b"%d" % v for v in row) for row in flat)
        return head + b"\n" + (b"# in the raster\n" if comments else b"") + body + b"\n"
    if ptype == 4:
        return head + b"\n" + np.packbits(s[:, :, 0].astype(np.uint8) & 1, axis=1).tobytes()
    flat = s.reshape(h, -1)
    return head + b"\n" + (flat.astype(">u2").tobytes() if maxval > 255 else flat.astype(np.uint8).tobytes())


def expected_pnm(ptype, s, maxval=255):
    s = np.asarray(s).astype(np.int64)
    if ptype in (1, 4):
        v = np.where(s[:, :, 0] != 0, 0, 255)
        return np.stack([v, v, v], -1).astype(np.uint8)
    s = np.minimum(s, maxval)  # (only ASCII files can exceed it)
    v = s >> 8 if maxval > 255 else s  # the high byte of a 16-bit sample; 8-bit samples as they are: no rescaling
    if s.shape[2] == 1:
        return np.repeat(v, 3, 2).astype(np.uint8)
    return v[:, :, ::-1].astype(np.uint8)


# ---------------------------------------------------------------------------------------------- stored rows (ocr_raw_frame)

KINDS = ["INDEX1", "INDEX4", "INDEX8", "BGR555", "BGR565", "BGR24", "BGRX32", "RGB24", "GREY8", "GREY16BE", "RGB48BE", "BIT1_INV"]


def row_bytes(kind, w):
    name = KINDS[kind]
    return {"INDEX1": (w + 7) // 8, "BIT1_INV": (w + 7) // 8, "INDEX4": (w + 1) // 2, "INDEX8": w, "GREY8": w, "BGR555": 2 * w, "BGR565": 2 * w,
            "GREY16BE": 2 * w, "BGR24": 3 * w, "RGB24": 3 * w, "BGRX32": 4 * w, "RGB48BE": 6 * w}[name]


def convert_rows(kind, rows, w, palette, bottom_up):
    """rows: (h, stride) uint8 stored rows -> (h, w, 3) BGR by the rules of include/ocr_hip.h.  palette: (256, 4) B,G,R,x"""
    name = KINDS[kind]
    r = rows[:, :row_bytes(kind, w)]
    h = r.shape[0]
    pal = np.asarray(palette, np.uint8).reshape(256, 4)[:, :3]
    if name in ("INDEX1", "BIT1_INV"):
        bits = np.unpackbits(r, axis=1)[:, :w]
        out = pal[bits] if name == "INDEX1" else np.repeat(np.where(bits != 0, 0, 255)[:, :, None], 3, 2)
    elif name == "INDEX4":
        nibbles = np.stack([r >> 4, r & 15], -1).reshape(h, -1)[:, :w]
        out = pal[nibbles]
    elif name == "INDEX8":
        out = pal[r]
    elif name in ("BGR555", "BGR565"):
        out = expand16(r.reshape(h, w, 2)[:, :, 0].astype(np.uint32) | (r.reshape(h, w, 2)[:, :, 1].astype(np.uint32) << 8), name == "BGR565")
    elif name == "BGR24":
        out = r.reshape(h, w, 3)
    elif name == "BGRX32":
        out = r.reshape(h, w, 4)[:, :, :3]
    elif name == "RGB24":
        out = r.reshape(h, w, 3)[:, :, ::-1]
    elif name == "GREY8":
        out = np.repeat(r[:, :, None], 3, 2)
    elif name == "GREY16BE":
        out = np.repeat(r.reshape(h, w, 2)[:, :, :1], 3, 2)
    else:
        out = r.reshape(h, w, 3, 2)[:, :, ::-1, 0]
    out = np.ascontiguousarray(out).astype(np.uint8)
    return np.ascontiguousarray(out[::-1]) if bottom_up else out
