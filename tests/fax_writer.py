"""CCITT fax streams and TIFF files for the tests of the fax route (host: host/ccitt_decode.h through tiff::parse / parse_fax /
unfax_all; device: csrc/kernels_tiff_fax.hip), in pure Python: Modified Huffman RLE (Compression 2) and its word-aligned form
(32771), T.4 / Group 3 in one and two dimensions (3) and T.6 / Group 4 (4).  One table of code words, written from ITU-T T.4
tables 2, 3 and 4; an encoder that turns rows into a list of symbols; pack(), which turns any list of symbols - the
encoder's or a hand-built one - into bytes; and write_fax(), which stores such streams through tiff_writer.write_tiff.

A bitmap is (height, width) of 0 (white) and 1 (black) - what the decoder's rows hold, whatever the photometric says."""
import numpy as np

import tiff_writer as tw

MH, MHW, G3, G4 = 2, 32771, 3, 4
WHITE, BLACK = 0, 1

_WHITE_TERM = """00110101 000111 0111 1000 1011 1100 1110 1111 10011 10100 00111 01000 001000 000011 110100 110101 101010 101011
0100111 0001100 0001000 0010111 0000011 0000100 0101000 0101011 0010011 0100100 0011000 00000010 00000011 00011010 00011011
00010010 00010011 00010100 00010101 00010110 00010111 00101000 00101001 00101010 00101011 00101100 00101101 00000100 00000101
00001010 00001011 01010010 01010011 01010100 01010101 00100100 00100101 01011000 01011001 01011010 01011011 01001010 01001011
00110010 00110011 00110100""".split()
_WHITE_MAKE = """11011 10010 010111 0110111 00110110 00110111 01100100 01100101 01101000 01100111 011001100 011001101 011010010
011010011 011010100 011010101 011010110 011010111 011011000 011011001 011011010 011011011 010011000 010011001 010011010 011000
010011011""".split()
_BLACK_TERM = """0000110111 010 11 10 011 0011 0010 00011 000101 000100 0000100 0000101 0000111 00000100 00000111 000011000
0000010111 0000011000 0000001000 00001100111 00001101000 00001101100 00000110111 00000101000 00000010111 00000011000
000011001010 000011001011 000011001100 000011001101 000001101000 000001101001 000001101010 000001101011 000011010010
000011010011 000011010100 000011010101 000011010110 000011010111 000001101100 000001101101 000011011010 000011011011
000001010100 000001010101 000001010110 000001010111 000001100100 000001100101 000001010010 000001010011 000000100100
000000110111 000000111000 000000100111 000000101000 000001011000 000001011001 000000101011 000000101100 000001011010
000001100110 000001100111""".split()
_BLACK_MAKE = """0000001111 000011001000 000011001001 000001011011 000000110011 000000110100 000000110101 0000001101100
0000001101101 0000001001010 0000001001011 0000001001100 0000001001101 0000001110010 0000001110011 0000001110100 0000001110101
0000001110110 0000001110111 0000001010010 0000001010011 0000001010100 0000001010101 0000001011010 0000001011011 0000001100100
0000001100101""".split()
_SHARED_MAKE = """00000001000 00000001100 00000001101 000000010010 000000010011 000000010100 000000010101 000000010110
000000010111 000000011100 000000011101 000000011110 000000011111""".split()
assert (len(_WHITE_TERM), len(_WHITE_MAKE), len(_BLACK_TERM), len(_BLACK_MAKE), len(_SHARED_MAKE)) == (64, 27, 64, 27, 13)

CODES = {  # colour -> {run: code word}: 0 .. 63 terminate a run, 64 .. 2560 (in steps of 64) are make-ups
    WHITE: {**dict(enumerate(_WHITE_TERM)), **{64 * (i + 1): c for i, c in enumerate(_WHITE_MAKE)}, **{1792 + 64 * i: c for i, c in enumerate(_SHARED_MAKE)}},
    BLACK: {**dict(enumerate(_BLACK_TERM)), **{64 * (i + 1): c for i, c in enumerate(_BLACK_MAKE)}, **{1792 + 64 * i: c for i, c in enumerate(_SHARED_MAKE)}},
}
MODES = {"pass": "0001", "horiz": "001", 0: "1", 1: "011", 2: "000011", 3: "0000011", -1: "010", -2: "000010", -3: "0000010"}
EOL = "000000000001"
UNCOMPRESSED = "0000001111"  # the 2-D extension code that enters uncompressed mode


def run_words(colour, n):
    """the code words of a run of n: 2560s while more than 2623 remain, one make-up, one terminating code"""
    out = []
    while n > 2623:
        out.append(CODES[colour][2560])
        n -= 2560
    if n >= 64:
        out.append(CODES[colour][n // 64 * 64])
    out.append(CODES[colour][n % 64])
    return out


# Symbols: ("run", colour, n) a run with its make-ups; ("word", colour, r) the single code word of table entry r (a hand-built
# chain of make-ups); ("pass",) ("horiz",) ("v", d) the 2-D modes; ("eol",); ("bits", "0101") anything; ("zeros", n);
# ("align", m) zeros up to a multiple of m bits; ("eol_aligned",) zeros so that the EOL behind them ends on a byte boundary, and it
def pack(symbols):
    bits = []
    n = 0
    for s in symbols:
        kind = s[0]
        if kind == "run":
            w = "".join(run_words(s[1], s[2]))
        elif kind == "word":
            w = CODES[s[1]][s[2]]
        elif kind == "pass" or kind == "horiz":
            w = MODES[kind]
        elif kind == "v":
            w = MODES[s[1]]
        elif kind == "eol":
            w = EOL
        elif kind == "bits":
            w = s[1]
        elif kind == "zeros":
            w = "0" * s[1]
        elif kind == "align":
            w = "0" * (-n % s[1])
        elif kind == "eol_aligned":
            w = "0" * (-(n + len(EOL)) % 8) + EOL
        else:
            raise ValueError(s)
        bits.append(w)
        n += len(w)
    text = "".join(bits)
    text += "0" * (-len(text) % 8)
    return bytes(int(text[i:i + 8], 2) for i in range(0, len(text), 8))


def changes(row):
    """the changing elements of a row: where the colour differs from the pixel before (white before the row), the first to black"""
    row = np.asarray(row, np.int64)
    return [int(x) for x in np.flatnonzero(np.diff(np.concatenate([[0], row])))]


def row_1d(row):
    """a row as alternating runs, the first white (of length 0 where the row begins black)"""
    w, out, x, colour = len(row), [], 0, WHITE
    for c in changes(row) + [w]:
        out.append(("run", colour, c - x))
        x, colour = c, colour ^ 1
        if x == w and c == w:
            break
    return out


def row_2d(row, ref):
    """a row against its reference row, by the coding procedure of T.4 section 4.2.1.3"""
    w = len(row)
    cur, rf = changes(row), changes(ref)
    out, a0, colour, i = [], -1, WHITE, 0
    while a0 < w:
        while i < len(cur) and cur[i] <= a0:
            i += 1
        a1 = cur[i] if i < len(cur) else w
        a2 = cur[i + 1] if i + 1 < len(cur) else w
        j = colour  # changes to black have even places
        while j < len(rf) and rf[j] <= a0:
            j += 2
        b1 = rf[j] if j < len(rf) else w
        b2 = rf[j + 1] if j + 1 < len(rf) else w
        if b2 < a1:
            out.append(("pass",))
            a0 = b2
        elif abs(a1 - b1) <= 3:
            out.append(("v", a1 - b1))
            a0, colour = a1, colour ^ 1
        else:
            out += [("horiz",), ("run", colour, a1 - max(a0, 0)), ("run", colour ^ 1, a2 - a1)]
            a0 = a2
    return out


def chunk_symbols(rows, compression, t4=0, k=2, fill=False, end=True):
    """the symbols of a chunk.  t4: T4Options (bit 0: two-dimensional, every k-th row 1-D); fill: zeros before each EOL so that it
    ends on a byte boundary - whether or not t4 bit 2 says so; end: the RTC (Compression 3) or EOFB (4) behind the last row"""
    rows = np.asarray(rows)
    out = []
    ref = np.zeros(rows.shape[1], np.int64)
    for y, row in enumerate(rows):
        if compression in (MH, MHW):
            out.append(("align", 8 if compression == MH else 16))
            out += row_1d(row)
        elif compression == G3:
            out.append(("eol_aligned",) if fill else ("eol",))
            if t4 & 1:
                one_d = y % k == 0
                out.append(("bits", "1" if one_d else "0"))
                out += row_1d(row) if one_d else row_2d(row, ref)
            else:
                out += row_1d(row)
        else:
            out += row_2d(row, ref)
        ref = row
    if end and compression == G3:
        out += [("eol",)] + ([("bits", "1")] if t4 & 1 else [])
        out += ([("eol",)] + ([("bits", "1")] if t4 & 1 else [])) * 5
    if end and compression == G4:
        out += [("eol",), ("eol",)]
    return out


def encode(rows, compression, **kw):
    return pack(chunk_symbols(rows, compression, **kw))


def split(bitmap, tile=None, rows_per_strip=None, rs=None):
    """the chunks of a bitmap in file order, as (rows the decoder reads, rows x width bits): a tile at its full size (what lies
    beyond the image: rs's noise, else white), a strip at the rows it has"""
    bitmap = np.asarray(bitmap, np.int64)
    h, w = bitmap.shape
    tw_, th_ = tile if tile else (w, min(h, rows_per_strip or h))
    out = []
    for y0 in range(0, h, th_):
        for x0 in range(0, w, tw_):
            part = bitmap[y0:y0 + th_, x0:x0 + tw_]
            rows = th_ if tile else part.shape[0]
            block = rs.randint(0, 2, (rows, tw_)) if rs is not None else np.zeros((rows, tw_), np.int64)
            block[:part.shape[0], :part.shape[1]] = part
            out.append(block)
    return out, (tw_, th_)


def expanded(bitmap, tile=None, rows_per_strip=None, rs=None):
    """Frame::data of the file write_fax makes with the same arguments (and the same rs state)"""
    blocks, (tw_, th_) = split(bitmap, tile, rows_per_strip, rs)
    parts = []
    for b in blocks:
        full = np.zeros((th_, (tw_ + 7) // 8), np.uint8)
        full[:b.shape[0]] = np.packbits(b.astype(np.uint8), axis=1)
        parts.append(full.tobytes())
    return b"".join(parts)


def write_fax(bitmap, compression, photometric=tw.MINISWHITE, t4=0, k=2, fill=False, end=True, fill_order=1, tile=None, rows_per_strip=None,
              big_endian=False, rs=None, streams=None, more_tags=(), **kw):
    """bitmap -> TIFF file bytes.  streams: coded chunks (before FillOrder) to store instead of the encoder's"""
    bitmap = np.asarray(bitmap, np.int64)
    if streams is None:
        blocks, _ = split(bitmap, tile, rows_per_strip, rs)
        streams = [encode(b, compression, t4=t4 or 0, k=k, fill=fill, end=end) for b in blocks]  # (t4 None: no T4Options tag, which means 0)
    if fill_order == 2:
        streams = [tw._REVERSED[np.frombuffer(s, np.uint8)].tobytes() for s in streams]
    tags = list(more_tags)
    if compression == G3 and t4 is not None:
        tags.append((292, tw.LONG, [t4]))
    return tw.write_tiff(bitmap[:, :, None], 1, photometric, big_endian=big_endian, compression=tw.NONE, tile=tile, rows_per_strip=rows_per_strip,
                         fill_order=fill_order, streams=streams, drop=(259,), more_tags=[(259, tw.SHORT, [compression])] + tags, **kw)


def wanted(bitmap, photometric):
    """the BGR image of a bitmap: white is 255 under MinIsWhite and under MinIsBlack it is 0"""
    return tw.convert(np.asarray(bitmap)[:, :, None], 1, photometric)


# Coded fax frames for the tests of the expansion: what tiff::parse_fax hands over, in the flat form host/tiff_check.cpp reads
# with --unfax (the form of tiff_coded.flat with the T4 options behind the compression)
def coded(bitmap, compression, photometric=tw.MINISWHITE, t4=0, tile=None, rows_per_strip=None, rs=None, streams=None, name=None, **kw):
    """bitmap -> the coded frame (a dict, as tiff_coded.make_coded's) with its chunks coded by encode(**kw), or `streams`"""
    import struct
    bitmap = np.asarray(bitmap, np.int64)
    h, w = bitmap.shape
    blocks, (tw_, th_) = split(bitmap, tile, rows_per_strip, rs)
    if streams is None:
        streams = [encode(b, compression, t4=t4, **kw) for b in blocks]
    records, pool = [], bytearray()
    for b, s in zip(blocks, streams):
        records.append((len(pool), len(s), b.shape[0]))
        pool += s
    return dict(w=w, h=h, photometric=photometric, bits=1, samples=1, planar=1, predictor=1, big_endian=0, premultiply=0, tile=(tw_, th_),
                palette=np.zeros((256, 4), np.uint8), compression=compression, t4=t4, chunks=records, data=bytes(pool), name=name)


def one_chunk(symbols, width, rows, compression, t4=0, tile_height=None, name=None):
    """a hand-built stream as a frame of one strip"""
    s = pack(symbols)
    return dict(w=width, h=rows, photometric=tw.MINISWHITE, bits=1, samples=1, planar=1, predictor=1, big_endian=0, premultiply=0,
                tile=(width, tile_height or rows), palette=np.zeros((256, 4), np.uint8), compression=compression, t4=t4,
                chunks=[(0, len(s), rows)], data=s, name=name)


def flat(c):
    import struct
    import tiff_coded as tc
    out = tc.head(c) + struct.pack("<iIQ", c["compression"], c["t4"], len(c["chunks"]))
    out += b"".join(struct.pack("<QII", *k) for k in c["chunks"])
    return out + struct.pack("<Q", len(c["data"])) + c["data"]


def host_unfax(exe, codeds, directory, tag="x"):
    """tiff::unfax_all (tiff_check --unfax, one process) over sound fax frames: the expanded chunks of each"""
    import os
    import subprocess
    import tiff_coded as tc
    src, out = os.path.join(str(directory), tag + ".fax"), os.path.join(str(directory), tag + ".chunks")
    with open(src, "wb") as f:
        for c in codeds:
            f.write(flat(c))
    r = subprocess.run([exe, "--unfax", src, out], capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    data = np.fromfile(out, np.uint8)
    res, pos = [], 0
    for c in codeds:
        n = tc.nominal(c)
        res.append(data[pos:pos + n])
        pos += n
    assert pos == len(data)
    return res


def to_pkg(pkg, c):
    return pkg.TiffFax(c["w"], c["h"], c["photometric"], c["compression"], c["chunks"], c["data"], tile=c["tile"], t4_options=c["t4"])


CODINGS = [  # (name, compression, arguments of write_fax / coded): every coding in scope
    ("mh", MH, {}), ("mhw", MHW, {}), ("g3", G3, {}), ("g3-2d", G3, dict(t4=1, k=2)), ("g3-fill", G3, dict(t4=4, fill=True)), ("g4", G4, {}),
]


def branch_bitmaps():
    """[(name, bitmap)]: the bitmaps that reach each branch of the decoder"""
    out = []
    w = 40
    out.append(("all white", np.zeros((3, w), int)))
    out.append(("all black", np.ones((3, w), int)))
    out.append(("alternating pixels, white first", np.tile(np.arange(w) % 2, (3, 1))))
    out.append(("alternating pixels, black first", np.tile((np.arange(w) + 1) % 2, (3, 1))))
    b = np.zeros((4, w), int)
    b[:, :5] = 1
    out.append(("black from column 0", b))
    base = (np.arange(64) // 9) % 2
    for d in range(-4, 5):  # stripes that shift by d a row: every vertical mode, and +-4 the horizontal one
        out.append(("stripes shifting by %d" % d, np.stack([np.roll(base, d * y) for y in range(6)])))
    b = np.zeros((4, 48), int)
    b[0, 5:9] = 1; b[0, 14:17] = 1; b[0, 30:40] = 1   # runs of the reference row wholly left of the next change below:
    b[1, 32:38] = 1                                    # two passes in a row
    b[2, 3:6] = 1; b[2, 32:38] = 1
    b[3, 40:44] = 1                                    # and one pass
    out.append(("pass modes", b))
    for n in (63, 64, 65, 1791, 1792, 1793, 2560, 2561, 5200):
        b = np.zeros((2, n + 2), int)
        b[0, n:n + 1] = 1      # a white run of n
        b[1, 1:n + 1] = 1      # a black run of n
        out.append(("runs of %d" % n, b))
    return out


def many_strips(n):
    """an all-white Group 4 file of width 1 and n rows in n strips of one row (each the byte 0x80: V0), written by hand - the
    general writer walks every chunk in Python: more chunks than the device stage takes when n > 2 ** 20"""
    import struct
    body = bytearray(b"II*\0\0\0\0\0") + b"\x80" * n
    if len(body) & 1:
        body += b"\0"
    offs = len(body)
    body += struct.pack("<%dI" % n, *range(8, 8 + n))
    counts = len(body)
    body += struct.pack("<%dI" % n, *([1] * n))
    tags = [(256, 4, 1, 1), (257, 4, 1, n), (258, 3, 1, 1), (259, 3, 1, G4), (262, 3, 1, 0), (273, 4, n, offs), (277, 3, 1, 1), (278, 4, 1, 1), (279, 4, n, counts)]
    struct.pack_into("<I", body, 4, len(body))
    body += struct.pack("<H", len(tags))
    for tid, typ, count, value in tags:
        body += struct.pack("<HHI", tid, typ, count) + (struct.pack("<HH", value, 0) if typ == 3 else struct.pack("<I", value))
    return bytes(body + b"\0\0\0\0")
