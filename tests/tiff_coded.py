"""Coded TIFF frames for the tests of the chunk expansion (host: tiff::parse_coded / tiff::expand of host/tiff_decode.h; device:
csrc/kernels_tiff_lzw.hip): LZW streams built code by code, coded frames made from samples with tests/tiff_writer.py's
encoders, the flat form host/tiff_check.cpp reads and writes, and the mutations of the extent-scan corpus."""
import os
import struct
import subprocess

import numpy as np

import tiff_writer as tw

CLEAR, EOI = 256, 257


def lzw_codes(data, clear_first=True, end=True):
    """the greedy LZW code list of `data` (a table reset with a clear code at 4094 entries, as tiff_writer.lzw_encode)"""
    codes = [CLEAR] if clear_first else []
    table, nxt = {}, 258
    if len(data):
        ent = data[0]
        for c in data[1:]:
            key = (ent << 8) | c
            if key in table:
                ent = table[key]
                continue
            codes.append(ent)
            table[key] = nxt
            nxt += 1
            ent = c
            if nxt == 4094:
                codes.append(CLEAR)
                table, nxt = {}, 258
        codes.append(ent)
    if end:
        codes.append(EOI)
    return codes


def pack_codes(codes):
    """codes -> bytes, most significant bit first, at the widths a TIFF decoder reads them with: 9 bits behind a clear, one more
    once 511 / 1023 / 2047 entries exist (an entry is made by every code but the first behind a clear)"""
    out, acc, have = bytearray(), 0, 0
    bits, nxt, first = 9, 258, True
    for code in codes:
        acc = (acc << bits) | code
        have += bits
        while have >= 8:
            out.append((acc >> (have - 8)) & 0xFF)
            have -= 8
        acc &= (1 << have) - 1
        if code == CLEAR:
            bits, nxt, first = 9, 258, True
        elif code == EOI:
            pass
        elif first:
            first = False
        else:
            nxt += 1
            if nxt > (1 << bits) - 2 and bits < 12:
                bits += 1
    if have:
        out.append((acc << (8 - have)) & 0xFF)
    return bytes(out)


def grey_strip(stream, need, compression=tw.LZW, rows=1, tile_height=None):
    """one chunk as a coded frame: 8-bit grey, one strip of `rows` rows of need // rows bytes"""
    width = need // rows
    return dict(w=width, h=rows, photometric=tw.MINISBLACK, bits=8, samples=1, planar=1, predictor=1, big_endian=0, premultiply=0,
                tile=(width, tile_height or rows), palette=np.zeros((256, 4), np.uint8), compression=compression,
                chunks=[(0, len(stream), rows)], data=bytes(stream))


def make_coded(samples, form, compression, planar=1, predictor=1, big_endian=False, tile=None, rows_per_strip=None, colormap=None, rs=None):
    """samples of a form of tiff_writer.FORMS -> the coded frame tiff::parse_coded would hand over, and the expanded chunks"""
    name, photometric, bits, spp, extra = form
    chunks, (tw_, th_) = tw.chunk_list(samples, bits, planar=planar, predictor=predictor, tile=tile, rows_per_strip=rows_per_strip, big_endian=big_endian, rs=rs)
    records, pool, expanded = [], bytearray(), []
    for block, rows in chunks:
        raw = block[:block.shape[0] if tile else rows].tobytes()
        c = tw.compress(raw, compression, block.shape[1])
        records.append((len(pool), len(c), block.shape[0] if tile else rows))
        pool += c
        full = np.zeros((th_, block.shape[1]), np.uint8)
        full[:block.shape[0]] = block
        expanded.append(full.tobytes())
    palette = np.zeros((256, 4), np.uint8)
    if colormap is not None:
        palette[:1 << bits, :3] = tw.reduce_colormap(colormap)
    h, w = np.asarray(samples).shape[:2]
    coded = dict(w=w, h=h, photometric=photometric, bits=bits, samples=spp, planar=planar if spp > 1 else 1, predictor=predictor, big_endian=int(big_endian),
                 premultiply=tw.premultiplies(photometric, planar, extra, spp), tile=(tw_, th_), palette=palette, compression=compression,
                 chunks=records, data=bytes(pool))
    return coded, b"".join(expanded)


def head(c):
    return struct.pack("<11i", c["w"], c["h"], c["photometric"], c["bits"], c["samples"], c["planar"], c["predictor"], c["big_endian"], c["premultiply"],
                       *c["tile"]) + np.asarray(c["palette"], np.uint8).tobytes()


def flat(c):
    """the flat little-endian form of host/tiff_check.cpp --coded / --expand"""
    out = head(c) + struct.pack("<iQ", c["compression"], len(c["chunks"]))
    out += b"".join(struct.pack("<QII", *k) for k in c["chunks"])
    return out + struct.pack("<Q", len(c["data"])) + c["data"]


def nominal(c):
    planes = c["samples"] if c["planar"] == 2 else 1
    row = (c["tile"][0] * (1 if c["planar"] == 2 else c["samples"]) * c["bits"] + 7) // 8
    return row * c["tile"][1] * (-(-c["w"] // c["tile"][0])) * (-(-c["h"] // c["tile"][1])) * planes


def host_expand(exe, codeds, directory, tag="x"):
    """tiff::expand (tiff_check --expand, one process) over sound coded frames: the expanded chunks of each"""
    src, out = os.path.join(str(directory), tag + ".coded"), os.path.join(str(directory), tag + ".chunks")
    with open(src, "wb") as f:
        for c in codeds:
            f.write(flat(c))
    r = subprocess.run([exe, "--expand", src, out], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    data = np.fromfile(out, np.uint8)
    res, pos = [], 0
    for c in codeds:
        n = nominal(c)
        res.append(data[pos:pos + n])
        pos += n
    assert pos == len(data)
    return res


def to_pkg(pkg, c):
    return pkg.TiffCoded(c["w"], c["h"], c["photometric"], c["bits"], c["samples"], c["compression"], c["chunks"], c["data"], tile=c["tile"], planar=c["planar"],
                         predictor=c["predictor"], big_endian=c["big_endian"], premultiply=c["premultiply"], palette=c["palette"])


def mutate(rs, stream, others):
    """a cut, a bit flip, a byte splice from another stream, or the stream as it is"""
    s = bytearray(stream)
    kind = rs.randint(4)
    if kind == 0 and len(s) > 1:
        del s[rs.randint(1, len(s)):]
    elif kind == 1 and len(s):
        i = rs.randint(len(s))
        s[i] ^= 1 << rs.randint(8)
    elif kind == 2 and len(s) > 2:
        o = others[rs.randint(len(others))]
        n = rs.randint(1, 8)
        i, j = rs.randint(len(s)), rs.randint(max(1, len(o) - n))
        s[i:i + n] = o[j:j + n]
    return bytes(s)


def corpus(seed=5, count=2400):
    """[(compression, need, stream)]: LZW and PackBits streams of text-like, run-heavy and random rows, cut, bit-flipped and
    byte-spliced, with `need` at, below and above what the sound stream holds; and pure random bytes"""
    rs = np.random.RandomState(seed)
    bases = []
    for k in range(24):
        n = int(rs.choice([1, 2, 7, 64, 300, 900, 3000, 9000]))
        kind = k % 3
        if kind == 0:
            data = rs.randint(0, 256, n).astype(np.uint8).tobytes()
        elif kind == 1:
            data = np.repeat(rs.randint(0, 4, n // 8 + 1), 8)[:n].astype(np.uint8).tobytes()
        else:
            data = (b"the quick brown fox " * (n // 20 + 1))[:n]
        bases.append((tw.LZW, data, tw.lzw_encode(data)))
        bases.append((tw.PACKBITS, data, tw.packbits_encode(data, max(1, n // 3))))
    streams = {comp: [b[2] for b in bases if b[0] == comp] for comp in (tw.LZW, tw.PACKBITS)}
    out = []
    while len(out) < count - 200:
        comp, data, stream = bases[rs.randint(len(bases))]
        need = max(1, int(len(data) * rs.choice([0.5, 0.9, 1.0, 1.0, 1.0, 1.1])) + int(rs.choice([-1, 0, 0, 1])))
        out.append((comp, need, mutate(rs, stream, streams[comp])))
    while len(out) < count:
        n = rs.randint(0, 200)
        out.append((tw.LZW if len(out) & 1 else tw.PACKBITS, rs.randint(1, 400), (b"\x80\x00" if rs.randint(2) else b"") + rs.randint(0, 256, n).astype(np.uint8).tobytes()))
    return out
