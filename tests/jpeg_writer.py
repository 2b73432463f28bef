"""A small deterministic baseline JPEG writer in numpy (test helper for tests/test_jpeg_formats.py and
tests/test_gpu_jpeg_formats.py).  Pillow writes only 4:4:4 / 4:2:2 / 4:2:0 YCbCr, grey and Adobe CMYK; the decoder also takes
every integral sampling, YCCK, Adobe RGB and files without a marker, so those files are made here: float DCT, one fixed
quantisation table per quality, the Annex K Huffman tables, 1..5 components with arbitrary per-component (h, v), an optional
JFIF or Adobe APP14 marker, chosen component ids, an optional restart interval, interleaved or per-component scans.  How
good the encoder is does not matter: the expectation of every test is Pillow's decode of the same bytes.

relabel() is the independent cross-check of the writer: a Pillow-written file whose SOF sampling byte and size are changed
so that the MCU block counts stay equal is a valid stream of another sampling."""
import struct

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# ITU-T T.81 Annex K.1 (luminance) in natural order
K1 = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
               18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])


def _run(a, b):
    return list(range(a, b + 1))


# Annex K.3: (bits[16], values) of the DC / AC tables for luminance (index 0) and chrominance (index 1)
DC_TABLES = [([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], _run(0, 11)),
             ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], _run(0, 11))]
AC_TABLES = [
    ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
     [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
      0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a] + _run(0x16, 0x1a) + _run(0x25, 0x2a) +
     _run(0x34, 0x3a) + _run(0x43, 0x4a) + _run(0x53, 0x5a) + _run(0x63, 0x6a) + _run(0x73, 0x7a) + _run(0x83, 0x8a) + _run(0x92, 0x9a) +
     _run(0xa2, 0xaa) + _run(0xb2, 0xba) + _run(0xc2, 0xca) + _run(0xd2, 0xda) + _run(0xe1, 0xea) + _run(0xf1, 0xfa)),
    ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
     [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
      0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1] + _run(0x17, 0x1a) +
     _run(0x26, 0x2a) + _run(0x35, 0x3a) + _run(0x43, 0x4a) + _run(0x53, 0x5a) + _run(0x63, 0x6a) + _run(0x73, 0x7a) + _run(0x82, 0x8a) +
     _run(0x92, 0x9a) + _run(0xa2, 0xaa) + _run(0xb2, 0xba) + _run(0xc2, 0xca) + _run(0xd2, 0xda) + _run(0xe2, 0xea) + _run(0xf2, 0xfa)),
]


def _codes(bits, vals):
    """symbol -> (code, length) of the canonical code"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def quant_table(quality):
    """libjpeg's scaling of Annex K.1 (one table for every component), natural order"""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((K1 * scale + 50) // 100, 1, 255).astype(np.int64)


_C = np.array([[(np.sqrt(0.125) if u == 0 else 0.5) * np.cos((2 * x + 1) * u * np.pi / 16) for x in range(8)] for u in range(8)])


def _blocks(plane, bw, bh, q):
    """(bh, bw, 64) quantised coefficients in natural order of a plane edge-padded to whole blocks"""
    p = np.pad(plane.astype(np.float64), ((0, bh * 8 - plane.shape[0]), (0, bw * 8 - plane.shape[1])), mode="edge") - 128.0
    b = p.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
    d = np.einsum("ux,abxy,vy->abuv", _C, b, _C).reshape(bh, bw, 64)
    return np.rint(d / q).astype(np.int64)


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            self.n -= 8
            byte = (self.acc >> self.n) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _category(v):
    return int(abs(int(v))).bit_length()


def _encode_block(bits, blk, pred, dc, ac):
    diff = int(blk[0]) - pred
    s = _category(diff)
    bits.put(*dc[s])
    if s:
        bits.put(diff if diff >= 0 else diff + (1 << s) - 1, s)
    run = 0
    zz = blk[ZIGZAG]
    last = int(np.max(np.nonzero(zz)[0])) if zz[1:].any() else 0
    for k in range(1, last + 1):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            bits.put(*ac[0xF0])
            run -= 16
        s = _category(v)
        bits.put(*ac[(run << 4) | s])
        bits.put(v if v >= 0 else v + (1 << s) - 1, s)
        run = 0
    if last < 63:
        bits.put(*ac[0x00])
    return int(blk[0])


def _segment(marker, payload):
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + payload


def _dht(tc, th, table):
    bits, vals = table
    return _segment(0xC4, bytes([(tc << 4) | th]) + bytes(bits) + bytes(vals))


def write_jpeg(planes, factors, quality=90, jfif=False, adobe=None, ids=None, restart=0, interleaved=True, segments=()):
    """planes: one (rows, cols) uint8 array per component at full resolution (point-sampled down to the component's own
    size); factors: [(h, v)] per component; adobe: the transform byte of an APP14 marker, None for no marker; ids: the
    component ids (default 1, 2, ...); segments: raw marker segments put in front of the tables (an Exif APP1, say)."""
    n = len(planes)
    rows, cols = planes[0].shape
    ids = list(ids) if ids is not None else list(range(1, n + 1))
    hmax, vmax = max(h for h, _ in factors), max(v for _, v in factors)
    if n == 1:
        hmax = vmax = 1                      # a single component is never subsampled (its factors are still written)
    mcux, mcuy = -(-cols // (8 * hmax)), -(-rows // (8 * vmax))
    q = quant_table(quality)
    comps = []
    for i, ((h, v), plane) in enumerate(zip(factors, planes)):
        if n == 1:
            eh = ev = 1
        else:
            eh, ev = h, v
        dw, dh = -(-cols * eh // hmax), -(-rows * ev // vmax)
        ys = np.minimum(np.arange(dh) * vmax // ev, rows - 1)
        xs = np.minimum(np.arange(dw) * hmax // eh, cols - 1)
        small = plane[np.ix_(ys, xs)]
        bw, bh = mcux * eh, mcuy * ev
        comps.append(dict(h=eh, v=ev, dw=dw, dh=dh, bw=bw, bh=bh, coef=_blocks(small, bw, bh, q), t=0 if i == 0 else 1))
    out = bytearray(b"\xff\xd8")
    if jfif:
        out += _segment(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    if adobe is not None:
        out += _segment(0xEE, b"Adobe\x00\x64\x00\x00\x00\x00" + bytes([adobe]))
    for s in segments:
        out += s
    out += _segment(0xDB, bytes([0]) + bytes(int(x) for x in q[ZIGZAG]))
    out += _segment(0xC0, struct.pack(">BHHB", 8, rows, cols, n) +
                    b"".join(bytes([ids[i], (factors[i][0] << 4) | factors[i][1], 0]) for i in range(n)))
    for t in (0, 1):
        out += _dht(0, t, DC_TABLES[t]) + _dht(1, t, AC_TABLES[t])
    if restart:
        out += _segment(0xDD, struct.pack(">H", restart))
    dc = [_codes(*t) for t in DC_TABLES]
    ac = [_codes(*t) for t in AC_TABLES]

    def scan(members):
        hdr = bytes([len(members)]) + b"".join(bytes([ids[i], (comps[i]["t"] << 4) | comps[i]["t"]]) for i in members) + b"\x00\x3f\x00"
        data = bytearray(_segment(0xDA, hdr))
        bits, pred, done, rst = _Bits(), {i: 0 for i in members}, 0, 0
        if len(members) == 1:
            c = comps[members[0]]
            units = [[(members[0], by, bx)] for by in range(-(-c["dh"] // 8)) for bx in range(-(-c["dw"] // 8))]
        else:
            units = [[(i, my * comps[i]["v"] + by, mx * comps[i]["h"] + bx) for i in members for by in range(comps[i]["v"]) for bx in range(comps[i]["h"])]
                     for my in range(mcuy) for mx in range(mcux)]
        for unit in units:
            if restart and done and done % restart == 0:
                bits.flush()
                bits.out += bytes([0xFF, 0xD0 + rst])
                rst = (rst + 1) & 7
                pred = {i: 0 for i in members}
            for i, by, bx in unit:
                pred[i] = _encode_block(bits, comps[i]["coef"][by, bx], pred[i], dc[comps[i]["t"]], ac[comps[i]["t"]])
            done += 1
        bits.flush()
        return bytes(data) + bytes(bits.out)

    if interleaved and n > 1:
        out += scan(list(range(n)))
    else:
        for i in range(n):
            out += scan([i])
    return bytes(out) + b"\xff\xd9"


def relabel(data, old, new, swap):
    """a Pillow-written 3-component file with luma's sampling byte `old` turned into `new` (and width / height swapped when the
    MCU changes from wide to tall): the entropy-coded data stays a valid stream of the new sampling"""
    p = data.index(b"\xff\xc0")
    b = bytearray(data)
    height, width = struct.unpack(">HH", data[p + 5:p + 9])
    assert b[p + 9] == 3 and b[p + 11] == old and b[p + 14] == 0x11 and b[p + 17] == 0x11
    b[p + 11] = new
    if swap:
        b[p + 5:p + 9] = struct.pack(">HH", width, height)
    return bytes(b)
