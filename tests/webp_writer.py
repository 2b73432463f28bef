"""A lossless WebP (VP8L) writer for the tests, bit by bit, and `convert`: the numpy statement of the inverse transforms.

The writer takes the CODED data - the entropy-coded ARGB image and the transforms with their sub-images, exactly what
webp::parse hands over - so every decoder branch gets a file whether libwebp's encoder would write it or not: any transform
order, any predictor mode in any block, palette indices beyond the palette, any colour-cache size, back references with any
distance code, several prefix-code groups, both code forms.  What such a file decodes to is `convert` of the coded data; the
tests hold libwebp, the host decoder, `convert` and the device stage against each other.  `encode` goes the other way for a
real image (subtract-green, cross-colour and predictor applied forwards) where a test needs a file OF an image.

A pixel is a uint32 A << 24 | R << 16 | G << 8 | B; images are (h, w) uint32 arrays."""
import heapq
import struct

import numpy as np

PREDICTOR, CROSS_COLOUR, ADD_GREEN, COLOUR_INDEXING = 0, 1, 2, 3
BLACK = 0xFF000000

# the 120 short distance codes: (dy << 4) | (8 - dx)  (the format specification's table)
SHORT = [0x18, 0x07, 0x17, 0x19, 0x28, 0x06, 0x27, 0x29, 0x16, 0x1a, 0x26, 0x2a, 0x38, 0x05, 0x37, 0x39, 0x15, 0x1b, 0x36, 0x3a, 0x25, 0x2b, 0x48, 0x04,
         0x47, 0x49, 0x14, 0x1c, 0x35, 0x3b, 0x46, 0x4a, 0x24, 0x2c, 0x58, 0x45, 0x4b, 0x34, 0x3c, 0x03, 0x57, 0x59, 0x13, 0x1d, 0x56, 0x5a, 0x23, 0x2d,
         0x44, 0x4c, 0x55, 0x5b, 0x33, 0x3d, 0x68, 0x02, 0x67, 0x69, 0x12, 0x1e, 0x66, 0x6a, 0x22, 0x2e, 0x54, 0x5c, 0x43, 0x4d, 0x65, 0x6b, 0x32, 0x3e,
         0x78, 0x01, 0x77, 0x79, 0x53, 0x5d, 0x11, 0x1f, 0x64, 0x6c, 0x42, 0x4e, 0x76, 0x7a, 0x21, 0x2f, 0x75, 0x7b, 0x31, 0x3f, 0x63, 0x6d, 0x52, 0x5e,
         0x00, 0x74, 0x7c, 0x41, 0x4f, 0x10, 0x20, 0x62, 0x6e, 0x30, 0x73, 0x7d, 0x51, 0x5f, 0x40, 0x72, 0x7e, 0x61, 0x6f, 0x50, 0x71, 0x7f, 0x60, 0x70]
LENGTH_ORDER = [17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]


def ceil_shift(v, bits):
    return (v + (1 << bits) - 1) >> bits


def index_bits(colours):
    return 0 if colours > 16 else 1 if colours > 4 else 2 if colours > 2 else 3


def plane_distance(code, xs):
    """the distance a distance code (1 ..) stands for in an image xs wide"""
    if code > 120:
        return code - 120
    e = SHORT[code - 1]
    return max(1, (e >> 4) * xs + 8 - (e & 15))


# ------------------------------------------------------------------------------------------------------------------ bits
class Bits:
    """least significant bit of each byte first"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):
        assert 0 <= value < (1 << nbits) or nbits == 0 and value == 0, (value, nbits)
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c):
        """a prefix code word (value, length): most significant bit first"""
        value, length = c
        for k in range(length - 1, -1, -1):
            self.put((value >> k) & 1, 1)

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc & 255]) if self.n else b"")


# ----------------------------------------------------------------------------------------------------------- prefix codes
def huffman_lengths(hist, limit):
    """code lengths (0 for unused symbols) of a Huffman code over hist, at most `limit` long: counts are halved until it fits"""
    hist = [int(c) for c in hist]
    used = [s for s, c in enumerate(hist) if c]
    lengths = [0] * len(hist)
    if len(used) == 1:
        lengths[used[0]] = 1
        return lengths
    shift = 0
    while True:
        heap = [(max(1, hist[s] >> shift), s, (s,)) for s in used]
        heapq.heapify(heap)
        depth = {s: 0 for s in used}
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for s in a[2] + b[2]:
                depth[s] += 1
            heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
        if max(depth.values()) <= limit:
            for s in used:
                lengths[s] = depth[s]
            return lengths
        shift += 1


def skewed_lengths(hist):
    """1, 2, .., n-1, n-1 by falling count: the longest codes n symbols can have (15 bits at n = 16)"""
    used = sorted((s for s, c in enumerate(hist) if c), key=lambda s: -hist[s])
    assert 2 <= len(used) <= 16
    lengths = [0] * len(hist)
    for k, s in enumerate(used):
        lengths[s] = min(k + 1, len(used) - 1)
    return lengths


def canonical(lengths):
    """{symbol: (value, length)}"""
    code, words = 0, {}
    for n in range(1, 16):
        for s, l in enumerate(lengths):
            if l == n:
                words[s] = (code, n)
                code += 1
        code <<= 1
    return words


def put_normal_code(bw, lengths, repeats=True, max_symbol=False):
    """the normal form: a code-length code in the fixed order, then the lengths, with 16 / 17 / 18 repeats when `repeats`"""
    tokens, i, prev = [], 0, 8  # (code-length symbol, extra value, extra bits)
    n = len(lengths)
    while i < n:
        v = lengths[i]
        run = 1
        while i + run < n and lengths[i + run] == v:
            run += 1
        if repeats and v == 0 and run >= 3:
            take = min(run, 138)
            tokens.append((17, take - 3, 3) if take <= 10 else (18, take - 11, 7))
            i += take
        elif repeats and v != 0 and v == prev and run >= 3:
            take = min(run, 6)
            tokens.append((16, take - 3, 2))
            i += take
        else:
            tokens.append((v, 0, 0))
            if v:
                prev = v
            i += 1
    if max_symbol:
        while len(tokens) > 2 and tokens[-1][0] in (0, 17, 18):
            tokens.pop()
    hist = [0] * 19
    for t in tokens:
        hist[t[0]] += 1
    cl = huffman_lengths(hist, 7)
    words = canonical(cl)
    single = sum(1 for c in cl if c) == 1
    ncodes = max(4, 1 + max(k for k in range(19) if cl[LENGTH_ORDER[k]]))
    bw.put(0, 1)
    bw.put(ncodes - 4, 4)
    for k in range(ncodes):
        bw.put(cl[LENGTH_ORDER[k]], 3)
    if max_symbol:
        nbits = 2
        while len(tokens) - 2 >= (1 << nbits):
            nbits += 2
        bw.put(1, 1)
        bw.put((nbits - 2) // 2, 3)
        bw.put(len(tokens) - 2, nbits)
    else:
        bw.put(0, 1)
    for sym, extra, nbits in tokens:
        if not single:
            bw.code(words[sym])
        bw.put(extra, nbits)


def put_code(bw, hist, form="auto", repeats=True, max_symbol=False, skew=False):
    """writes a prefix code for the symbols hist counts and returns {symbol: (value, length)}; a code of one symbol has
    zero-length words.  form: "auto" (simple where the format allows it), "normal", "simple1bit" (a single symbol 0 / 1 in the
    one-bit field)"""
    used = [s for s, c in enumerate(hist) if c]
    if not used:  # a code no pixel uses still has to be a code
        bw.put(1, 1); bw.put(0, 1); bw.put(0, 1); bw.put(0, 1)
        return {}
    if form != "normal" and len(used) <= 2 and used[-1] < 256:
        bw.put(1, 1)
        bw.put(len(used) - 1, 1)
        if used[0] < 2:
            bw.put(0, 1); bw.put(used[0], 1)
        else:
            bw.put(1, 1); bw.put(used[0], 8)
        if len(used) == 2:
            bw.put(used[1], 8)
            return {used[0]: (0, 1), used[1]: (1, 1)}
        return {used[0]: (0, 0)}
    lengths = skewed_lengths(hist) if skew and 2 <= len(used) <= 16 else huffman_lengths(hist, 15)
    put_normal_code(bw, lengths, repeats, max_symbol)
    if len(used) == 1:
        return {used[0]: (0, 0)}
    return canonical(lengths)


def prefix_symbol(v):
    """a length or distance code v >= 1 -> (symbol, extra value, extra bits)"""
    if v <= 4:
        return v - 1, 0, 0
    d = v - 1
    extra = d.bit_length() - 2
    return 2 * extra + 2 + ((d >> extra) & 1), d & ((1 << extra) - 1), extra


# ------------------------------------------------------------------------------------------------- entropy-coded images
def tokenize(px, xs, cache_bits=0, lz=None, rs=None, used_codes=None):
    """pixels -> (0, argb) literals, (1, length, distance code) copies, (2, key) cache hits.
    lz: dict(codes=[distance codes tried in turn], prob=chance of trying at a pixel, maxlen=..); a copy is taken wherever the
    next code in turn gives a match of at least one pixel (copies overlap and cross row ends as they come)"""
    px = [int(v) for v in px]
    n = len(px)
    cache = [0] * (1 << cache_bits) if cache_bits else None
    key = lambda v: ((v * 0x1e35a7bd) & 0xFFFFFFFF) >> (32 - cache_bits)
    tokens, pos, turn = [], 0, 0
    while pos < n:
        if lz and pos and rs.rand() < lz.get("prob", 0.5):
            codes = lz["codes"]
            for attempt in range(8):
                code = codes[turn % len(codes)]
                dist = plane_distance(code, xs)
                if dist <= pos:
                    length = 0
                    top = min(lz.get("maxlen", 4096), n - pos)
                    while length < top and px[pos + length] == px[pos - dist + length]:
                        length += 1
                    if length:
                        break
                turn += 1
            else:
                length = 0
            if length:
                turn += 1
                if used_codes is not None:
                    used_codes.add(code)
                tokens.append((1, length, code))
                if cache:
                    for v in px[pos:pos + length]:
                        cache[key(v)] = v
                pos += length
                continue
        v = px[pos]
        if cache and cache[key(v)] == v and (rs is None or rs.rand() < 0.8):
            tokens.append((2, key(v)))
        else:
            tokens.append((0, v))
        if cache:
            cache[key(v)] = v
        pos += 1
    return tokens


def put_image(bw, px, xs, ys, top=False, cache_bits=0, meta=None, lz=None, rs=None, code_opts=None, used_codes=None):
    """one entropy-coded image.  meta (main image only): (prefix bits, (mh, mw) array of group numbers).  code_opts: keyword
    arguments of put_code for every code of the image"""
    px = np.asarray(px, np.uint32).reshape(-1)
    assert len(px) == xs * ys
    code_opts = code_opts or {}
    tokens = tokenize(px, xs, cache_bits, lz, rs, used_codes)
    bw.put(1 if cache_bits else 0, 1)
    if cache_bits:
        bw.put(cache_bits, 4)
    ngroups = 1
    if top:
        bw.put(1 if meta else 0, 1)
        if meta:
            mbits, groups = meta
            groups = np.asarray(groups)
            assert groups.shape == (ceil_shift(ys, mbits), ceil_shift(xs, mbits))
            bw.put(mbits - 2, 3)
            put_image(bw, (groups.astype(np.uint32) << 8).reshape(-1), groups.shape[1], groups.shape[0], rs=rs)
            ngroups = int(groups.max()) + 1
    green = 256 + 24 + ((1 << cache_bits) if cache_bits else 0)
    hists = [[[0] * a for a in (green, 256, 256, 256, 40)] for _ in range(ngroups)]

    def group_at(pos):
        return int(meta[1][(pos // xs) >> meta[0], (pos % xs) >> meta[0]]) if top and meta else 0

    pos = 0
    for t in tokens:
        h = hists[group_at(pos)]
        if t[0] == 0:
            v = t[1]
            h[0][(v >> 8) & 255] += 1; h[1][(v >> 16) & 255] += 1; h[2][v & 255] += 1; h[3][v >> 24] += 1
            pos += 1
        elif t[0] == 1:
            h[0][256 + prefix_symbol(t[1])[0]] += 1
            h[4][prefix_symbol(t[2])[0]] += 1
            pos += t[1]
        else:
            h[0][280 + t[1]] += 1
            pos += 1
    words = [[put_code(bw, h, **code_opts) for h in hg] for hg in hists]
    pos = 0
    for t in tokens:
        w = words[group_at(pos)]
        if t[0] == 0:
            v = t[1]
            bw.code(w[0][(v >> 8) & 255]); bw.code(w[1][(v >> 16) & 255]); bw.code(w[2][v & 255]); bw.code(w[3][v >> 24])
            pos += 1
        elif t[0] == 1:
            s, e, nb = prefix_symbol(t[1])
            bw.code(w[0][256 + s]); bw.put(e, nb)
            s, e, nb = prefix_symbol(t[2])
            bw.code(w[4][s]); bw.put(e, nb)
            pos += t[1]
        else:
            bw.code(w[0][280 + t[1]])
            pos += 1


# ---------------------------------------------------------------------------------------------------------------- files
def coded_width(width, transforms):
    for kind, bits, _ in transforms:
        if kind == COLOUR_INDEXING:
            width = ceil_shift(width, bits)
    return width


def put_header(bw, width, height, alpha=0, version=0):
    bw.put(0x2f, 8); bw.put(width - 1, 14); bw.put(height - 1, 14); bw.put(alpha, 1); bw.put(version, 3)


def put_transform(bw, kind, bits, data, w, height, rs=None, **image_opts):
    """one transform, its presence bit in front; w: the width it works on.  Returns the width behind it"""
    bw.put(1, 1); bw.put(kind, 2)
    if kind in (PREDICTOR, CROSS_COLOUR):
        bw.put(bits - 2, 3)
        put_image(bw, data, ceil_shift(w, bits), ceil_shift(height, bits), rs=rs, **image_opts)
    elif kind == COLOUR_INDEXING:
        pal = np.asarray(data, np.uint32).reshape(-1)
        bw.put(len(pal) - 1, 8)
        b = pal.view(np.uint8).reshape(-1, 4).astype(np.int64)
        delta = b.copy()
        delta[1:] = (b[1:] - b[:-1]) & 255
        put_image(bw, delta.astype(np.uint8).reshape(-1).view(np.uint32), len(pal), 1, rs=rs, **image_opts)
        w = ceil_shift(w, bits)
    return w


def write_vp8l(width, height, coded, transforms=(), alpha=0, version=0, rs=None, sub_opts=None, **image_opts):
    """the VP8L chunk's payload.  coded: (height, coded width) uint32; transforms: [(kind, bits, data)] in file order - data the
    (bh, bw) sub-image of a predictor (mode << 8) / cross-colour transform, the palette of colour indexing (its bits follow from
    its length), None for add-green.  image_opts go to the main image's put_image, sub_opts to the sub-images'"""
    bw = Bits()
    put_header(bw, width, height, alpha, version)
    w = width
    for kind, bits, data in transforms:
        w = put_transform(bw, kind, bits, data, w, height, rs=rs, **(sub_opts or {}))
    bw.put(0, 1)
    coded = np.asarray(coded, np.uint32)
    assert coded.shape == (height, w), (coded.shape, height, w)
    put_image(bw, coded, w, height, top=True, rs=rs, **image_opts)
    return bw.bytes()


def chunk(tag, body):
    return tag + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def riff(chunks):
    body = b"WEBP" + b"".join(chunks)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def vp8x(width, height, flags=0):
    return chunk(b"VP8X", bytes([flags, 0, 0, 0]) + struct.pack("<I", width - 1)[:3] + struct.pack("<I", height - 1)[:3])


def write_webp(width, height, coded, transforms=(), container="simple", **kw):
    """a file: "simple" = RIFF / WEBP / VP8L; "vp8x" = a VP8X container with ICCP, EXIF, XMP and unknown chunks around the
    image, one of them odd-sized"""
    image = chunk(b"VP8L", write_vp8l(width, height, coded, transforms, **kw))
    if container == "simple":
        return riff([image])
    return riff([vp8x(width, height, 0x20 | 0x08 | 0x04), chunk(b"ICCP", b"not a profile"), chunk(b"odd ", b"abc"), image,
                 chunk(b"EXIF", b"II*\0\x08\0\0\0\0\0"), chunk(b"XMP ", b"<x/>")])


# ------------------------------------------------------------------------------------------------- the inverse transforms
def _bytes(a):
    """(..) uint32 -> (.., 4) int64, bytes B, G, R, A"""
    return np.ascontiguousarray(a, np.uint32).view(np.uint8).reshape(a.shape + (4,)).astype(np.int64)


def _dwords(b):
    return np.ascontiguousarray(b & 255, np.int64).astype(np.uint8).view(np.uint32).reshape(b.shape[:-1])


def _avg(a, b):
    return (a + b) >> 1


def predict(mode, L, T, TL, TR):
    """the prediction of one mode from neighbours as (n, 4) byte arrays"""
    if mode == 1:
        return L
    if mode == 2:
        return T
    if mode == 3:
        return TR
    if mode == 4:
        return TL
    if mode == 5:
        return _avg(_avg(L, TR), T)
    if mode == 6:
        return _avg(L, TL)
    if mode == 7:
        return _avg(L, T)
    if mode == 8:
        return _avg(TL, T)
    if mode == 9:
        return _avg(T, TR)
    if mode == 10:
        return _avg(_avg(L, TL), _avg(T, TR))
    if mode == 11:  # Select: the Manhattan distance of L + T - TL to L is |T - TL|, to T |L - TL|; T on a tie
        to_l, to_t = np.abs(T - TL).sum(-1, keepdims=True), np.abs(L - TL).sum(-1, keepdims=True)
        return np.where(to_t <= to_l, T, L)
    if mode == 12:
        return np.clip(L + T - TL, 0, 255)
    if mode == 13:
        a = _avg(L, T)
        d = a - TL
        return np.clip(a + np.where(d < 0, -((-d) // 2), d // 2), 0, 255)  # C's division: towards zero
    black = np.zeros_like(L)  # 0, 14, 15
    black[..., 3] = 255
    return black


def block_map(sub, bits, h, w):
    """the (h, w) map of a (bh, bw) sub-image's values"""
    sub = np.asarray(sub)
    return sub[(np.arange(h) >> bits)[:, None], (np.arange(w) >> bits)[None, :]]


def pixel_modes(sub, bits, h, w):
    """the mode every pixel is predicted with: black at (0, 0), L along the top row, T down the left column, the block's elsewhere"""
    m = ((block_map(sub, bits, h, w) >> 8) & 15).astype(np.int64)
    m[0, :] = 1
    m[:, 0] = 2
    m[0, 0] = 0
    return m


def neighbours(P, ys, xs, w, tr="rule"):
    """L, T, TL, TR of pixels (ys, xs) of the byte image P; TR of the last column is the row's own pixel 0.
    tr: "zero" and "past" are two WRONG readings of that rule, which the tests tell apart from the right one: 0, and what a
    reader that steps one past the row above's end and is clamped there gets - the row above's LAST pixel"""
    xl, yu = np.maximum(xs - 1, 0), np.maximum(ys - 1, 0)
    last = xs + 1 >= w
    TR = np.where(last[:, None], P[ys, 0], P[yu, np.minimum(xs + 1, w - 1)])
    if tr == "zero":
        TR = np.where(last[:, None], 0, TR)
    elif tr == "past":
        TR = np.where(last[:, None], P[yu, w - 1], TR)
    return P[ys, xl], P[yu, xs], P[yu, xl], TR


def undo_predictor(res, sub, bits, tr="rule"):
    """(h, w) uint32 residuals -> pixels.  Pixel (x, y) needs (x + 1, y - 1): all pixels with x + 2 y = t are independent, so
    the image is walked by t with every row's pixel of that t done at once"""
    h, w = res.shape
    R, P = _bytes(res), np.zeros((h, w, 4), np.int64)
    modes = pixel_modes(sub, bits, h, w)
    for t in range(w + 2 * (h - 1)):
        ys = np.arange(max(0, (t - w + 2) // 2), min(h - 1, t // 2) + 1)
        xs = t - 2 * ys
        ys, xs = ys[(xs >= 0) & (xs < w)], xs[(xs >= 0) & (xs < w)]
        nb = neighbours(P, ys, xs, w, tr)
        m = modes[ys, xs]
        pred = np.zeros((len(ys), 4), np.int64)
        for mode in np.unique(m):
            pred[m == mode] = predict(int(mode), *[a[m == mode] for a in nb])
        P[ys, xs] = (R[ys, xs] + pred) & 255
    return _dwords(P)


def undo_cross_colour(px, sub, bits):
    h, w = px.shape
    b, m = _bytes(px), _bytes(block_map(sub, bits, h, w))
    s8 = lambda v: np.where(v >= 128, v - 256, v)
    green = s8(b[..., 1])
    red = (b[..., 2] + ((s8(m[..., 0]) * green) >> 5)) & 255
    blue = (b[..., 0] + ((s8(m[..., 1]) * green) >> 5) + ((s8(m[..., 2]) * s8(red)) >> 5)) & 255
    b[..., 2], b[..., 0] = red, blue
    return _dwords(b)


def add_green(px):
    b = _bytes(px)
    b[..., 2] += b[..., 1]
    b[..., 0] += b[..., 1]
    return _dwords(b)


def undo_indexing(px, palette, bits, width):
    """(h, coded w) -> (h, width): the green byte holds 2^bits indices, lowest bits first; beyond the palette: transparent black"""
    pal = np.zeros(256, np.uint32)
    pal[:len(palette)] = np.asarray(palette, np.uint32)
    each = 8 >> bits
    x = np.arange(width)
    packed = (px[:, x >> bits] >> 8) & 255
    return pal[(packed >> ((x & ((1 << bits) - 1)) * each).astype(np.uint32)) & ((1 << each) - 1)]


def convert(width, height, coded, transforms, tr="rule"):
    """the (height, width, 3) BGR image of coded data: the inverse transforms, last in the file first, alpha dropped"""
    px = np.asarray(coded, np.uint32)
    widths, w = [], width
    for kind, bits, _ in transforms:
        widths.append(w)
        if kind == COLOUR_INDEXING:
            w = ceil_shift(w, bits)
    assert px.shape == (height, w)
    for (kind, bits, data), w_at in zip(reversed(list(transforms)), reversed(widths)):
        if kind == PREDICTOR:
            px = undo_predictor(px, data, bits, tr)
        elif kind == CROSS_COLOUR:
            px = undo_cross_colour(px, data, bits)
        elif kind == ADD_GREEN:
            px = add_green(px)
        else:
            px = undo_indexing(px, data, bits, w_at)
    return np.ascontiguousarray(_bytes(px)[..., :3]).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------ forwards, for images
def encode(bgr, rs, predictor_bits=4, cross_bits=5, modes=None, **kw):
    """a BGR image as a file with subtract-green, cross-colour (random small multipliers) and a predictor (random modes, or
    `modes`, a (bh, bw) array) - the three transforms libwebp's encoder uses on photographs, applied forwards here.
    Returns (file, (coded, transforms))"""
    h, w = bgr.shape[:2]
    b = np.concatenate([bgr.astype(np.int64), np.full((h, w, 1), 255, np.int64)], 2)
    b[..., 2] -= b[..., 1]
    b[..., 0] -= b[..., 1]
    b &= 255
    cross = rs.randint(0, 256, (ceil_shift(h, cross_bits), ceil_shift(w, cross_bits), 4)).astype(np.uint8)
    cross[..., 3] = 255
    cross = cross.view(np.uint32)[..., 0]
    m = _bytes(block_map(cross, cross_bits, h, w))
    s8 = lambda v: np.where(v >= 128, v - 256, v)
    green, red = s8(b[..., 1]), b[..., 2].copy()
    b[..., 2] = (red - ((s8(m[..., 0]) * green) >> 5)) & 255
    b[..., 0] = (b[..., 0] - ((s8(m[..., 1]) * green) >> 5) - ((s8(m[..., 2]) * s8(red)) >> 5)) & 255
    if modes is None:
        modes = rs.randint(0, 14, (ceil_shift(h, predictor_bits), ceil_shift(w, predictor_bits)))
    sub = (np.asarray(modes).astype(np.uint32) << 8) | np.uint32(BLACK)
    ys, xs = [a.reshape(-1) for a in np.mgrid[0:h, 0:w]]
    nb = neighbours(b, ys, xs, w)
    pm = pixel_modes(sub, predictor_bits, h, w).reshape(-1)
    pred = np.zeros((h * w, 4), np.int64)
    for mode in np.unique(pm):
        pred[pm == mode] = predict(int(mode), *[a[pm == mode] for a in nb])
    coded = _dwords((b.reshape(-1, 4) - pred) & 255).reshape(h, w)
    transforms = [(ADD_GREEN, 0, None), (CROSS_COLOUR, cross_bits, cross), (PREDICTOR, predictor_bits, sub)]
    return write_webp(w, h, coded, transforms, rs=rs, **kw), (coded, transforms)


# ------------------------------------------------------------------------------------------------------------ test cases
def random_transform(rs, kind, w, h, bits=None, colours=None, modes=None):
    """(kind, bits, data) with random data for an image (at this point of the file) w wide"""
    if kind == PREDICTOR:
        bits = bits or int(rs.randint(2, 10))
        shape = (ceil_shift(h, bits), ceil_shift(w, bits))
        m = rs.randint(0, 16, shape) if modes is None else np.broadcast_to(np.asarray(modes), shape)
        noise = rs.randint(0, 256, shape + (4,)).astype(np.uint8).view(np.uint32)[..., 0] & np.uint32(0xFFFF00FF)  # only bits 8 .. 11 count
        return kind, bits, noise | (m.astype(np.uint32) << 8) | (rs.randint(0, 16, shape).astype(np.uint32) << 12)
    if kind == CROSS_COLOUR:
        bits = bits or int(rs.randint(2, 10))
        shape = (ceil_shift(h, bits), ceil_shift(w, bits))
        return kind, bits, rs.randint(0, 256, shape + (4,)).astype(np.uint8).view(np.uint32)[..., 0]
    if kind == ADD_GREEN:
        return kind, 0, None
    colours = colours or int(rs.randint(1, 257))
    return kind, index_bits(colours), rs.randint(0, 256, (colours, 4)).astype(np.uint8).view(np.uint32)[:, 0]


def random_case(rs, width, height, kinds, values=None, beyond=False, **kw):
    """coded data and transforms (file order `kinds`) for a width x height image.  values: how many different coded pixels
    there are (few: back references and cache hits abound; None: noise).  beyond: palette indices run past the palette"""
    transforms, w = [], width
    for kind in kinds:
        opts = {k: v for k, v in kw.items() if k in ("bits", "modes")} if kind in (PREDICTOR, CROSS_COLOUR) else {"colours": kw.get("colours")} if kind == COLOUR_INDEXING else {}
        t = random_transform(rs, kind, w, height, **opts)
        transforms.append(t)
        if kind == COLOUR_INDEXING:
            w = ceil_shift(w, t[1])
    if values:
        table = rs.randint(0, 256, (values, 4)).astype(np.uint8).view(np.uint32)[:, 0]
        coded = table[rs.randint(0, values, (height, w))]
    else:
        coded = rs.randint(0, 256, (height, w, 4)).astype(np.uint8).view(np.uint32)[..., 0]
    pal = [t for t in transforms if t[0] == COLOUR_INDEXING]
    if pal and not beyond and pal[0][1] == 0:
        # one index a pixel: keep them inside the palette (bundled indices are any bit pattern: 3, 5 .. colours leave some beyond)
        g = rs.randint(0, len(pal[0][2]), (height, w)).astype(np.uint32)
        coded = (coded & np.uint32(0xFFFF00FF)) | (g << 8)
    return coded, transforms
