"""zlib streams for the tests of the Deflate route (host: tiff::detail::inflate of host/tiff_decode.h, which is zlib; device:
csrc/kernels_inflate.hip, whose walk csrc/inflate_core.h also runs on the CPU in host/inflate_check.cpp): an LSB-first bit
writer and block builders for hand-built streams, Python's zlib with its levels and strategies for whole ones, the seeded
mutations of the refusal corpus, the stream-file form of `tiff_check --inflate` / `inflate_check`, and the coded frame that
carries one stream per chunk."""
import os
import struct
import subprocess
import zlib

import numpy as np

import tiff_writer as tw

ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


class Bits:
    """bits as Deflate packs them: fields from the least significant bit of each byte on, Huffman codes most significant bit first"""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, bits):
        self.acc |= (value & ((1 << bits) - 1)) << self.n
        self.n += bits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8
        return self

    def code(self, code, bits):
        for k in range(bits - 1, -1, -1):
            self.put((code >> k) & 1, 1)
        return self

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)
        return self

    def raw(self, data):
        assert self.n == 0
        self.out += data
        return self

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def header(cinfo=7, cm=8, fdict=0, fcheck_off=0):
    cmf = (cinfo << 4) | cm
    flg = (2 << 6) | (fdict << 5)
    flg += (31 - ((cmf << 8) + flg) % 31) % 31
    return bytes([cmf, (flg + fcheck_off) & 255])


def wrap(body, data=None, hdr=None, adler=None):
    """header + body + Adler-32 of `data` (none where data is None)"""
    tail = b"" if data is None and adler is None else struct.pack(">I", zlib.adler32(data) if adler is None else adler)
    return (header() if hdr is None else hdr) + body + tail


def canonical(lens):
    """{symbol: (code, length)} of a list of code lengths"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


FIXED_LIT = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = canonical([5] * 32)
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def length_symbol(n, by_284=False):
    if n == 258 and by_284:
        return 284, 5, 31
    k = max(i for i in range(29) if LEN_BASE[i] <= n)
    return 257 + k, LEN_EXTRA[k], n - LEN_BASE[k]


def distance_symbol(d):
    k = max(i for i in range(30) if DIST_BASE[i] <= d)
    return k, DIST_EXTRA[k], d - DIST_BASE[k]


def symbols(b, ops, lit=FIXED_LIT, dist=FIXED_DIST):
    """ops: bytes (literals), ("m", length, distance[, by_284]), ("l", symbol) a bare literal/length symbol, ("d", symbol) a bare
    distance symbol, ("e",) the end-of-block code"""
    for op in ops:
        if isinstance(op, (bytes, bytearray)):
            for v in op:
                b.code(*lit[v])
        elif op[0] == "m":
            s, xb, xv = length_symbol(op[1], len(op) > 3 and op[3])
            b.code(*lit[s]).put(xv, xb)
            s, xb, xv = distance_symbol(op[2])
            b.code(*dist[s]).put(xv, xb)
        elif op[0] == "l":
            b.code(*lit[op[1]])
        elif op[0] == "d":
            b.code(*dist[op[1]])
        else:
            b.code(*lit[256])
    return b


def fixed(b, ops, final=1, end=True):
    b.put(final, 1).put(1, 2)
    return symbols(b, list(ops) + ([("e",)] if end else []))


def stored(b, data, final=1, nlen=None):
    b.put(final, 1).put(0, 2).align()
    b.put(len(data), 16).put((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
    return b.raw(data)


def run_tokens(lens):
    """the greedy run-length tokens of a list of code lengths: (symbol, extra value)"""
    out, i = [], 0
    while i < len(lens):
        v, j = lens[i], i
        while j < len(lens) and lens[j] == v:
            j += 1
        n = j - i
        if v == 0 and n >= 3:
            n = min(n, 138)
            out.append((17, n - 3) if n <= 10 else (18, n - 11))
        elif v and n >= 4:
            n = min(n - 1, 6)
            out += [(v, 0), (16, n - 3)]
            n += 1
        else:
            n = 1
            out.append((v, 0))
        i += n
    return out


CL_ALL = [4] * 13 + [5] * 6  # a complete code-length code over all 19 symbols


def dynamic(b, lit_lens, dist_lens, ops, final=1, end=True, tokens=None, cl_lens=None, hclen=None, hlit=None, hdist=None):
    """a dynamic block: the two sets of lengths (lists, at least 257 and 1 long), sent by `tokens` (default: their greedy runs)
    under the code-length code `cl_lens` (19 lengths by symbol; default: complete over the symbols the tokens use where that is
    8 symbols of 3 bits, else CL_ALL), HCLEN / HLIT / HDIST fields as given or as the lists say"""
    if tokens is None:
        tokens = run_tokens(list(lit_lens) + list(dist_lens))
    if cl_lens is None:
        cl_lens = CL_ALL
    cl = canonical(cl_lens)
    if hclen is None:
        hclen = max([4] + [ORDER.index(s) + 1 for s in range(19) if cl_lens[s]])
    b.put(final, 1).put(2, 2)
    b.put(len(lit_lens) - 257 if hlit is None else hlit, 5).put(len(dist_lens) - 1 if hdist is None else hdist, 5).put(hclen - 4, 4)
    for k in range(hclen):
        b.put(cl_lens[ORDER[k]], 3)
    for s, x in tokens:
        b.code(*cl[s])
        if s >= 16:
            b.put(x, {16: 2, 17: 3, 18: 7}[s])
    lit = canonical(lit_lens)
    dist = canonical(dist_lens)
    return symbols(b, list(ops) + ([("e",)] if end and 256 in lit else []), lit, dist)


def lens_of(n, **by_symbol):
    out = [0] * n
    for k, v in by_symbol.items():
        out[int(k[1:])] = v
    return out


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, 8, 15, 8, strategy)
    return c.compress(data) + c.flush()


TEXT = b"the quick brown fox jumps over the lazy dog. Pack my box with five dozen liquor jugs! "


def hand_built():
    """[(name, need, stream)]: the list of the issue, block by block"""
    rs = np.random.RandomState(31)
    rnd = lambda n: rs.randint(0, 256, n).astype(np.uint8).tobytes()  # noqa: E731
    out = []

    def add(name, b, data=None, need=None, **kw):
        body = b.bytes() if isinstance(b, Bits) else b
        out.append((name, len(data) if need is None else need, wrap(body, data, **kw)))

    # ---- stored blocks
    add("stored LEN 0 then LEN 3", stored(stored(Bits(), b"", 0), b"abc"), b"abc")
    add("stored LEN 0 alone", stored(Bits(), b""), b"", need=1)
    add("stored LEN 1", stored(Bits(), b"z"), b"z")
    big = rnd(65535)
    add("stored LEN 65535", stored(Bits(), big), big)
    three = [rnd(70), rnd(1), rnd(300)]
    add("three stored blocks", stored(stored(stored(Bits(), three[0], 0), three[1], 0), three[2]), b"".join(three))
    add("stored behind a fixed block that ends off a byte boundary", stored(fixed(Bits(), [b"ab"], 0), b"cdefg"), b"abcdefg")
    add("stored NLEN mismatch", stored(Bits(), b"abc", nlen=0x1234), b"abc")
    add("stored block cut by the input", stored(Bits(), rnd(100)).bytes()[:60], None, need=100)
    # ---- fixed Huffman
    for n in (1, 2, 3, 4, 5, 6, 63, 64, 65, 127, 128, 129, 299, 300):
        data = rnd(n)
        add("fixed literals %d" % n, fixed(Bits(), [data]), data)
    for n, by_284 in ((3, 0), (10, 0), (11, 0), (257, 0), (258, 0), (258, 1)):
        data = (b"abc" * 100)[:3 + n]
        add("fixed match %d%s" % (n, " by 284 + 31" if by_284 else ""), fixed(Bits(), [b"abc", ("m", n, 3, by_284)]), data)
    for d in (1, 2, 3, 63, 64, 65):
        for n in (63, 64, 65, 127, 128, 129, 258):
            head = rnd(d + 2)
            data = bytearray(head)
            for k in range(n):
                data.append(data[len(data) - d])
            add("fixed match %d at distance %d" % (n, d), fixed(Bits(), [head, ("m", n, d)]), bytes(data))
    add("distance == o", fixed(Bits(), [b"hello", ("m", 5, 5)]), b"hellohello")
    add("distance == o + 1", fixed(Bits(), [b"hello", ("m", 5, 6)]), None, need=10)
    far = rnd(32768)
    add("distance 32768 in 33000 bytes", fixed(stored(Bits(), far, 0), [("m", 232, 32768)]), far + far[:232])
    add("distance 32768 one byte early", fixed(stored(Bits(), far[:32767], 0), [("m", 232, 32768)]), None, need=32999)
    for s in (286, 287):
        add("length code %d" % s, fixed(Bits(), [b"abc", ("l", s), ("d", 0)]), None, need=6)
    for s in (30, 31):
        add("distance code %d" % s, fixed(Bits(), [b"abc", ("l", 257), ("d", s)]), None, need=6)
    # ---- dynamic blocks
    # a b c at 2 bits, the end-of-block code at 3, lengths 3, 7, 13-14, 19-22, 27-30, 35-42, 227-257 and 258 at 6: complete
    abc = lens_of(286, s97=2, s98=2, s99=2, s256=3, s257=6, s261=6, s266=6, s269=6, s271=6, s273=6, s284=6, s285=6)
    one_d = [1]
    add("HCLEN 19", dynamic(Bits(), abc, [1, 1], [b"abcabc", ("m", 7, 2)]), b"abcabc" + b"bcbcbcb")
    # HCLEN 4: 16, 17, 18 and 0 alone have codes, so every length is 0 and there is no end-of-block code
    add("HCLEN 4", dynamic(Bits(), [0] * 257, [0], [], cl_lens=lens_of(19, s18=1, s0=1), tokens=[(18, 127), (18, 98)], hclen=4), None, need=1)
    # 18 x 138 and x 11, 17 x 10 and x 3, 16 x 3 and x 6, a zero run from the literal lengths into the distance lengths
    lit = [0] * 162 + [2] + [4] * 4 + [5] * 7 + [0] * 82 + [3, 4, 4, 5] + [0] * 26
    dst = [0] * 10 + [1, 1] + [0] * 18
    tokens = [(18, 127), (18, 0), (17, 7), (17, 0), (2, 0), (4, 0), (16, 0), (5, 0), (16, 3), (18, 71), (3, 0), (4, 0), (4, 0), (5, 0), (18, 25), (1, 0), (1, 0), (18, 7)]
    cl8 = lens_of(19, s1=3, s2=3, s3=3, s4=3, s5=3, s16=3, s17=3, s18=3)
    body = bytes(range(162, 174)) * 4
    add("runs of 16 / 17 / 18 at their shortest and longest, one across the two sets",
        dynamic(Bits(), lit, dst, [body, ("m", 3, 40), ("m", 4, 48), ("m", 5, 33)], tokens=tokens, cl_lens=cl8), body + body[8:11] + body[3:7] + body[22:27])
    add("16 as the first symbol", dynamic(Bits(), lit, dst, [body], tokens=[(16, 0)] + tokens[1:], cl_lens=cl8), None, need=len(body))
    add("a run past the end", dynamic(Bits(), lit, dst, [body], tokens=tokens[:-1] + [(18, 8)], cl_lens=cl8), None, need=len(body))
    deep = list(range(1, 14)) + [15] + [0] * 242 + [15] + [0] * 29  # 13, 256, 263 (length 9) and 273 (35 .. 42) at 15 bits
    deep[263] = deep[273] = 15
    ddeep = list(range(1, 16)) + [15]
    data = bytes([13, 12, 0, 11, 13, 1, 2, 3]) * 30
    tail = bytearray(data)
    ops = [data]
    for n, d in ((9, 150), (36, 200), (9, 129), (42, 192), (35, 1)):
        ops.append(("m", n, d))
        for k in range(n):
            tail.append(tail[len(tail) - d])
    add("code lengths of 15 in both sets", dynamic(Bits(), deep, ddeep, ops), bytes(tail))
    add("one distance code of length 1", dynamic(Bits(), abc, one_d, [b"abc", ("m", 20, 1)]), b"abc" + b"c" * 20)
    add("one distance code, the other bit", dynamic(Bits(), lens_of(258, s97=2, s98=2, s256=2, s257=2), one_d, [b"ab", ("l", 257)], end=False).put(1, 1).put(0, 7), None, need=5)
    add("no distance code, literals only", dynamic(Bits(), abc, [0], [b"abccba" * 9]), b"abccba" * 9)
    add("no distance code and a match", dynamic(Bits(), lens_of(258, s97=2, s98=2, s256=2, s257=2), [0], [b"ab", ("l", 257)], end=False).put(0, 8), None, need=5)
    add("an over-subscribed literal set", dynamic(Bits(), lens_of(257, s97=1, s98=1, s256=1), [1, 1], []), None, need=1)
    add("an over-subscribed distance set", dynamic(Bits(), abc, [1, 1, 1], []), None, need=1)
    add("an incomplete literal set", dynamic(Bits(), lens_of(257, s97=2, s256=2), [1, 1], []), None, need=1)
    add("an incomplete distance set", dynamic(Bits(), abc, [2, 2], []), None, need=1)
    add("an incomplete code-length code", dynamic(Bits(), abc, [1, 1], [], cl_lens=lens_of(19, s0=2, s2=2, s18=2), tokens=[(0, 0)] * 40), None, need=1)
    add("no end-of-block code", dynamic(Bits(), lens_of(257, s97=1, s98=1), [1, 1], [b"abab"], end=False), None, need=4)
    add("HLIT 287", dynamic(Bits(), abc, [1, 1], [b"abc"], hlit=30), None, need=3)
    add("HDIST 31", dynamic(Bits(), abc, [1, 1], [b"abc"], hdist=30), None, need=3)
    add("HDIST 32", dynamic(Bits(), abc, [1, 1], [b"abc"], hdist=31), None, need=3)
    # ---- whole streams
    mixed = dynamic(stored(fixed(Bits(), [b"fixed ", ("m", 12, 6)], 0), b" stored ", 0), abc, [1, 1], [b"abcabc", ("m", 30, 2)])
    whole = b"fixed fixed fixed  stored abcabc" + b"bc" * 15
    add("fixed + stored + dynamic", mixed, whole)
    add("bytes behind the final block", mixed.bytes() + struct.pack(">I", zlib.adler32(whole)) + b"more bytes behind", None, need=len(whole))
    open_end = fixed(fixed(Bits(), [b"never "], 0), [b"final"], 0)
    add("no final block, the bytes are there", open_end, None, need=11)
    add("no final block, one byte short", open_end, None, need=12)
    text = (TEXT * 4)[:300]
    sound = deflate(text)
    for name, hdr in (("CM 7", header(cm=7)), ("CINFO 8", header(cinfo=8)), ("FCHECK", header(fcheck_off=1)), ("FDICT", header(fdict=1))):
        out.append(("header fault: " + name, 300, hdr + sound[2:]))
    out.append(("a header of one byte", 1, sound[:1]))
    out.append(("an empty stream", 1, b""))
    out.append(("a wrong Adler-32", 300, sound[:-4] + bytes(4)))
    out.append(("a cut trailer", 300, sound[:-3]))
    out.append(("no trailer", 300, sound[:-4]))
    lead = rnd(300)
    add("CINFO 0 with a distance of 300", fixed(stored(Bits(), lead, 0), [("m", 100, 300)]), lead + lead[:100], hdr=header(cinfo=0))
    # ---- need against the stream
    out.append(("a surplus behind need", 200, sound))
    for need in range(280, 300):
        add("the last match cut at %d, period 1" % need, fixed(Bits(), [b"a", ("m", 258, 1), ("m", 41, 1)]), b"a" * 300, need=need)
        add("the last match cut at %d, period 2" % need, fixed(Bits(), [b"ab", ("m", 258, 2), ("m", 40, 2)]), b"ab" * 150, need=need)
    out.append(("one byte short", 301, sound))
    for k in range(1, 13):
        out.append(("the input cut by %d" % k, 300, sound[:-k]))
    return out


def refill_streams():
    """[(name, need, stream)]: coded bytes several times the LDS window, symbols across its edge; every level and strategy"""
    rs = np.random.RandomState(32)
    out = []
    for n in (3000, 9000):
        data = rs.randint(0, 256, n).astype(np.uint8).tobytes()
        out.append(("random %d level 9" % n, n, deflate(data, 9)))
    n = 40000
    kinds = {"text": (TEXT * (n // len(TEXT) + 1))[:n], "zeros": bytes(n), "period 3": (b"xyz" * n)[:n], "random": rs.randint(0, 256, n).astype(np.uint8).tobytes()}
    for kind, data in kinds.items():
        for level in (0, 1, 6, 9):
            for strategy in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_RLE, zlib.Z_HUFFMAN_ONLY, zlib.Z_FILTERED):
                out.append(("%s level %d strategy %d" % (kind, level, strategy), n, deflate(data, level, strategy)))
    return out


def fuzz_corpus(seed=33, count=240):
    """[(name, need, stream)]: seeded mutations - single-bit flips, truncations, random bytes - of sound streams of 55 .. 311 bytes"""
    rs = np.random.RandomState(seed)
    bases = []
    while len(bases) < 24:
        n = int(rs.randint(60, 2000))
        kind = len(bases) % 4
        data = (rs.randint(0, 256, n) if kind == 0 else rs.randint(0, 4, n) if kind == 1 else np.repeat(rs.randint(0, 256, n // 7 + 1), 7)[:n]).astype(np.uint8).tobytes() if kind < 3 else (TEXT * 30)[:n]
        s = deflate(data, int(rs.choice([1, 6, 9])), int(rs.choice([0, 0, zlib.Z_FIXED, zlib.Z_RLE, zlib.Z_HUFFMAN_ONLY])))
        if 55 <= len(s) <= 311:
            bases.append((data, s))
    out = []
    for i in range(count):
        data, s = bases[rs.randint(len(bases))]
        s = bytearray(s)
        kind = i % 4
        if kind in (0, 1):
            s[rs.randint(len(s))] ^= 1 << rs.randint(8)
        elif kind == 2:
            del s[rs.randint(2, len(s)):]
        else:
            j, n = rs.randint(len(s)), rs.randint(1, 6)
            s[j:j + n] = rs.randint(0, 256, n).astype(np.uint8).tobytes()
        need = len(data) if rs.randint(4) else max(1, int(len(data) * rs.choice([0.5, 0.9])))
        out.append(("mutation %d of kind %d" % (i, kind), need, bytes(s)))
    return out


def stream_file(cases):
    """the form `tiff_check --inflate` and `inflate_check` read"""
    return b"".join(struct.pack("<II", need, len(s)) + s for _, need, s in cases)


def verdicts(exe, cases, directory, tag):
    """[(good, produced, bytes written: `need` of them, zeros behind)] per case, from a program of that form"""
    src, dst = os.path.join(str(directory), tag + ".streams"), os.path.join(str(directory), tag + ".out")
    with open(src, "wb") as f:
        f.write(stream_file(cases))
    r = subprocess.run([exe, src, dst] if os.path.basename(exe).startswith("inflate_check") else [exe, "--inflate", src, dst], capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-3000:])
    raw, pos, out = open(dst, "rb").read(), 0, []
    for _, need, _ in cases:
        good, produced = struct.unpack_from("<BI", raw, pos)
        out.append((bool(good), produced, raw[pos + 5:pos + 5 + need]))
        pos += 5 + need
    assert pos == len(raw)
    return out


def frame_of(cases, compression=tw.ADOBE_DEFLATE):
    """one coded frame, one stream per chunk (as tiff_coded.grey_strip): 8-bit grey, one pixel wide, a strip per stream whose
    `rows` is the stream's `need`, every strip as high as the longest"""
    high = max(need for _, need, _ in cases)
    chunks, pool = [], bytearray()
    for _, need, s in cases:
        chunks.append((len(pool), len(s), need))
        pool += s
    return dict(w=1, h=high * len(cases), photometric=tw.MINISBLACK, bits=8, samples=1, planar=1, predictor=1, big_endian=0, premultiply=0,
                tile=(1, high), palette=np.zeros((256, 4), np.uint8), compression=compression, chunks=chunks, data=bytes(pool))
