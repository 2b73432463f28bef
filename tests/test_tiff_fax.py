"""CCITT fax TIFF requests, host half (host/ccitt_decode.h through host/tiff_decode.h): Modified Huffman RLE (Compression 2,
32771), Group 3 in one and two dimensions (3) and Group 4 (4).  Every decode equals the bitmap that was encoded (by
tests/fax_writer.py, a pure-Python encoder with a code table of its own), TIFFReadRGBAImageOriented of the system's libtiff
through ctypes and - for the files Pillow writes - Pillow.  The decoder runs in host/tiff_check.cpp, a plain host program built
with -fsanitize=address,undefined; nothing of it is loaded into Python.  The device half is tests/test_gpu_tiff_fax.py.

Two differences from libtiff (4.3.0, and the 4.7.1 Pillow bundles) are deliberate; both are libtiff misreading clean files, and
test_libtiff_misreads_two_clean_forms pins the observations:
  - Compression 2: tif_fax3.c pads its bit accumulator with imaginary zeros when fewer than 13 bits are left in a chunk, and
    its byte alignment then counts them: rows within the last two bytes of a chunk come out white.  The libtiff comparison
    therefore stores the Modified Huffman chunks with two zero bytes behind them (which the decoder here must not mind)
  - Compression 32771: its word alignment is taken relative to how far it has read ahead, not to the chunk's start, and fails
    for most rows.  Those files are compared with the bitmap, and with the decode of the same bitmap in Compression 2"""
import ctypes
import io
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fax_writer as fx  # noqa: E402
import tiff_writer as tw  # noqa: E402
from test_tiff_decode import build_check, libtiff_bgr, load_libtiff  # noqa: E402

WIDTHS = [1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 257, 1728]
HEIGHTS = [1, 2, 5, 17]
LAYOUTS = [dict(rows_per_strip=1), dict(rows_per_strip=2), dict(rows_per_strip=16), dict(), dict(tile=(16, 16)), dict(tile=(32, 16))]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """host/tiff_check.cpp with AddressSanitizer and UBSan: a stand-alone host program"""
    return build_check(tmp_path_factory.mktemp("tifffax"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return r


def bitmap_of(rs, kind, h, w):
    if kind == 0:
        return (rs.rand(h, w) < 0.5).astype(int)
    if kind == 1:
        return np.repeat(rs.randint(0, 2, (h, w // 5 + 1)), 5, 1)[:, :w]
    base = np.repeat(rs.randint(0, 2, (1, w // 7 + 1)), 7, 1)[:, :w]
    return np.concatenate([np.roll(base, y % 4, 1) for y in range(h)], 0)  # text-like: rows that repeat, shifted a little


class Case:
    def __init__(self, name, bitmap, compression, photometric=0, **kw):
        self.name, self.bitmap, self.compression, self.photometric, self.kw = name, np.asarray(bitmap), compression, photometric, kw
        self.data = fx.write_fax(bitmap, compression, photometric=photometric, **kw)
        self.want = fx.wanted(bitmap, photometric)

    def padded(self):
        """the file with two zero bytes behind every chunk's stream (module docstring)"""
        kw = dict(self.kw)
        blocks, _ = fx.split(self.bitmap, kw.get("tile"), kw.get("rows_per_strip"))
        kw["streams"] = [fx.encode(b, self.compression) + b"\0\0" for b in blocks]
        return fx.write_fax(self.bitmap, self.compression, photometric=self.photometric, **kw)


def matrix(seed=4):
    """every coding x layout x fill order x photometric, the widths and heights walked through so that every coding meets every
    width and every height; then the branch bitmaps in every coding, K = 2 and 4, RTC / EOFB present and absent, fill bits
    that T4Options does not announce, both byte orders"""
    rs = np.random.RandomState(seed)
    cases, n = [], 0
    for ci, (cname, comp, ckw) in enumerate(fx.CODINGS):
        for li, layout in enumerate(LAYOUTS):
            for fill_order in (1, 2):
                for photometric in (0, 1):
                    w, h = WIDTHS[(n + ci) % len(WIDTHS)], HEIGHTS[(n // 2 + li) % len(HEIGHTS)]
                    bm = bitmap_of(rs, n % 3, h, w)
                    cases.append(Case("%s %dx%d %s fill=%d ph=%d" % (cname, w, h, layout, fill_order, photometric), bm, comp, photometric,
                                      fill_order=fill_order, big_endian=bool(n & 4), **ckw, **layout))
                    n += 1
        for w in WIDTHS:  # every width and height at least once per coding, as one strip
            cases.append(Case("%s %dx%d" % (cname, w, HEIGHTS[n % 4]), bitmap_of(rs, n % 3, HEIGHTS[n % 4], w), comp, **ckw))
            n += 1
        for bname, bm in fx.branch_bitmaps():
            cases.append(Case("%s %s" % (cname, bname), bm, comp, **ckw))
    bm = bitmap_of(rs, 2, 9, 65)
    for k in (2, 4):
        cases.append(Case("g3-2d K=%d" % k, bm, fx.G3, t4=1, k=k))
        cases.append(Case("g3-2d K=%d with fill bits" % k, bm, fx.G3, t4=5, k=k, fill=True))
    cases.append(Case("g3 without RTC", bm, fx.G3, end=False))
    cases.append(Case("g3-2d without RTC", bm, fx.G3, t4=1, end=False))
    cases.append(Case("g4 without EOFB", bm, fx.G4, end=False))
    cases.append(Case("g3 fill bits that T4Options does not announce", bm, fx.G3, t4=0, fill=True))
    cases.append(Case("g3 without a T4Options tag", bm, fx.G3, t4=None))
    return cases


@pytest.fixture(scope="module")
def decoded(checker, tmp_path_factory):
    """the matrix through ONE tiff_check --decode process (parse + pixels), and the files' paths"""
    cases = matrix()
    d = tmp_path_factory.mktemp("faxmatrix")
    args = []
    for i, c in enumerate(cases):
        p = os.path.join(str(d), "c%04d.tif" % i)
        open(p, "wb").write(c.data)
        args += [p, p + ".bgr"]
    r = run(checker, "--decode", *args)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = [np.fromfile(args[2 * i + 1], np.uint8).reshape(c.want.shape) for i, c in enumerate(cases)]
    return cases, got, args[0::2]


def test_code_table_is_a_prefix_code_with_the_eol_prefix_free():
    """the writer's table (the decoder's is written separately, in C++): no code word begins another of its colour, and together
    they leave exactly the words that begin with eight zeros - the EOL's"""
    for colour in (fx.WHITE, fx.BLACK):
        words = sorted(fx.CODES[colour].values())
        assert len(set(words)) == 64 + 27 + 13
        assert not any(b.startswith(a) for a, b in zip(words, words[1:]))
        assert sum(2 ** (13 - len(w)) for w in words) == 8192 - 32


def test_decoder_equals_the_bitmap(decoded):
    cases, got, _ = decoded
    assert len(cases) >= 6 * (len(LAYOUTS) * 4 + len(WIDTHS) + 20)
    for c, g in zip(cases, got):
        assert np.array_equal(g, c.want), (c.name, int((g != c.want).sum()))


def test_decoder_equals_libtiff(decoded, checker, tmp_path):
    """skipped only as a whole, when no libtiff loads.  Compression 2 with two zero bytes behind each chunk, 32771 against the
    Compression 2 decode of the same bitmap (module docstring); the decoder gives the same image with and without the bytes"""
    L = load_libtiff()
    if L is None:
        pytest.skip("no libtiff.so.* on this machine")
    cases, got, _ = decoded
    path = tmp_path / "x.tif"
    padded = []
    for c, g in zip(cases, got):
        if c.compression == fx.MHW:
            twin = Case(c.name, c.bitmap, fx.MH, c.photometric, **c.kw)
            padded.append(twin)
            continue
        data = c.data
        if c.compression == fx.MH:
            padded.append(c)
            data = c.padded()
        path.write_bytes(data)
        ref = libtiff_bgr(L, path, g.shape[1], g.shape[0])
        assert ref is not None, ("libtiff refuses a written file", c.name)
        assert np.array_equal(g, ref), (c.name, int((g != ref).sum()))
    args = []
    for i, c in enumerate(padded):
        p = str(tmp_path / ("p%04d.tif" % i))
        open(p, "wb").write(c.padded())
        args += [p, p + ".bgr"]
    assert run(checker, "--decode", *args).returncode == 0
    for i, c in enumerate(padded):
        assert np.array_equal(np.fromfile(args[2 * i + 1], np.uint8).reshape(c.want.shape), c.want), c.name


def test_decoder_equals_pillow_on_the_files_pillow_writes(checker, tmp_path):
    """Pillow's own libtiff writes the three kinds; the decoder reads them as Pillow and the system's libtiff do"""
    pytest.importorskip("PIL")
    from PIL import Image, features
    if not features.check("libtiff"):
        pytest.skip("this Pillow has no libtiff")
    L = load_libtiff()
    rs = np.random.RandomState(9)
    args, wants = [], []
    for i, (kind, w, h) in enumerate((k, w, h) for k in ("tiff_ccitt", "group3", "group4") for w in (1, 9, 64, 257, 1728) for h in (1, 17)):
        bm = bitmap_of(rs, i % 3, h, w)
        im = Image.fromarray((bm * 255).astype(np.uint8)).convert("1")
        b = io.BytesIO()
        im.save(b, format="TIFF", compression=kind)
        p = str(tmp_path / ("pil%02d.tif" % i))
        open(p, "wb").write(b.getvalue())
        rgb = np.asarray(Image.open(p).convert("RGB"))
        assert np.array_equal(rgb[:, :, 0], bm * 255), (kind, w, h)
        if L is not None:
            assert np.array_equal(libtiff_bgr(L, p, w, h), rgb[:, :, ::-1]), (kind, w, h)
        args += [p, p + ".bgr"]
        wants.append(rgb[:, :, ::-1])
    assert run(checker, "--decode", *args).returncode == 0
    for i, want in enumerate(wants):
        assert np.array_equal(np.fromfile(args[2 * i + 1], np.uint8).reshape(want.shape), want), args[2 * i]


def test_libtiff_misreads_two_clean_forms(tmp_path):
    """the observations of the module docstring: a 3 x 2 Modified Huffman file whose rows are one byte each loses its last row
    in libtiff and keeps it with two zero bytes behind the stream; the same bitmap word-aligned is misread too"""
    L = load_libtiff()
    if L is None:
        pytest.skip("no libtiff.so.* on this machine")
    bm = np.array([[0, 0, 1], [0, 1, 1]])
    p = tmp_path / "q.tif"
    p.write_bytes(fx.write_fax(bm, fx.MH))
    assert fx.encode(bm, fx.MH) == bytes([0b01110100, 0b00011111])
    ref = libtiff_bgr(L, p, 3, 2)
    assert np.array_equal(ref[0], fx.wanted(bm, 0)[0]) and (ref[1] == 255).all()
    p.write_bytes(fx.write_fax(bm, fx.MH, streams=[fx.encode(bm, fx.MH) + b"\0\0"]))
    assert np.array_equal(libtiff_bgr(L, p, 3, 2), fx.wanted(bm, 0))
    p.write_bytes(fx.write_fax(bm, fx.MHW, streams=[fx.encode(bm, fx.MHW) + b"\0\0"]))
    assert not np.array_equal(libtiff_bgr(L, p, 3, 2), fx.wanted(bm, 0))


def test_word_aligned_rows_begin_at_multiples_of_16_bits(checker, tmp_path):
    """Compression 32771 as TIFF 6.0 states it, on a stream placed by hand (no "align" symbol of the writer): three rows of
    7, 15 and 7 coded bits at bit 0, 16 and 32 of the chunk.  The same rows at bit 0, 8 and 24 are the Compression 2 stream"""
    bm = np.array([[0, 0, 1], [1, 0, 0], [0, 0, 1]])
    rows = ["".join("".join(fx.run_words(c, n)) for c, n in r) for r in ([(0, 2), (1, 1)], [(0, 0), (1, 1), (0, 2)], [(0, 2), (1, 1)])]
    assert [len(r) for r in rows] == [7, 15, 7]
    word = rows[0] + "0" * 9 + rows[1] + "0" + rows[2]
    byte = rows[0] + "0" + rows[1] + "0" + rows[2]
    args = []
    for name, comp, bits in (("w", fx.MHW, word), ("b", fx.MH, byte)):
        assert fx.pack([("bits", bits)]) == fx.encode(bm, comp)
        p = str(tmp_path / (name + ".tif"))
        open(p, "wb").write(fx.write_fax(bm, comp, streams=[fx.pack([("bits", bits)])]))
        args += [p, p + ".bgr"]
    assert run(checker, "--decode", *args).returncode == 0
    for out in args[1::2]:
        assert np.array_equal(np.fromfile(out, np.uint8).reshape(3, 3, 3), fx.wanted(bm, 0))
    # and a row moved off its boundary is not found: the word-aligned stream read as byte-aligned, and the other way round
    open(args[0], "wb").write(fx.write_fax(bm, fx.MH, streams=[fx.pack([("bits", word)])]))
    open(args[2], "wb").write(fx.write_fax(bm, fx.MHW, streams=[fx.pack([("bits", byte)])]))
    for p in args[0::2]:
        r = run(checker, "--decode", p, p + ".bgr")
        assert r.returncode == 1 or not np.array_equal(np.fromfile(p + ".bgr", np.uint8).reshape(3, 3, 3), fx.wanted(bm, 0))


def test_parse_is_parse_fax_and_the_expansion(decoded, checker, tmp_path):
    """Frame::data of parse == of parse_fax + unfax_all == the rows that were encoded, at nominal chunk size, on the whole
    matrix; parse_coded answers "fax" for every file"""
    cases, _, paths = decoded
    args_chunks, args_fax = [], []
    for p in paths:
        args_chunks += [p, p + ".chunks"]
        args_fax += [p, p + ".fax"]
    assert run(checker, "--chunks", *args_chunks).returncode == 0
    assert run(checker, "--route-fax", *args_fax).returncode == 0
    with open(tmp_path / "all.fax", "wb") as f:
        for p in paths:
            f.write(open(p + ".fax", "rb").read())
    r = run(checker, "--unfax", str(tmp_path / "all.fax"), str(tmp_path / "all.chunks"))
    assert r.returncode == 0 and r.stdout.split() == ["ok"] * len(cases)
    got, pos = open(tmp_path / "all.chunks", "rb").read(), 0
    for c, p in zip(cases, paths):
        want = fx.expanded(c.bitmap, c.kw.get("tile"), c.kw.get("rows_per_strip"))
        assert open(p + ".chunks", "rb").read() == want, ("parse differs from the rows that were encoded", c.name)
        assert got[pos:pos + len(want)] == want, ("parse_fax + unfax_all differs from parse", c.name)
        pos += len(want)
    assert pos == len(got)
    r = run(checker, "--why", *paths)
    assert [line.rsplit(": ", 1)[1] for line in r.stdout.strip().splitlines()] == ["fax"] * len(cases)


def refusals():
    """[(name, file bytes, the reason's words, whether libtiff must call the file damaged too)]: one file per refusal class"""
    W, B = fx.WHITE, fx.BLACK
    white16 = [("run", W, 16)]
    bm = np.zeros((2, 16), int)
    bm[0, 1:6] = 1

    def f(symbols, comp, rows=1, width=16, **kw):
        return fx.write_fax(np.zeros((rows, width), int), comp, streams=[fx.pack(symbols)], **kw)

    g4_row0 = fx.row_2d(bm[0], np.zeros(16, int))
    return [
        ("uncompressed mode: the extension code", f([("bits", fx.UNCOMPRESSED + "0" * 16)], fx.G4), "uncompressed mode", True),
        ("uncompressed mode: T4Options bit 1", fx.write_fax(bm, fx.G3, t4=2), "uncompressed mode", False),
        ("uncompressed mode: T6Options bit 1", fx.write_fax(bm, fx.G4, more_tags=[(293, tw.LONG, [2])]), "uncompressed mode", False),
        ("no code word", f([("bits", "0000000011111111" + "1" * 16)], fx.MH), "no code word", True),
        ("a run that passes the width", f([("run", W, 20), ("run", B, 4), ("zeros", 16)], fx.MH), "passes the row's width", True),
        ("a vertical move left of a0", f(g4_row0 + [("v", -2), ("v", 0), ("zeros", 16)], fx.G4, rows=2), "goes left of a0", True),
        ("a row that ends early", f([("eol",), ("run", W, 5), ("eol",)] + white16 + [("zeros", 16)], fx.G3, rows=2), "row ends before its width", True),
        ("a stream that ends early", f([("eol",)] + white16, fx.G3, rows=3), "stream ends before", True),
        ("a missing EOL", f(white16 + [("eol",)] + white16, fx.G3, rows=2), "does not begin with an EOL", True),
        ("four zero bytes as Group 4", tw.write_tiff(np.zeros((4, 4, 1), int), 1, tw.MINISWHITE, drop=(259,), more_tags=[(259, tw.SHORT, [4])]), "stream ends before", True),
        ("zero-length runs beyond the list", f([("horiz",), ("run", W, 0), ("run", B, 0)] * 4 + [("zeros", 16)], fx.G4, width=4), "more changing elements", False),
        ("8 bits", tw.write_tiff(np.zeros((4, 4, 1), int), 8, tw.MINISBLACK, drop=(259,), more_tags=[(259, tw.SHORT, [4])]), "1 bit per sample", False),
        ("2 samples", tw.write_tiff(np.zeros((4, 4, 2), int), 1, tw.MINISBLACK, drop=(259,), more_tags=[(259, tw.SHORT, [3])]), "1 bit per sample", False),
        ("predictor 2", fx.write_fax(bm, fx.G4, more_tags=[(317, tw.SHORT, [2])]), "no predictor", False),
    ]


def test_every_refusal_class_has_its_reason(checker, tmp_path):
    """parse_fax and parse refuse each file with the same reason, parse_coded answers "refused", --decode refuses"""
    cases = refusals()
    paths = []
    for i, (name, data, reason, _) in enumerate(cases):
        paths.append(str(tmp_path / ("r%02d.tif" % i)))
        open(paths[-1], "wb").write(data)
    r = run(checker, "--fax-why", *paths)
    assert r.returncode == 0
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(cases)
    for (name, _, reason, _), line in zip(cases, lines):
        scan, full = line.split(": ", 1)[1].split(" | ")
        assert reason in scan and scan == full, (name, line)
    r = run(checker, "--why", *paths)
    assert [line.rsplit(": ", 1)[1] for line in r.stdout.strip().splitlines()] == ["refused"] * len(cases)
    assert run(checker, "--reject", str(tmp_path)).returncode == 0


def test_libtiff_calls_the_refused_streams_damaged(tmp_path):
    """for the stream-level refusal classes libtiff's warning or error handler fires on the same file: what is refused here is
    what libtiff patches, not a clean file.  Skipped only as a whole, when no libtiff loads"""
    L = load_libtiff()
    if L is None:
        pytest.skip("no libtiff.so.* on this machine")
    cases = refusals()
    paths = []
    for i, (name, data, reason, _) in enumerate(cases):
        paths.append(str(tmp_path / ("r%02d.tif" % i)))
        open(paths[-1], "wb").write(data)
    fired = []
    handler = ctypes.CFUNCTYPE(None, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p)(lambda module, fmt, ap: fired.append(fmt))
    for setter in (L.TIFFSetWarningHandler, L.TIFFSetErrorHandler):
        setter.restype, setter.argtypes = ctypes.c_void_p, [ctypes.c_void_p]
    old = [L.TIFFSetWarningHandler(ctypes.cast(handler, ctypes.c_void_p)), L.TIFFSetErrorHandler(ctypes.cast(handler, ctypes.c_void_p))]
    try:
        for (name, data, _, stream_level), p in zip(cases, paths):
            if not stream_level:
                continue
            del fired[:]
            libtiff_bgr(L, p, 16, 4)
            assert fired, ("libtiff reads this file without a complaint", name)
    finally:
        L.TIFFSetWarningHandler(old[0])
        L.TIFFSetErrorHandler(old[1])


def corpus(seed=12, count=2400):
    """[(compression, t4, width, rows, stream)]: sound streams of every coding, as they are, cut, bit-flipped and spliced"""
    rs = np.random.RandomState(seed)
    bases = []
    for k in range(36):
        cname, comp, ckw = fx.CODINGS[k % len(fx.CODINGS)]
        w, h = int(rs.choice([1, 8, 33, 64, 200])), int(rs.choice([1, 3, 9]))
        enc = {a: b for a, b in ckw.items() if a in ("t4", "k", "fill")}
        bases.append((comp, ckw.get("t4", 0), w, h, fx.encode(bitmap_of(rs, k % 3, h, w), comp, **enc)))
    out = []
    while len(out) < count:
        comp, t4, w, h, s = bases[rs.randint(len(bases))]
        s = bytearray(s)
        kind = rs.randint(6)
        if kind == 0 and len(s) > 1:
            del s[rs.randint(1, len(s)):]
        elif kind == 1:
            s[rs.randint(len(s))] ^= 1 << rs.randint(8)
        elif kind == 2 and len(s) > 2:
            o = bases[rs.randint(len(bases))][4]
            n = rs.randint(1, 6)
            i, j = rs.randint(len(s)), rs.randint(max(1, len(o) - n))
            s[i:i + n] = o[j:j + n]
        elif kind == 3:
            h = max(1, h + int(rs.choice([-1, 1])))
        out.append((comp, t4, w, h, bytes(s)))
    return out


def test_the_scan_agrees_with_the_decoder(checker, tmp_path):
    """2400 streams of every coding - as they are, cut, bit-flipped, spliced, with a row more or less asked for: ccitt::walk as
    the scan says what it says as the decoder, in the sanitizer build (a read past a stream, a write past the rows or past a
    list is its to see).  Both answers occur, and a tenth of the streams at least are accepted"""
    cases = corpus()
    assert len(cases) >= 2000
    with open(tmp_path / "streams.bin", "wb") as f:
        for comp, t4, w, h, s in cases:
            f.write(struct.pack("<5I", comp, t4, w, h, len(s)) + s)
    assert run(checker, "--fax-scan", str(tmp_path / "streams.bin"), str(tmp_path / "verdicts.bin")).returncode == 0
    v = np.fromfile(tmp_path / "verdicts.bin", np.uint8).reshape(-1, 2)
    assert len(v) == len(cases)
    assert (v[:, 0] == v[:, 1]).all()
    print("%d streams, %d accepted" % (len(v), int(v[:, 1].sum())))
    assert v[:, 1].sum() * 10 >= len(v) and (v[:, 1] == 0).sum() * 10 >= len(v), int(v[:, 1].sum())


def sound_frame():
    bm = np.zeros((5, 16), int)
    bm[:, 3:9] = 1
    return bm


def test_fax_rules_are_refused_before_any_device_call(built, pkg):
    """every rule of ocr_tiff_fax and every refusal class of the streams drives ocr_tiff_unfax and ocr_tiff_decode_fax to
    OCR_ERR_ARG with a message that names it - on a machine with or without a GPU: the check comes before the runtime is
    touched, so nothing was launched and the output buffer is as it was"""
    def refused_as(t, what):
        for call in (t.unfax, t.decode):
            with pytest.raises(pkg.OcrError, match=what) as e:
                call(fill=0xA5)
            assert e.value.code == -1  # OCR_ERR_ARG
            assert (e.value.out == 0xA5).all()

    W, B = fx.WHITE, fx.BLACK
    bm = sound_frame()

    def tampered(**kw):
        c = fx.coded(bm, kw.pop("compression", fx.G4), rows_per_strip=3, **{k: kw.pop(k) for k in ("t4", "chunks") if k in kw})
        if "records" in kw:
            c["chunks"] = kw.pop("records")
        t = fx.to_pkg(pkg, c)
        for name, value in kw.items():
            if name in ("compression", "chunks_len", "bytes_len", "bytes"):
                setattr(t.c.coded, name, value)
            elif name == "t4_options":
                t.c.t4_options = value
            else:
                setattr(t.c.coded.frame, name, value)
        return t, c

    _, sound = tampered()
    (o0, l0, r0), (o1, l1, r1) = sound["chunks"]
    refused_as(tampered(width=0)[0], "positive")
    refused_as(tampered(bits_per_sample=8)[0], "1 bit per sample")
    refused_as(tampered(bits_per_sample=8, samples_per_pixel=2)[0], "1 bit per sample")
    refused_as(tampered(photometric=3)[0], "photometric 0 or 1")
    refused_as(tampered(compression=5)[0], "compression must be 2, 3, 4 or 32771")
    refused_as(tampered(t4_options=2, compression=3)[0], "uncompressed mode")
    refused_as(tampered(t4_options=8, compression=3)[0], "T4Options")
    refused_as(tampered(t4_options=1)[0], "T4Options")
    refused_as(tampered(chunks_len=1)[0], "as many chunk records")
    refused_as(tampered(records=[(o0, l0, 0), (o1, l1, r1)])[0], "rows must be 1 .. tile_height")
    refused_as(tampered(records=[(o0, l0, r0), (o1, l1 + 1, r1)])[0], "outside the pool")
    refused_as(tampered(bytes=None)[0], "byte pool is missing")
    refused_as(tampered(records=[(o0, l0, r0), (o1, l1, 3)])[0], "stream ends before")
    refused_as(tampered(tile_width=8193, width=8193)[0], "wider than the device")  # (a bound of the device comes before any stream is walked)
    g4_row0 = fx.row_2d(np.array([0] + [1] * 5 + [0] * 10), np.zeros(16, int))
    for symbols, comp, rows, width, what in (
            ([("bits", fx.UNCOMPRESSED + "0" * 16)], fx.G4, 1, 16, "uncompressed mode"),
            ([("bits", "0000000011111111" + "1" * 16)], fx.MH, 1, 16, "no code word"),
            ([("run", W, 20), ("run", B, 4), ("zeros", 16)], fx.MH, 1, 16, "passes the row's width"),
            (g4_row0 + [("v", -2), ("v", 0), ("zeros", 16)], fx.G4, 2, 16, "goes left of a0"),
            ([("eol",), ("run", W, 5), ("eol",), ("run", W, 16), ("zeros", 16)], fx.G3, 2, 16, "row ends before its width"),
            ([("eol",), ("run", W, 16)], fx.G3, 3, 16, "stream ends before"),
            ([("run", W, 16), ("eol",), ("run", W, 16)], fx.G3, 2, 16, "does not begin with an EOL"),
            ([("bits", "0" * 32)], fx.G4, 4, 4, "stream ends before"),
            ([("horiz",), ("run", W, 0), ("run", B, 0)] * 4 + [("zeros", 16)], fx.G4, 1, 4, "more changing elements")):
        refused_as(fx.to_pkg(pkg, fx.one_chunk(symbols, width, rows, comp)), what)
    # a sound chunk wider than the device expansion takes: tiff::unfax_all is the route for such a frame
    wide = fx.coded(np.zeros((1, 8193), int), fx.G4)
    refused_as(fx.to_pkg(pkg, wide), "wider than the device")
    # more chunks than the device stage takes: 2^20 + 1 strips of one row
    n = (1 << 20) + 1
    records = np.ones(n, pkg.TIFF_CHUNK)
    records["byte_off"] = np.arange(n)
    many = dict(fx.one_chunk([("v", 0)], 1, 1, fx.G4), h=n, tile=(1, 1), chunks=records, data=b"\x80" * n)
    refused_as(fx.to_pkg(pkg, many), "beyond the device bounds")


def test_the_library_exports_the_fax_route(built, pkg):
    L = pkg.lib()
    for name in ("ocr_tiff_unfax", "ocr_tiff_decode_fax", "ocr_tiff_time_fax", "ocr_tiff_time_fax_batch"):
        assert hasattr(L, name) and name in pkg.EXPORTS
    assert pkg.FRAME_TIFF_FAX == 10
