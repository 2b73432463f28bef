"""TIFF requests, host half (host/tiff_decode.h): the container, PackBits / LZW / Deflate expansion and the host pixel stage,
which must return what cv::imdecode(IMREAD_COLOR) returns.  The files are written tag by tag and sample by sample
(tests/tiff_writer.py); every decode is compared byte for byte with the numpy statement of the rules (tiff_writer.convert),
with TIFFReadRGBAImageOriented of the system's libtiff through ctypes (alpha dropped, RGB swapped to BGR) and, where Pillow
agrees by design (8-bit grey, RGB, palette, bilevel), with Pillow.  The decoder runs in host/tiff_check.cpp, a plain host
program built with -fsanitize=address,undefined.  The device half is tests/test_gpu_tiff.py.

One difference from libtiff 4.3.0 is deliberate.  Its routines for 16-bit grey and for 8-bit grey with an extra sample step
over the hidden part of a tile that is clipped on the RIGHT by the wrong amount (bytes for samples): of such a tile only the
first row comes back right, the others are read from elsewhere in the tile.  The decoder here returns what the file holds.
For those forms the libtiff comparison therefore uses images a whole number of tiles wide (clipped at the bottom only);
test_libtiff_misreads_right_clipped_tiles_of_two_forms pins the observation itself."""
import ctypes
import io
import os
import resource
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiff_writer as tw  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cpp-paddle-ocr_amd", "host")
WIDTHS = [1, 3, 4, 5, 31, 32, 33, 65, 257]
HEIGHTS = [1, 2, 5, 17]
SKEW_FORMS = ("black16", "white16", "greya8", "greya16", "whitea8")  # libtiff 4.3.0 misreads their right-clipped tiles


def build_check(directory, *flags):
    exe = os.path.join(str(directory), "tiff_check" + ("_san" if flags else ""))
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", *flags, "-o", exe, os.path.join(HOST, "tiff_check.cpp"), "-ldl"])
    return exe


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """host/tiff_check.cpp with AddressSanitizer and UBSan: a stand-alone host program, nothing of it is loaded into Python"""
    return build_check(tmp_path_factory.mktemp("tiffcheck"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


class Case:
    def __init__(self, name, data, want, libtiff=True, pillow=False):
        self.name, self.data, self.want, self.libtiff, self.pillow = name, data, want, libtiff, pillow


def decode_all(exe, cases, directory):
    """every file through ONE tiff_check --decode process; the decoded BGR arrays"""
    args = []
    for i, c in enumerate(cases):
        src = os.path.join(str(directory), "c%05d.tif" % i)
        with open(src, "wb") as f:
            f.write(c.data)
        args += [src, src + ".bgr"]
    r = subprocess.run([exe, "--decode"] + args, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = []
    for i, c in enumerate(cases):
        h, w = c.want.shape[:2]
        out.append(np.fromfile(os.path.join(str(directory), "c%05d.tif.bgr" % i), np.uint8).reshape(h, w, 3))
    return out


def make(rs, form, h, w, libtiff=True, **kw):
    name, photometric, bits, spp, extra = form
    samples, colormap = tw.random_case(rs, form, h, w)
    planar = kw.get("planar", 1)
    data = tw.write_tiff(samples, bits, photometric, extra=extra, colormap=colormap, rs=rs, **kw)
    label = "%s %dx%d %s" % (name, w, h, " ".join("%s=%s" % kv for kv in sorted(kw.items())))
    pillow = name in ("black8", "rgb8", "pal8", "black1", "white1") and planar == 1 and kw.get("fill_order", 1) == 1
    return Case(label, data, tw.convert(samples, bits, photometric, planar, extra, colormap), libtiff, pillow)


def matrix(seed=1):
    """every form x every compression x {strips, tiles} x both byte orders, the widths and heights of the lists in turn;
    the predictor on for every LZW / Deflate file of 8- and 16-bit samples but one in three; planar 2 wherever it is in scope"""
    rs = np.random.RandomState(seed)
    cases, k = [], 0
    for form in tw.FORMS:
        name, photometric, bits, spp, extra = form
        for comp in tw.COMPRESSIONS:
            for be in (False, True):
                for layout in ("strips", "tiles"):
                    w, h = WIDTHS[k % len(WIDTHS)], HEIGHTS[(k // 2) % len(HEIGHTS)]
                    k += 1
                    kw = dict(compression=comp, big_endian=be)
                    if comp in (tw.LZW, tw.ADOBE_DEFLATE, tw.DEFLATE) and bits >= 8 and k % 3:
                        kw["predictor"] = 2
                    if layout == "strips":
                        kw["rows_per_strip"] = (None, 1, 2, 4, h + 3)[k % 5]
                    else:
                        kw["tile"] = ((16, 16), (32, 16), (16, 32))[k % 3]
                        if name in SKEW_FORMS:
                            w = (w + kw["tile"][0] - 1) // kw["tile"][0] * kw["tile"][0]
                    cases.append(make(rs, form, h, w, **kw))
                    if bits >= 8 and (photometric == tw.RGB or (photometric <= 1 and spp >= 2)):
                        cases.append(make(rs, form, h, w, planar=2, **kw))
    return cases


def variants(seed=2):
    """every width x every height for a bilevel, a 4-bit, a predicted RGB and a predicted 16-bit RGBA form; FillOrder 2;
    RowsPerStrip absent and above the height; a ColorMap of 8-bit values; a Predictor tag on an uncompressed and a PackBits file
    (not read); foreign tags of other types; Orientation 1"""
    rs = np.random.RandomState(seed)
    by_name = {f[0]: f for f in tw.FORMS}
    cases = []
    for w in WIDTHS:
        for h in HEIGHTS:
            cases.append(make(rs, by_name["white1"], h, w, compression=tw.PACKBITS, rows_per_strip=3))
            cases.append(make(rs, by_name["pal4"], h, w, compression=tw.LZW, big_endian=True))
            cases.append(make(rs, by_name["rgb8"], h, w, compression=tw.LZW, predictor=2, rows_per_strip=2))
            cases.append(make(rs, by_name["rgba16"], h, w, compression=tw.ADOBE_DEFLATE, predictor=2, big_endian=bool(w & 1), tile=(16, 16)))
            cases.append(make(rs, by_name["black16"], h, w, compression=tw.LZW, predictor=2, big_endian=bool(h & 1)))
    for name in ("white1", "pal2", "black4", "rgb8", "black16"):
        for comp in tw.COMPRESSIONS:
            cases.append(make(rs, by_name[name], 5, 33, compression=comp, fill_order=2))
    cases.append(make(rs, by_name["rgb8"], 5, 33, rows_per_strip=100))
    cases.append(make(rs, by_name["rgb8"], 5, 33, drop=(278,)))
    cases.append(make(rs, by_name["rgb8"], 5, 33, predictor_tag=2))
    cases.append(make(rs, by_name["black8"], 5, 33, compression=tw.PACKBITS, predictor_tag=2))
    cases.append(make(rs, by_name["rgb8"], 5, 33, orientation=1,
                      more_tags=[(282, tw.RATIONAL, [(300, 1)]), (283, tw.RATIONAL, [(300, 1)]), (296, tw.SHORT, [2]), (305, tw.ASCII, list(b"writer\0"))]))
    s = rs.randint(0, 16, (5, 33, 1))
    cm = rs.randint(0, 256, (3, 16))
    cases.append(Case("pal4 with an 8-bit ColorMap", tw.write_tiff(s, 4, tw.PALETTE, colormap=cm), tw.convert(s, 4, tw.PALETTE, colormap=cm)))
    # a long flat file: LZW strings grow to the table's end, the width changes at 511, 1023 and 2047 and the table is cleared
    flat = np.repeat(rs.randint(0, 256, (40, 40, 3)), 8, 1)
    cases.append(Case("rgb8 320x40 flat LZW", tw.write_tiff(flat, 8, tw.RGB, compression=tw.LZW), tw.convert(flat, 8, tw.RGB)))
    noise = rs.randint(0, 256, (64, 257, 3))
    cases.append(Case("rgb8 257x64 noise LZW", tw.write_tiff(noise, 8, tw.RGB, compression=tw.LZW), tw.convert(noise, 8, tw.RGB)))
    return cases


@pytest.fixture(scope="module")
def decoded(checker, tmp_path_factory):
    cases = matrix() + variants()
    return cases, decode_all(checker, cases, tmp_path_factory.mktemp("tiffs"))


def test_the_matrix_covers_the_case_list():
    cases = matrix()
    names = " ".join(c.name for c in cases)
    assert len(cases) >= len(tw.FORMS) * len(tw.COMPRESSIONS) * 4
    for token in [f[0] + " " for f in tw.FORMS] + ["compression=%d " % c for c in tw.COMPRESSIONS] + ["tile=", "rows_per_strip=", "big_endian=True",
                                                                                                       "planar=2", "predictor=2"]:
        assert token in names, token
    assert {c.want.shape[1] for c in cases} >= set(WIDTHS) and {c.want.shape[0] for c in cases} == set(HEIGHTS)


def test_decoder_equals_the_numpy_rules(decoded):
    cases, got = decoded
    for c, g in zip(cases, got):
        assert np.array_equal(g, c.want), (c.name, int((g != c.want).sum()))


def load_libtiff():
    for name in ("libtiff.so.5", "libtiff.so.6", "libtiff.so"):
        try:
            L = ctypes.CDLL(name)
        except OSError:
            continue
        L.TIFFOpen.restype = ctypes.c_void_p
        L.TIFFOpen.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
        L.TIFFReadRGBAImageOriented.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        L.TIFFClose.argtypes = [ctypes.c_void_p]
        return L
    return None


def libtiff_bgr(L, path, w, h):
    """TIFFReadRGBAImageOriented (top-left origin) -> BGR, alpha dropped; None when libtiff refuses the file"""
    t = L.TIFFOpen(str(path).encode(), b"r")
    if not t:
        return None
    buf = np.zeros((h, w, 4), np.uint8)  # a pixel is R | G << 8 | B << 16 | A << 24 on this little-endian machine
    ok = L.TIFFReadRGBAImageOriented(t, w, h, buf.ctypes.data, 1, 0)
    L.TIFFClose(t)
    return buf[:, :, 2::-1].copy() if ok else None


def test_decoder_equals_libtiff(decoded, tmp_path):
    """skipped only as a whole, when no libtiff loads; a written file that libtiff refuses fails"""
    L = load_libtiff()
    if L is None:
        pytest.skip("no libtiff.so.* on this machine")
    cases, got = decoded
    path = tmp_path / "x.tif"
    for c, g in zip(cases, got):
        if not c.libtiff:
            continue
        path.write_bytes(c.data)
        ref = libtiff_bgr(L, path, g.shape[1], g.shape[0])
        assert ref is not None, ("libtiff refuses a written file", c.name)
        assert np.array_equal(g, ref), (c.name, int((g != ref).sum()))


def test_decoder_equals_pillow(decoded):
    from PIL import Image
    cases, got = decoded
    seen = 0
    for c, g in zip(cases, got):
        if not c.pillow:
            continue
        im = Image.open(io.BytesIO(c.data))
        rgb = np.asarray(im.convert("RGB"))
        assert np.array_equal(g, rgb[:, :, ::-1]), c.name
        seen += 1
    assert seen >= 20


def test_libtiff_misreads_right_clipped_tiles_of_two_forms(checker, tmp_path):
    """the known difference of the module docstring, observed: 16-bit grey and grey with alpha, 33 x 17 in 16 x 16 tiles - the
    decoder returns the file's samples; libtiff agrees on every pixel outside the right-hand tiles and on their first rows"""
    L = load_libtiff()
    if L is None:
        pytest.skip("no libtiff.so.* on this machine")
    rs = np.random.RandomState(5)
    by_name = {f[0]: f for f in tw.FORMS}
    cases = [make(rs, by_name[n], 17, 33, tile=(16, 16)) for n in ("black16", "greya8")]
    for c, g in zip(cases, decode_all(checker, cases, tmp_path)):
        assert np.array_equal(g, c.want), c.name
        p = tmp_path / "skew.tif"
        p.write_bytes(c.data)
        ref = libtiff_bgr(L, p, 33, 17)
        assert ref is not None
        assert np.array_equal(ref[:, :32], g[:, :32]) and np.array_equal(ref[0], g[0]) and np.array_equal(ref[16], g[16]), c.name


def hostile_files(seed=3):
    """the refusal corpus: {name: bytes}"""
    rs = np.random.RandomState(seed)
    s = rs.randint(0, 256, (5, 33, 3))
    good = tw.write_tiff(s, 8, tw.RGB)
    ifd = int.from_bytes(good[4:8], "little")
    out = {}
    out["empty"] = b""
    out["magic_only"] = good[:8]
    out["bigtiff"] = b"II+\0" + good[4:]
    out["ifd_offset_past_end"] = good[:4] + (len(good) + 10).to_bytes(4, "little") + good[8:]
    out["ifd_offset_zero"] = good[:4] + b"\0\0\0\0" + good[8:]
    out["ifd_cut_in_count"] = good[:ifd + 1]
    out["ifd_cut_in_entries"] = good[:ifd + 2 + 12 * 3 + 5]
    out["ifd_claims_more_entries"] = good[:ifd] + b"\xff\xff" + good[ifd + 2:]
    out["strip_offset_past_end"] = tw.write_tiff(s, 8, tw.RGB, drop=(273,), more_tags=[(273, tw.LONG, [1 << 30])])
    out["strip_count_past_end"] = tw.write_tiff(s, 8, tw.RGB, drop=(279,), more_tags=[(279, tw.LONG, [1 << 30])])
    out["strip_inside_header"] = tw.write_tiff(s, 8, tw.RGB, drop=(273,), more_tags=[(273, tw.LONG, [4])])
    # BitsPerSample's three values stored over the header (value offset 2)
    k = good.index(bytes([0x02, 0x01, 0x03, 0x00, 0x03, 0x00, 0x00, 0x00]), ifd)
    out["table_over_header"] = good[:k + 8] + (2).to_bytes(4, "little") + good[k + 12:]
    out["table_past_end"] = good[:k + 8] + (len(good) - 2).to_bytes(4, "little") + good[k + 12:]
    out["short_strip_uncompressed"] = tw.write_tiff(s, 8, tw.RGB, drop=(279,), more_tags=[(279, tw.LONG, [5 * 33 * 3 - 1])])
    for comp in (tw.PACKBITS, tw.LZW, tw.ADOBE_DEFLATE):
        full = tw.compress(np.asarray(s, np.uint8).tobytes(), comp, 99)
        out["short_chunk_%d" % comp] = tw.write_tiff(s, 8, tw.RGB, compression=comp, streams=[full[:len(full) // 2]])
        out["empty_chunk_%d" % comp] = tw.write_tiff(s, 8, tw.RGB, compression=comp, streams=[b""])
    # LZW: clear, byte 65, then code 300 while the table ends at 258
    bits = "{:09b}{:09b}{:09b}".format(256, 65, 300)
    bits += "0" * (-len(bits) % 8)
    out["lzw_code_beyond_table"] = tw.write_tiff(s, 8, tw.RGB, compression=tw.LZW, streams=[int(bits, 2).to_bytes(len(bits) // 8, "big")])
    out["lzw_old_style"] = tw.write_tiff(s, 8, tw.RGB, compression=tw.LZW, streams=[b"\x00\x01" + bytes(600)])
    out["lzw_no_clear_first_code_high"] = tw.write_tiff(s, 8, tw.RGB, compression=tw.LZW, streams=[b"\xff\xff\xff\xff"])
    out["claims_2_31_by_1"] = tw.write_tiff(s, 8, tw.RGB, drop=(256, 257), more_tags=[(256, tw.LONG, [1 << 31]), (257, tw.LONG, [1])])
    out["claims_65536_by_65536"] = tw.write_tiff(s, 8, tw.RGB, drop=(256, 257), more_tags=[(256, tw.LONG, [65536]), (257, tw.LONG, [65536])])
    out["claims_8192_squared_lzw_tile"] = tw.write_tiff(s, 8, tw.RGB, compression=tw.LZW, drop=(256, 257, 278),
                                                        more_tags=[(256, tw.LONG, [8192]), (257, tw.LONG, [8192])])
    out["zero_width"] = tw.write_tiff(s, 8, tw.RGB, drop=(256,), more_tags=[(256, tw.LONG, [0])])
    out["no_photometric"] = tw.write_tiff(s, 8, tw.RGB, drop=(262,))
    out["no_byte_counts"] = tw.write_tiff(s, 8, tw.RGB, drop=(279,))
    out["rows_per_strip_zero"] = tw.write_tiff(s, 8, tw.RGB, rows_per_strip=0, drop=(278,), more_tags=[(278, tw.LONG, [0])])
    out["width_as_rational"] = tw.write_tiff(s, 8, tw.RGB, drop=(256,), more_tags=[(256, tw.RATIONAL, [(33, 1)])])
    out["tile_width_not_16"] = tw.write_tiff(s, 8, tw.RGB, tile=(24, 16))
    for comp in (2, 3, 4, 6, 7, 34712, 50000):
        out["compression_%d" % comp] = tw.write_tiff(s, 8, tw.RGB, drop=(259,), more_tags=[(259, tw.SHORT, [comp])])
    for ph in (4, 6, 8, 9, 10, 32844):
        out["photometric_%d" % ph] = tw.write_tiff(s, 8, tw.RGB, drop=(262,), more_tags=[(262, tw.SHORT, [ph])])
    out["predictor_3"] = tw.write_tiff(s, 8, tw.RGB, compression=tw.LZW, predictor_tag=3)
    out["sample_format_float"] = tw.write_tiff(s, 8, tw.RGB, more_tags=[(339, tw.SHORT, [3, 3, 3])])
    out["rgb_4_bits"] = tw.write_tiff(rs.randint(0, 16, (5, 33, 3)), 4, tw.RGB)
    out["rgb_32_bits"] = tw.write_tiff(s, 8, tw.RGB, drop=(258,), more_tags=[(258, tw.SHORT, [32, 32, 32])])
    out["mixed_bits"] = tw.write_tiff(s, 8, tw.RGB, drop=(258,), more_tags=[(258, tw.SHORT, [8, 8, 16])])
    out["palette_16_bits"] = tw.write_tiff(rs.randint(0, 65536, (5, 33, 1)), 16, tw.PALETTE, colormap=rs.randint(0, 65536, (3, 256)))
    out["palette_without_colormap"] = tw.write_tiff(rs.randint(0, 256, (5, 33, 1)), 8, tw.PALETTE)
    out["cmyk_16_bits"] = tw.write_tiff(rs.randint(0, 65536, (5, 33, 4)), 16, tw.CMYK)
    out["cmyk_planar"] = tw.write_tiff(rs.randint(0, 256, (5, 33, 4)), 8, tw.CMYK, planar=2)
    out["cmyk_three_samples"] = tw.write_tiff(s, 8, tw.CMYK)
    out["grey_predictor_4_bits"] = tw.write_tiff(rs.randint(0, 16, (5, 33, 1)), 4, tw.MINISBLACK, compression=tw.LZW, predictor_tag=2)
    out["rgb_two_samples"] = tw.write_tiff(s[:, :, :2], 8, tw.RGB)
    out["fill_order_3"] = tw.write_tiff(s, 8, tw.RGB, more_tags=[(266, tw.SHORT, [3])])
    return out


def test_refusal_corpus_is_refused_and_allocates_nothing_large(checker, tmp_path):
    """tiff_check --reject over the corpus: under the sanitizers (no read outside a file's bytes, no overflow), and once more in
    a plain build whose address space is capped at 256 MiB - a hostile header buys no memory"""
    corpus = tmp_path / "corpus"
    corpus.mkdir()
    files = hostile_files()
    assert len(files) >= 50
    for name, data in files.items():
        (corpus / name).write_bytes(data)
    r = subprocess.run([checker, "--reject", str(corpus)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    assert r.stdout.split()[:4] == ["refused", str(len(files)), "accepted", "0"]
    plain = build_check(tmp_path)
    r = subprocess.run([plain, "--reject", str(corpus)], capture_output=True, text=True,
                       preexec_fn=lambda: resource.setrlimit(resource.RLIMIT_AS, (256 << 20, 256 << 20)))
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    # and the check itself checks: a good file in the directory is reported
    (corpus / "good").write_bytes(tw.write_tiff(np.zeros((2, 2, 3), int), 8, tw.RGB))
    r = subprocess.run([plain, "--reject", str(corpus)], capture_output=True, text=True)
    assert r.returncode == 1 and "accepted 1 good" in r.stdout


def tiff_frame(pkg, **kw):
    """a sound 4 x 5 RGB frame in one strip, then the overrides"""
    f = pkg.TiffFrame(kw.pop("w", 4), kw.pop("h", 5), kw.pop("photometric", 2), kw.pop("bits", 8), kw.pop("samples", 3), np.zeros(kw.pop("size", 60), np.uint8),
                      tile=(kw.pop("tile_width", 4), kw.pop("tile_height", 5)))
    for k, v in kw.items():
        setattr(f.c, k, v)
    return f


def test_descriptor_rules_are_refused_before_any_device_call(built, pkg):
    """every rule of ocr_tiff_frame drives ocr_tiff_decode to OCR_ERR_ARG with a message that names it - on a machine with or
    without a GPU: the check comes before the runtime is touched, so nothing was launched"""
    def refused_as(f, what):
        with pytest.raises(pkg.OcrError, match=what) as e:
            f.decode()
        assert e.value.code == -1  # OCR_ERR_ARG

    refused_as(tiff_frame(pkg, w=0), "positive")
    refused_as(tiff_frame(pkg, h=-3), "positive")
    refused_as(tiff_frame(pkg, w=70000, h=70000), "64 Mpixel")
    refused_as(tiff_frame(pkg, bits=3), "bits per sample")
    refused_as(tiff_frame(pkg, bits=32), "bits per sample")
    refused_as(tiff_frame(pkg, samples=0), "samples per pixel")
    refused_as(tiff_frame(pkg, samples=17), "samples per pixel")
    refused_as(tiff_frame(pkg, planar=3), "planar must be")
    refused_as(tiff_frame(pkg, predictor=3), "predictor must be")
    refused_as(tiff_frame(pkg, big_endian=2), "0 or 1")
    refused_as(tiff_frame(pkg, premultiply=-1), "0 or 1")
    refused_as(tiff_frame(pkg, photometric=6), "photometric")
    refused_as(tiff_frame(pkg, photometric=4), "photometric")
    refused_as(tiff_frame(pkg, samples=2), "fewer samples")
    refused_as(tiff_frame(pkg, photometric=5), "fewer samples")
    refused_as(tiff_frame(pkg, bits=4), "1, 2 and 4 bits")
    refused_as(tiff_frame(pkg, photometric=1, bits=4, samples=1, predictor=2), "1, 2 and 4 bits")
    refused_as(tiff_frame(pkg, photometric=3, bits=16, samples=1), "palette")
    refused_as(tiff_frame(pkg, photometric=5, bits=16, samples=4), "CMYK")
    refused_as(tiff_frame(pkg, photometric=5, samples=4, planar=2), "CMYK")
    refused_as(tiff_frame(pkg, photometric=1, samples=1, planar=2), "planar 2")
    refused_as(tiff_frame(pkg, premultiply=1), "premultiply")
    refused_as(tiff_frame(pkg, photometric=1, samples=2, premultiply=1), "premultiply")
    refused_as(tiff_frame(pkg, tile_width=0), "tile_width")
    refused_as(tiff_frame(pkg, tile_height=-16), "tile_width")
    refused_as(tiff_frame(pkg, tile_width=1 << 20, tile_height=1 << 20), "tile_width")
    refused_as(tiff_frame(pkg, w=8000, h=8000, samples=16, bits=16, tile_width=8000, tile_height=8000), "1 GiB")
    refused_as(tiff_frame(pkg, data_len=59), "data_len")
    refused_as(tiff_frame(pkg, tile_height=6), "data_len")  # a chunk is at its nominal size: 6 rows of 12 bytes
    refused_as(tiff_frame(pkg, tile_width=16, tile_height=16), "data_len")
    refused_as(tiff_frame(pkg, data=None), "data_len")
