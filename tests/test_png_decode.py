"""PNG requests, host half (host/png_decode.h): our own container parser, zlib's inflate, and the host pixel stage, which
must return what cv::imdecode(IMREAD_COLOR) returns - alpha dropped (not composited), the high byte of 16-bit samples, no
gamma.  The expectation is built from the samples the file was written from (tests/png_writer.py); Pillow only vouches
for the writer.  The device half is tests/test_gpu_png.py, with the same case table."""
import io
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_writer as pw  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cpp-paddle-ocr_amd", "host")
TOOL = os.path.join(HOST, "decode_tool")

# Average and Paeth on a first row (of the image, and of every Adam7 pass), every filter in both patterns
MIXED = ([3, 4, 0, 1, 2, 4, 3, 2], [4, 3, 2, 2, 1, 0, 4])
FILTER_CHOICES = [0, 1, 2, 3, 4, MIXED[0], MIXED[1]]


def make_case(rs, height, width, ct, depth, interlace, filters, name=None):
    """(name, file bytes, expected RGB array)"""
    s = pw.random_samples(rs, height, width, ct, depth)
    pal = rs.randint(0, 256, (max(1, (1 << depth) - 1), 3)) if ct == 3 else None  # one index past PLTE: black
    data = pw.write_png(s, ct, depth, interlace, filters, palette=pal, idat_pieces=1 + (height * width) % 3)
    tag = name or "type %d depth %d interlace %d filters %s %dx%d" % (ct, depth, interlace, filters, height, width)
    return tag, data, pw.expected_bgr(s, ct, depth, pal)[:, :, ::-1]


def matrix(sizes, seed):
    """all 15 legal (colour type, depth) pairs x interlace {0, 1} x each of the five filters on every row and the two mixed
    patterns, the sizes taken in turn"""
    rs = np.random.RandomState(seed)
    cases, k = [], 0
    for ct, depth in pw.LEGAL:
        for interlace in (0, 1):
            for filters in FILTER_CHOICES:
                h, w = sizes[k % len(sizes)]
                k += 1
                cases.append(make_case(rs, h, w, ct, depth, interlace, filters))
    return cases


def decode_files(cases, tmp_path, *flags, env=None):
    """all files through one decode_tool process; the decoded RGB arrays"""
    from PIL import Image
    args = []
    for i, (_, data, _) in enumerate(cases):
        src = tmp_path / ("p%04d.png" % i)
        src.write_bytes(data)
        args += [str(src), str(tmp_path / ("p%04d.ppm" % i))]
    r = subprocess.run([TOOL, *flags] + args, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return [np.array(Image.open(tmp_path / ("p%04d.ppm" % i))) for i in range(len(cases))]


def check_cases(cases, tmp_path, *flags, env=None):
    for (name, _, want), got in zip(cases, decode_files(cases, tmp_path, *flags, env=env)):
        assert got.shape == want.shape, (name, got.shape, want.shape)
        assert np.array_equal(got, want), (name, int(np.abs(got.astype(int) - want).max()))


@pytest.fixture(scope="module")
def tool(built):
    subprocess.check_call(["make", "-s", "-C", HOST])
    return TOOL


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """host/png_check.cpp as a plain host program under AddressSanitizer and UBSan: its own main, the runtimes linked in
    statically"""
    exe = str(tmp_path_factory.mktemp("pngcheck") / "png_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(HOST, "png_check.cpp"), "-ldl"])
    return exe


def run_checker(checker, tmp_path, files):
    bundle = tmp_path / "bundle.bin"
    bundle.write_bytes(b"".join(struct.pack("<I", len(f)) + f for f in files))
    r = subprocess.run([checker, str(bundle)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    verdicts = [l for l in r.stdout.splitlines() if l.startswith("verdicts ")][0][9:]
    assert len(verdicts) == len(files)
    return verdicts


def test_pillow_reads_back_the_writers_samples():
    """the writer, not the decoder: in the modes where Pillow hands out the raw samples (1, L, P, LA, RGB, RGBA, I;16) its
    reading of the writer's files is the generated samples - every filter, interlaced or not"""
    from PIL import Image
    rs = np.random.RandomState(5)
    for ct, depth, mode in ((0, 1, "1"), (0, 8, "L"), (3, 8, "P"), (3, 2, "P"), (4, 8, "LA"), (2, 8, "RGB"), (6, 8, "RGBA"), (0, 16, "I;16")):
        for interlace in (0, 1):
            for filters in FILTER_CHOICES:
                s = pw.random_samples(rs, 11, 13, ct, depth)
                pal = rs.randint(0, 256, (1 << depth, 3)) if ct == 3 else None
                im = Image.open(io.BytesIO(pw.write_png(s, ct, depth, interlace, filters, palette=pal, idat_pieces=2)))
                im.load()
                assert im.mode in (mode, "I;16B") if mode == "I;16" else im.mode == mode, (ct, depth, im.mode)
                got = np.array(im).astype(np.int64)
                if mode == "1":
                    got = (got != 0).astype(np.int64)
                want = s[:, :, 0] if s.shape[2] == 1 else s
                assert np.array_equal(got, want), (ct, depth, interlace, filters)
                if ct == 3:
                    assert np.array_equal(np.array(im.getpalette()).reshape(-1, 3)[:len(pal)], pal)


def test_host_decoder_against_construction(tool, tmp_path):
    """every legal (colour type, depth) pair, interlaced and not, every filter: the host pixel stage (decode_tool without
    --device, OCR_DEVICE_PNG=0 on top) gives the pixels the conversion rules give for the generated samples"""
    check_cases(matrix([(11, 13), (9, 5), (1, 1), (3, 2), (17, 33)], seed=7), tmp_path, env={"OCR_DEVICE_PNG": "0"})


def test_alpha_is_dropped_not_composited(tool, tmp_path):
    """RGBA with alpha 0 / 128 / 255 (and grey + alpha): the colour samples come back untouched.  libpng's simplified API,
    the path before, composites them on black."""
    rs = np.random.RandomState(11)
    rgba = pw.random_samples(rs, 12, 9, 6, 8)
    rgba[:, :, 3] = np.array([0, 128, 255])[np.arange(9) % 3][None, :]
    ga = pw.random_samples(rs, 12, 9, 4, 8)
    ga[:, :, 1] = np.array([0, 128, 255])[np.arange(9) % 3][None, :]
    cases = [("rgba", pw.write_png(rgba, 6, 8, filters=4), rgba[:, :, :3].astype(np.uint8)),
             ("grey alpha", pw.write_png(ga, 4, 8, filters=3), np.repeat(ga[:, :, :1], 3, 2).astype(np.uint8))]
    check_cases(cases, tmp_path)


def test_sixteen_bit_samples_keep_their_high_byte(tool, tmp_path):
    """16-bit grey / RGB / RGBA: the high byte of every sample (png_set_strip_16), not a linear-to-sRGB conversion"""
    rs = np.random.RandomState(12)
    cases = []
    for ct in (0, 2, 4, 6):
        s = pw.random_samples(rs, 10, 7, ct, 16)
        want = (s >> 8).astype(np.uint8)
        want = np.repeat(want[:, :, :1], 3, 2) if ct in (0, 4) else want[:, :, :3]
        cases.append(("type %d" % ct, pw.write_png(s, ct, 16, filters=MIXED[0]), want))
    check_cases(cases, tmp_path)


def test_gamma_and_colour_chunks_change_nothing(tool, tmp_path):
    """a file with gAMA 0.5 (and sRGB, bKGD, tRNS) decodes to the pixels of the same file without them"""
    rs = np.random.RandomState(13)
    cases = []
    for ct, depth in ((2, 8), (0, 16), (2, 16), (3, 4)):
        s = pw.random_samples(rs, 8, 6, ct, depth)
        pal = rs.randint(0, 256, (1 << depth, 3)) if ct == 3 else None
        want = pw.expected_bgr(s, ct, depth, pal)[:, :, ::-1]
        trns = pw.chunk(b"tRNS", bytes([0, 128]) if ct == 3 else struct.pack(">H", 5) if ct == 0 else struct.pack(">HHH", 1, 2, 3))
        cases.append(("plain", pw.write_png(s, ct, depth, palette=pal, filters=1), want))
        cases.append(("gamma", pw.write_png(s, ct, depth, palette=pal, filters=1, ancillary=[pw.chunk(b"gAMA", struct.pack(">I", 50000))]), want))
        cases.append(("all", pw.write_png(s, ct, depth, palette=pal, filters=1, ancillary=[pw.chunk(b"gAMA", struct.pack(">I", 50000)), pw.chunk(b"sRGB", b"\0")],
                                          before_idat=[trns]), want))
    got = decode_files(cases, tmp_path)
    for (name, _, want), g in zip(cases, got):
        assert np.array_equal(g, want), name
    for k in range(0, len(cases), 3):
        assert np.array_equal(got[k], got[k + 1]) and np.array_equal(got[k], got[k + 2])


def _split_idat(data):
    """the file with its one IDAT cut in two and a tEXt chunk between the halves"""
    pos = data.index(b"IDAT") - 4
    n = struct.unpack(">I", data[pos:pos + 4])[0]
    body = data[pos + 8:pos + 8 + n]
    return data[:pos] + pw.chunk(b"IDAT", body[:n // 2]) + pw.chunk(b"tEXt", b"k\0v") + pw.chunk(b"IDAT", body[n // 2:]) + data[pos + 12 + n:]


def hostile_files():
    """(name, file bytes, accepted?)"""
    rs = np.random.RandomState(17)
    s = pw.random_samples(rs, 6, 5, 2, 8)
    good = pw.write_png(s, 2, 8, filters=4)
    stream = pw.scanlines(s, 2, 8, 0, 4)
    idat = good.index(b"IDAT")
    idx = pw.random_samples(rs, 6, 5, 3, 8)
    bad_crc = bytearray(good)
    bad_crc[idat + 6] ^= 0x10  # inside the IDAT payload: its CRC no longer matches
    return [
        ("good", good, True),
        ("bad CRC in IDAT", bytes(bad_crc), False),
        ("bad CRC in IHDR", good[:20] + bytes([good[20] ^ 1]) + good[21:], False),
        ("filter byte 5", pw.write_png(s, 2, 8, filters=[4, 5, 1]), False),
        ("IDAT cut short", good[:idat + 10], False),
        ("file ends inside IDAT, chunk length intact", good[:len(good) - 12 - 6], False),
        ("one inflated byte too few", pw.write_png(s, 2, 8, stream=stream[:-1]), False),
        ("compression method 1", pw.write_png(s, 2, 8, header=pw.ihdr(5, 6, 8, 2, compression=1)), False),
        ("filter method 1", pw.write_png(s, 2, 8, header=pw.ihdr(5, 6, 8, 2, filter_method=1)), False),
        ("depth 3", pw.write_png(s, 2, 8, header=pw.ihdr(5, 6, 3, 0)), False),
        ("depth 4 for RGB", pw.write_png(s, 2, 8, header=pw.ihdr(5, 6, 4, 2)), False),
        ("palette image without PLTE", pw.write_png(idx, 3, 8), False),
        ("70000 x 70000 over a tiny body", pw.write_png(s, 2, 8, header=pw.ihdr(70000, 70000, 8, 2)), False),
        ("width 0", pw.write_png(s, 2, 8, header=pw.ihdr(0, 6, 8, 2)), False),
        ("no IEND", pw.write_png(s, 2, 8, iend=False), False),
        ("IDAT, another chunk, IDAT", _split_idat(good), False),
        ("unknown critical chunk", pw.write_png(s, 2, 8, ancillary=[pw.chunk(b"ABCD", b"x")]), False),
        ("bad CRC in an ancillary chunk", pw.write_png(s, 2, 8, filters=4, ancillary=[pw.chunk(b"gAMA", struct.pack(">I", 45455), crc_ok=False)]), True),
        ("unknown ancillary chunk", pw.write_png(s, 2, 8, filters=4, ancillary=[pw.chunk(b"abCd", b"xyz")]), True),
        ("surplus inflated bytes", pw.write_png(s, 2, 8, stream=stream + b"\x07" * 40), True),
    ]


def test_refusals_and_tolerances(tool, checker, tmp_path):
    """what refuses a file and what does not (png_decode.h's list), in the sanitizer build of the parser and through
    decode_tool; the accepted ones decode to the good file's pixels"""
    from PIL import Image
    files = hostile_files()
    verdicts = run_checker(checker, tmp_path, [f for _, f, _ in files])
    for (name, _, ok), v in zip(files, verdicts):
        assert v == ("A" if ok else "R"), name
    src = tmp_path / "good.png"
    src.write_bytes(files[0][1])
    subprocess.check_call([tool, str(src), str(tmp_path / "good.ppm")])
    want = np.array(Image.open(tmp_path / "good.ppm"))
    for i, (name, data, ok) in enumerate(files):
        src, out = tmp_path / ("h%02d.png" % i), tmp_path / ("h%02d.ppm" % i)
        src.write_bytes(data)
        r = subprocess.run([tool, str(src), str(out)], capture_output=True, text=True)
        assert (r.returncode == 0) == ok, (name, r.stderr[-500:])
        if ok:
            assert np.array_equal(np.array(Image.open(out)), want), name


def _repair_crcs(data):
    """the file with every chunk's CRC recomputed (so that a damaged byte reaches the code behind the CRC check)"""
    import zlib
    out, pos = bytearray(data[:8]), 8
    while pos + 12 <= len(data):
        n = struct.unpack(">I", data[pos:pos + 4])[0]
        if pos + 12 + n > len(data):
            break
        body = data[pos + 4:pos + 8 + n]
        out += data[pos:pos + 4] + body + struct.pack(">I", zlib.crc32(body) & 0xFFFFFFFF)
        pos += 12 + n
    return bytes(out + data[pos:])


def test_parser_under_sanitizers_on_damaged_files(checker, tmp_path):
    """every prefix of three small files, and seeded single-byte corruptions of them - as they are, and with the chunk CRCs
    repaired so that the damage reaches the header checks, the inflate and the unfiltering: each input is accepted or
    refused, and AddressSanitizer / UBSan have nothing to report (a report fails the run: stderr must stay empty)"""
    rs = np.random.RandomState(23)
    fixtures = [pw.write_png(pw.random_samples(rs, 7, 6, 6, 8), 6, 8, 1, MIXED[0], ancillary=[pw.chunk(b"gAMA", struct.pack(">I", 45455))], level=0),
                pw.write_png(pw.random_samples(rs, 9, 11, 3, 2), 3, 2, 0, MIXED[1], palette=rs.randint(0, 256, (3, 3)), idat_pieces=3),
                pw.write_png(pw.random_samples(rs, 5, 4, 0, 16), 0, 16, 1, 4, level=9)]
    inputs = []
    for f in fixtures:
        inputs += [f[:n] for n in range(len(f))]
        for _ in range(400):
            b = bytearray(f)
            b[rs.randint(8, len(b))] = rs.randint(0, 256)
            inputs.append(bytes(b))
            inputs.append(_repair_crcs(bytes(b)))
    verdicts = run_checker(checker, tmp_path, fixtures + inputs)
    assert verdicts[:3] == "AAA"
    assert "R" in verdicts and "A" in verdicts[3:]


def test_files_beyond_the_device_bounds_stay_on_the_host(tool, tmp_path):
    """a 1 x 70000 image with a None filter on every row would be 70000 segments of one row, and with Up on every row one
    segment of 1094 bands: both are beyond what the device stage takes (65536 segments, 16384 rows per pass), so the
    decoder finishes them on the host even where the device is asked for (--device), on any machine"""
    rs = np.random.RandomState(29)
    s = pw.random_samples(rs, 70000, 1, 0, 8)
    want = np.repeat(s.astype(np.uint8), 3, 2)
    for filters in (0, 2):
        stream = bytearray(70000 * 2)
        stream[0::2] = bytes([filters]) * 70000
        col = s[:, 0, 0].astype(np.int64)
        stream[1::2] = (col if filters == 0 else np.diff(col, prepend=0) & 0xFF).astype(np.uint8).tobytes()
        cases = [("1x70000 filter %d" % filters, pw.write_png(s, 0, 8, stream=bytes(stream)), want)]
        check_cases(cases, tmp_path, "--device")
