"""EXIF orientation of JPEG requests on the host (host/jpeg_decode.h): cv::imdecode, which the reference decodes with, turns
the decoded image as tag 0x0112 of the file's Exif APP1 segment says.  Pinned to an independent implementation, Pillow's
ImageOps.exif_transpose on top of libjpeg-turbo's decode, bit for bit; a corpus of malformed segments decodes as stored; and
the marker parser runs under AddressSanitizer + UBSan as a stand-alone program over all of those files and over truncations.
The device half is tests/test_gpu_jpeg_orientation.py."""
import io
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cpp-paddle-ocr_amd", "host")
TOOL = os.path.join(HOST, "decode_tool")

SHORT, LONG = 3, 4


def jpeg_bytes(arr, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def pillow_exif_jpeg(arr, tag, **kw):
    """the JPEG as Pillow writes it with Orientation = tag"""
    from PIL import Image
    exif = Image.Exif()
    exif[0x0112] = tag
    return jpeg_bytes(arr, exif=exif, **kw)


def app1(payload):
    return b"\xff\xe1" + struct.pack(">H", len(payload) + 2) + payload


def exif_payload(order, entries, ifd_offset=8, count=None, pad=True, magic=42):
    """'Exif\\0\\0' + a TIFF header and IFD0 in byte order `order` ('II' / 'MM'); entries: (tag, type, count, value)"""
    e = "<" if order == "II" else ">"
    tiff = order.encode() + struct.pack(e + "HI", magic, ifd_offset)
    if pad:
        tiff += bytes(ifd_offset - 8)
    tiff += struct.pack(e + "H", len(entries) if count is None else count)
    for tag, typ, cnt, value in entries:
        field = struct.pack(e + "H", value) + b"\0\0" if typ == SHORT else struct.pack(e + "I", value)
        tiff += struct.pack(e + "HHI", tag, typ, cnt) + field
    tiff += struct.pack(e + "I", 0)  # no IFD1
    return b"Exif\0\0" + tiff


def with_segments(jpeg, *segments):
    assert jpeg[:2] == b"\xff\xd8"
    return jpeg[:2] + b"".join(segments) + jpeg[2:]


def hand_exif_jpeg(jpeg, order, tag):
    # a second entry in front of the orientation, and an IFD that does not start right after the header
    return with_segments(jpeg, app1(exif_payload(order, [(0x010F, SHORT, 1, 7), (0x0112, SHORT, 1, tag)], ifd_offset=12)))


def orient_np(a, tag):
    """the table of host/jpeg_decode.h on an array (rows, cols[, 3])"""
    t = (1, 0, 2)[:a.ndim]
    return {1: a, 2: a[:, ::-1], 3: a[::-1, ::-1], 4: a[::-1], 5: a.transpose(t), 6: a[::-1].transpose(t),
            7: a[::-1, ::-1].transpose(t), 8: a[:, ::-1].transpose(t)}[tag]


def pillow_oriented(data):
    from PIL import Image, ImageOps
    return np.array(ImageOps.exif_transpose(Image.open(io.BytesIO(data))).convert("RGB"))


def base_images(card):
    from PIL import Image
    noise = np.random.RandomState(11).randint(0, 256, (53, 37, 3)).astype(np.uint8)
    rgb = card[:, :, ::-1].copy()
    out = []
    for name, arr in (("noise", noise), ("card", rgb)):
        out.append((name + " 444", arr, dict(quality=90, subsampling=0)))
        out.append((name + " 420", arr, dict(quality=90, subsampling=2)))
        out.append((name + " grey", np.array(Image.fromarray(arr).convert("L")), dict(quality=90)))
    out.append(("card progressive", rgb, dict(quality=85, subsampling=2, progressive=True)))
    return out


def oriented_cases(card):
    """[(name, file bytes)]: tags 1..8, each as Pillow writes it and hand-assembled in both byte orders"""
    cases = []
    for name, arr, kw in base_images(card):
        plain = jpeg_bytes(arr, **kw)
        for tag in range(1, 9):
            cases.append(("%s tag %d pillow" % (name, tag), pillow_exif_jpeg(arr, tag, **kw)))
            for order in ("II", "MM"):
                cases.append(("%s tag %d %s" % (name, tag, order), hand_exif_jpeg(plain, order, tag)))
    return cases


def malformed_cases():
    """[(name, file bytes, orientation the decoder must use)] on one 53 x 37 4:2:0 image"""
    arr = np.random.RandomState(12).randint(0, 256, (53, 37, 3)).astype(np.uint8)
    plain = jpeg_bytes(arr, quality=90, subsampling=2)
    cases = []
    for order in ("II", "MM"):
        good = exif_payload(order, [(0x0112, SHORT, 1, 6)])
        bad = {
            "cut inside the IFD entry": good[:6 + 8 + 2 + 5],
            "cut inside the entry count": good[:6 + 8 + 1],
            "cut inside the TIFF header": good[:6 + 5],
            "IFD offset past the segment": exif_payload(order, [(0x0112, SHORT, 1, 6)], ifd_offset=1000, pad=False),
            "IFD offset 0xFFFFFFFF": exif_payload(order, [(0x0112, SHORT, 1, 6)], ifd_offset=0xFFFFFFFF, pad=False),
            "entry count larger than the segment": exif_payload(order, [(0x0112, SHORT, 1, 6)], count=200),
            "entry count 0xFFFF": exif_payload(order, [(0x0112, SHORT, 1, 6)], count=0xFFFF),
            "type LONG": exif_payload(order, [(0x0112, LONG, 1, 6)]),
            "count 2": exif_payload(order, [(0x0112, SHORT, 2, 6)]),
            "value 0": exif_payload(order, [(0x0112, SHORT, 1, 0)]),
            "value 9": exif_payload(order, [(0x0112, SHORT, 1, 9)]),
            "value 0xFFFF": exif_payload(order, [(0x0112, SHORT, 1, 0xFFFF)]),
            "tag absent": exif_payload(order, [(0x010F, SHORT, 1, 6)]),
            "magic 43": exif_payload(order, [(0x0112, SHORT, 1, 6)], magic=43),
            "byte order XX": good[:6] + b"XX" + good[8:],
        }
        for name, payload in bad.items():
            cases.append(("%s %s" % (order, name), with_segments(plain, app1(payload)), 1))
        xmp = app1(b"http://ns.adobe.com/xap/1.0/\0<x:xmpmeta xmlns:x='adobe:ns:meta/'/>")
        cases.append((order + " XMP first, Exif second", with_segments(plain, xmp, app1(good)), 6))
        cases.append((order + " two Exif segments", with_segments(plain, app1(exif_payload(order, [(0x0112, SHORT, 1, 8)])),
                                                                 app1(exif_payload(order, [(0x0112, SHORT, 1, 3)]))), 8))
    return plain, cases


def run_tool(data, tmp_path, *flags):
    from PIL import Image
    src, dst = tmp_path / "t.jpg", tmp_path / "t.ppm"
    src.write_bytes(data)
    r = subprocess.run([TOOL, *flags, str(src), str(dst)], capture_output=True, text=True)
    return r, (np.array(Image.open(dst)) if r.returncode == 0 else None)


def test_orientation_table_is_pillows():
    """the numpy form of the table used below == Pillow's transposes (no JPEG involved)"""
    from PIL import Image, ImageOps
    a = np.random.RandomState(1).randint(0, 256, (5, 9, 3)).astype(np.uint8)
    for tag in range(1, 9):
        im = Image.fromarray(a)
        exif = im.getexif()
        exif[0x0112] = tag
        buf = io.BytesIO()
        im.save(buf, format="PNG", exif=exif)
        got = np.array(ImageOps.exif_transpose(Image.open(io.BytesIO(buf.getvalue()))).convert("RGB"))
        assert np.array_equal(got, orient_np(a, tag)), tag


def test_host_decode_applies_exif_orientation(built, card, tmp_path):
    """Tags 1..8 in both byte orders, 53 x 37 noise and the card, 4:4:4 / 4:2:0 / grey and one progressive file, through
    decode_tool (Decoder::decode): equal to ImageOps.exif_transpose of Pillow's decode, bit for bit.  (Without the feature
    tags 5..8 differ by shape alone.)"""
    subprocess.check_call(["make", "-s", "-C", HOST])
    cases = oriented_cases(card)
    orders = set()
    for name, data in cases:
        orders.add(data[data.index(b"Exif\0\0") + 6:][:2])
        want = pillow_oriented(data)
        r, got = run_tool(data, tmp_path)
        assert r.returncode == 0, (name, r.stderr)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        assert np.array_equal(got, want), name
    assert orders == {b"II", b"MM"}
    # the transform is applied to the finished stored pixel: upsampling stays in the stored frame
    arr = base_images(card)[1][1]
    plain = jpeg_bytes(arr, quality=90, subsampling=2)
    from PIL import Image
    stored = np.array(Image.open(io.BytesIO(plain)).convert("RGB"))
    for tag in range(1, 9):
        r, got = run_tool(hand_exif_jpeg(plain, "II", tag), tmp_path)
        assert r.returncode == 0 and np.array_equal(got, orient_np(stored, tag)), tag


def test_host_pixel_path_from_coefficients_applies_orientation(built, card, tmp_path):
    """Decoder::pixels (what a worker's materialise() runs when a JPEG batch is finished on the host) turns the image
    too: a stand-alone program decodes coefficients, then pixels, and writes them."""
    exe = _build_probe(tmp_path, sanitize=False)
    arr = base_images(card)[1][1]
    plain = jpeg_bytes(arr, quality=90, subsampling=2)
    for tag in (1, 3, 6, 8):
        data = hand_exif_jpeg(plain, "MM", tag)
        src, dst = tmp_path / "p.jpg", tmp_path / "p.rgb"
        src.write_bytes(data)
        out = subprocess.run([exe, "--pixels", str(dst), str(src)], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        _, orientation, ok, rows, cols = out.stdout.split()[-5:]
        assert int(orientation) == tag and ok == "1"
        want = pillow_oriented(data)
        got = np.frombuffer(dst.read_bytes(), np.uint8).reshape(int(rows), int(cols), 3)[:, :, ::-1]
        assert got.shape == want.shape and np.array_equal(got, want), tag


def test_malformed_exif_decodes_as_stored(built, tmp_path):
    """Truncated segments, offsets and counts that leave the segment, other types / counts / values, XMP: the image
    decodes as stored with exit status 0 (libjpeg ignores the marker).  The first Exif APP1 is the one that counts."""
    from PIL import Image
    subprocess.check_call(["make", "-s", "-C", HOST])
    plain, cases = malformed_cases()
    stored = np.array(Image.open(io.BytesIO(plain)).convert("RGB"))
    for name, data, tag in cases:
        r, got = run_tool(data, tmp_path)
        assert r.returncode == 0, (name, r.stderr)
        assert got.shape == orient_np(stored, tag).shape and np.array_equal(got, orient_np(stored, tag)), name


PROBE = r"""
// every file named on the command line through the JPEG decoder: the marker parser, the whole decode and the
// coefficient / pixel split.  Prints "<file> <orientation> <decoded 0|1> <rows> <cols>" per file.
#include <cstdio>
#include <cstring>
#include <vector>
#include "jpeg_decode.h"
int main(int argc, char** argv) {
  const char* dump = nullptr;
  int first = 1;
  if (argc > 3 && !strcmp(argv[1], "--pixels")) { dump = argv[2]; first = 3; }
  for (int i = first; i < argc; ++i) {
    FILE* f = fopen(argv[i], "rb");
    if (!f) return 2;
    std::vector<uint8_t> raw;
    uint8_t buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) raw.insert(raw.end(), buf, buf + n);
    fclose(f);
    // an allocation of exactly the file's size: a read past the end is a report, not a read of vector slack
    uint8_t* exact = new uint8_t[raw.size() ? raw.size() : 1];
    if (!raw.empty()) memcpy(exact, raw.data(), raw.size());
    std::vector<uint8_t> bgr, bgr2;
    int rows = 0, cols = 0, rows2 = 0, cols2 = 0;
    PaddleOCR::jpeg::Decoder whole, half;
    const bool ok = whole.decode(exact, raw.size(), bgr, rows, cols);
    PaddleOCR::jpeg::Coefs c;
    const bool ok2 = half.decode_coefficients(exact, raw.size(), c) && PaddleOCR::jpeg::Decoder::pixels(c, bgr2, rows2, cols2);
    delete[] exact;
    if (ok != ok2 || (ok && (rows != rows2 || cols != cols2 || bgr != bgr2))) { fprintf(stderr, "%s: the two paths differ\n", argv[i]); return 3; }
    if (ok && (rows != c.out_rows() || cols != c.out_cols())) return 4;
    printf("%s %d %d %d %d\n", argv[i], ok2 ? c.orientation : 0, (int)ok, rows, cols);
    if (dump && ok) { FILE* o = fopen(dump, "wb"); if (!o) return 2; fwrite(bgr2.data(), 1, bgr2.size(), o); fclose(o); }
  }
  return 0;
}
"""


def _build_probe(tmp_path, sanitize):
    src, exe = tmp_path / "exif_probe.cpp", tmp_path / ("exif_probe_san" if sanitize else "exif_probe")
    src.write_text(PROBE)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover", "-g", "-O1"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", *flags, "-I", HOST, str(src), "-o", str(exe)])
    return str(exe)


def test_parser_under_sanitizers(card, tmp_path):
    """The marker parser reads bytes from the network.  A stand-alone program that includes only host/jpeg_decode.h, built
    with AddressSanitizer + UBSan (no recovery), decodes every file of the tests above and every prefix of the first 200
    bytes of an Exif JPEG (each from an allocation of exactly its size): exit 0, no report, and the orientations the
    tests above expect."""
    exe = _build_probe(tmp_path, sanitize=True)
    files, want = [], []

    def add(data, orientation):
        p = tmp_path / ("f%04d.jpg" % len(files))
        p.write_bytes(data)
        files.append(str(p))
        want.append(orientation)

    for name, data in oriented_cases(card):
        add(data, int(name.split(" tag ")[1].split()[0]))
    _, bad = malformed_cases()
    for name, data, tag in bad:
        add(data, tag)
    arr = np.random.RandomState(13).randint(0, 256, (16, 24, 3)).astype(np.uint8)
    whole = hand_exif_jpeg(jpeg_bytes(arr, quality=90, subsampling=2), "MM", 6)
    assert whole.index(b"\xff\xda") > 200   # the prefixes end inside the headers: in APP1, in the IFD, in the tables
    for n in range(201):
        add(whole[:n], None)
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([exe] + files, capture_output=True, text=True, env=env)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(files)
    for line, f, o in zip(lines, files, want):
        _, orientation, ok, rows, cols = line.rsplit(" ", 4)
        if o is None:
            assert ok == "0", line      # a file cut in its headers is refused, not crashed on
        else:
            assert ok == "1" and int(orientation) == o, (line, o)
