"""JPEG requests beyond grey / YCbCr 4:4:4, 4:2:2, 4:2:0 on the host (host/jpeg_decode.h): every integral sampling on
every component, CMYK / YCCK, Adobe RGB.  The arbiter is Pillow (libjpeg-turbo) on the same bytes, bit for bit; 4-component
files are compared after OpenCV's CMYK -> BGR rule on libjpeg's raw samples (Pillow hands CMYK out inverted, raw mode
CMYK;I).  Most files come from tests/jpeg_writer.py, since Pillow cannot write them; Pillow files relabelled to another
sampling cross-check that writer.  The device half is tests/test_gpu_jpeg_formats.py, which shares the case table."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_writer as jw  # noqa: E402
from test_jpeg_orientation import HOST, TOOL, SHORT, app1, exif_payload, orient_np, with_segments  # noqa: E402

# (Y, Cb, Cr) sampling factors (h, v)
FAMILIES = {
    "1x2,1x1,1x1": [(1, 2), (1, 1), (1, 1)],   # 4:4:0: fancy h1v2
    "4x1,1x1,1x1": [(4, 1), (1, 1), (1, 1)],   # 4:1:1: box 4x1
    "1x4,1x1,1x1": [(1, 4), (1, 1), (1, 1)],
    "2x2,1x2,1x2": [(2, 2), (1, 2), (1, 2)],   # chroma h2v1 under a 2x2 luma
    "2x2,2x1,2x1": [(2, 2), (2, 1), (2, 1)],   # chroma h1v2 under a 2x2 luma
    "2x1,1x1,2x1": [(2, 1), (1, 1), (2, 1)],   # Cb and Cr differ
    "1x1,2x2,2x2": [(1, 1), (2, 2), (2, 2)],   # subsampled luma
    "3x1,1x1,1x1": [(3, 1), (1, 1), (1, 1)],
    "3x2,1x1,1x1": [(3, 2), (1, 1), (1, 1)],
    "4x2,1x1,1x1": [(4, 2), (1, 1), (1, 1)],
}
SIZES = [(1, 1), (2, 1), (1, 2), (3, 130), (53, 37), (17, 5)]


def planes(rows, cols, n, seed=0):
    """n smooth-plus-noise planes: interpolation and replication differ on them everywhere"""
    rs = np.random.RandomState(seed + 131 * rows + cols)
    yy, xx = np.mgrid[0:rows, 0:cols]
    return [np.clip(128 + 60 * np.sin(xx / 3.0 + i) + 50 * np.cos(yy / 2.5 + 2 * i) + rs.randint(-20, 20, (rows, cols)), 0, 255).astype(np.uint8)
            for i in range(n)]


def exif(tag):
    return app1(exif_payload("MM", [(0x0112, SHORT, 1, tag)]))


def expected_rgb(data, tag=1):
    """Pillow's decode of the bytes as the service must see it (RGB order, as decode_tool writes its PPM), turned by `tag`"""
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    if im.mode == "CMYK":
        raw = 255 - np.array(im).astype(np.int32)                 # libjpeg's samples: Pillow inverts what it hands out
        k = raw[..., 3:4]
        rgb = (k - (((255 - raw[..., :3]) * k) >> 8)).astype(np.uint8)  # icvCvt_CMYK2BGR_8u_C4C3R, per channel
    else:
        rgb = np.array(im.convert("RGB"))
    return np.ascontiguousarray(orient_np(rgb, tag))


def narrow_sizes(factors):
    """9-row images whose most expanded component is 1, 2 and 3 samples wide: where jdsample.c leaves its fancy forms"""
    hmax = max(h for h, _ in factors)
    e = max(hmax // h for h, _ in factors)
    return [(9, e * k) for k in (1, 2, 3)]


def pillow_bytes(arr, mode=None, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr, mode).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def relabelled():
    rs = np.random.RandomState(5)
    wide, tall = rs.randint(0, 256, (48, 64, 3)).astype(np.uint8), rs.randint(0, 256, (64, 48, 3)).astype(np.uint8)
    return [("4:2:2 relabelled 4:4:0", jw.relabel(pillow_bytes(wide, quality=90, subsampling=1), 0x21, 0x12, True)),
            ("4:2:0 relabelled 4:1:1", jw.relabel(pillow_bytes(wide, quality=90, subsampling=2), 0x22, 0x41, False)),
            ("4:2:0 relabelled 1x4", jw.relabel(pillow_bytes(tall, quality=90, subsampling=2), 0x22, 0x14, False))]


def case_table():
    """{group: [(name, file bytes, EXIF tag)]}; one decode_tool process per group"""
    table = {}
    for name, f in FAMILIES.items():
        table[name] = [("%s %dx%d" % (name, r, c), jw.write_jpeg(planes(r, c, 3), f, jfif=True), 1) for r, c in SIZES + narrow_sizes(f)]
    f440, f411 = FAMILIES["1x2,1x1,1x1"], FAMILIES["4x1,1x1,1x1"]
    table["scans"] = [("restart interval", jw.write_jpeg(planes(53, 37, 3), f440, jfif=True, restart=3), 1),
                      ("per-component scans", jw.write_jpeg(planes(53, 37, 3), f411, jfif=True, interleaved=False), 1)]
    cmyk = np.stack(planes(53, 37, 4), -1)
    luma_k = [(2, 2), (1, 1), (1, 1), (2, 2)]
    table["four components"] = [
        ("Pillow CMYK baseline", pillow_bytes(cmyk, "CMYK", quality=90), 1),
        ("Pillow CMYK progressive", pillow_bytes(cmyk, "CMYK", quality=90, progressive=True), 1),
        ("CMYK without a marker", jw.write_jpeg(planes(53, 37, 4), [(1, 1)] * 4), 1),
        ("CMYK Adobe transform 0, K at luma's factors", jw.write_jpeg(planes(53, 37, 4), luma_k, adobe=0), 1),
        ("YCCK Adobe transform 2, K at luma's factors", jw.write_jpeg(planes(53, 37, 4), luma_k, adobe=2), 1),
        ("YCCK 17x5", jw.write_jpeg(planes(17, 5, 4), luma_k, adobe=2), 1),
        ("4 components Adobe transform 1 (libjpeg: YCCK)", jw.write_jpeg(planes(17, 20, 4), [(2, 1), (1, 1), (1, 1), (2, 1)], adobe=1), 1)]
    table["three components, colour space"] = [
        ("Adobe transform 0 RGB", jw.write_jpeg(planes(53, 37, 3), [(1, 1)] * 3, adobe=0), 1),
        ("Adobe transform 0 RGB 2x1", jw.write_jpeg(planes(17, 20, 3), [(2, 1), (1, 1), (1, 1)], adobe=0), 1),
        ("Adobe transform 1 YCbCr", jw.write_jpeg(planes(17, 20, 3), [(1, 1)] * 3, adobe=1), 1),
        ("JFIF wins over Adobe transform 0", jw.write_jpeg(planes(17, 20, 3), [(1, 1)] * 3, jfif=True, adobe=0), 1),
        ("ids R G B without a marker", jw.write_jpeg(planes(53, 37, 3), [(1, 1)] * 3, ids=b"RGB"), 1),
        ("ids 1 2 3 without a marker", jw.write_jpeg(planes(17, 20, 3), [(2, 1), (1, 1), (1, 1)]), 1),
        ("grey with factors 2x2 written", jw.write_jpeg(planes(17, 20, 1), [(2, 2)]), 1)]
    table["relabelled Pillow files"] = [(n, d, 1) for n, d in relabelled()]
    turned = []
    for tag in (3, 6, 8):
        turned.append(("4:4:0 tag %d" % tag, jw.write_jpeg(planes(53, 37, 3), f440, jfif=True, segments=[exif(tag)]), tag))
        turned.append(("4:1:1 tag %d" % tag, jw.write_jpeg(planes(53, 37, 3), f411, jfif=True, segments=[exif(tag)]), tag))
        turned.append(("CMYK tag %d" % tag, with_segments(pillow_bytes(cmyk, "CMYK", quality=90), exif(tag)), tag))
    table["orientation"] = turned
    return table


GROUPS = list(FAMILIES) + ["scans", "four components", "three components, colour space", "relabelled Pillow files", "orientation"]


@pytest.fixture(scope="module")
def table():
    t = case_table()
    assert list(t) == GROUPS
    return t


def decode_group(cases, tmp_path, *flags):
    """all files of a group through one decode_tool process; [(name, decoded RGB array)]"""
    from PIL import Image
    args = []
    for i, (_, data, _) in enumerate(cases):
        src = tmp_path / ("c%03d.jpg" % i)
        src.write_bytes(data)
        args += [str(src), str(tmp_path / ("c%03d.ppm" % i))]
    r = subprocess.run([TOOL, *flags] + args, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return [(name, np.array(Image.open(tmp_path / ("c%03d.ppm" % i)))) for i, (name, _, _) in enumerate(cases)]


def check_group(cases, tmp_path, *flags):
    for (name, got), (_, data, tag) in zip(decode_group(cases, tmp_path, *flags), cases):
        want = expected_rgb(data, tag)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        assert np.array_equal(got, want), (name, int(np.abs(got.astype(int) - want).max()))


def test_writer_tables_are_annex_k():
    """the Huffman tables typed into jpeg_writer.py are the ones libjpeg writes by default"""
    data = pillow_bytes(np.zeros((8, 8, 3), np.uint8))
    for tc, th, (bits, vals) in ((0, 0, jw.DC_TABLES[0]), (1, 0, jw.AC_TABLES[0]), (0, 1, jw.DC_TABLES[1]), (1, 1, jw.AC_TABLES[1])):
        assert sum(bits) == len(vals)
        assert bytes([(tc << 4) | th]) + bytes(bits) + bytes(vals) in data, (tc, th)


def test_pillow_decodes_the_writers_files_as_labelled(table):
    """the expectation itself: Pillow opens every file of the table with the size and mode the writer meant, fancy h1v2 for
    4:4:0 (not replication) and replication for 4:1:1"""
    from PIL import Image
    for group, cases in table.items():
        for name, data, _ in cases:
            im = Image.open(io.BytesIO(data))
            im.load()
            assert im.mode in ("RGB", "CMYK", "L"), name

    def ycc(data):  # libjpeg's upsampled components, without a colour conversion
        im = Image.open(io.BytesIO(data))
        im.draft("YCbCr", im.size)
        assert im.mode == "YCbCr"
        return np.array(im)

    ramp = np.arange(0, 256, 8, dtype=np.uint8)
    up = ycc(jw.write_jpeg([np.tile(ramp[:, None], (1, 32))] * 3, FAMILIES["1x2,1x1,1x1"], quality=100, jfif=True))
    assert (up[2:-2:2, 0, 1] != up[3:-2:2, 0, 1]).all()                   # 4:4:0: the two rows of a pair differ (triangle filter)
    up = ycc(jw.write_jpeg([np.tile(ramp[None, :], (32, 1))] * 3, FAMILIES["4x1,1x1,1x1"], quality=100, jfif=True))
    assert (up[0, :, 1].reshape(8, 4) == up[0, ::4, 1][:, None]).all()    # 4:1:1: four equal chroma samples in a row
    assert len(set(up[0, ::4, 1].tolist())) == 8


@pytest.mark.parametrize("group", GROUPS)
def test_host_decode_equals_pillow(built, table, tmp_path, group):
    """decode_tool in host mode (Decoder::decode) on every file of the group == Pillow's decode (4 components: OpenCV's
    CMYK -> BGR on libjpeg's samples), oriented files against the numpy transpose of that expectation.  Without the feature
    every one of these files is refused."""
    subprocess.check_call(["make", "-s", "-C", HOST])
    check_group(table[group], tmp_path)


def test_refusals(built, tmp_path):
    """what libjpeg refuses is refused: exit status 1 (decode failed), no crash - and Pillow refuses the same bytes"""
    from PIL import Image
    subprocess.check_call(["make", "-s", "-C", HOST])
    bad = {"fractional expansion (3x1 luma, 2x1 Cb)": jw.write_jpeg(planes(17, 20, 3), [(3, 1), (2, 1), (1, 1)], jfif=True),
           "2 components": jw.write_jpeg(planes(17, 20, 2), [(1, 1)] * 2),
           "12 blocks per MCU": jw.write_jpeg(planes(17, 20, 3), [(4, 2), (2, 1), (2, 1)], jfif=True),
           "5 components": jw.write_jpeg(planes(17, 20, 5), [(1, 1)] * 5),
           "sampling factor 5": jw.write_jpeg(planes(17, 20, 3), [(5, 1), (1, 1), (1, 1)], jfif=True)}
    for name, data in bad.items():
        src = tmp_path / "bad.jpg"
        src.write_bytes(data)
        r = subprocess.run([TOOL, str(src), str(tmp_path / "bad.ppm")], capture_output=True, text=True)
        assert r.returncode == 1 and "decode failed" in r.stderr, (name, r.returncode, r.stderr)
        with pytest.raises(Exception):
            Image.open(io.BytesIO(data)).load()


PROBE = r"""
// a corpus file of [u32 little-endian length][bytes] records through the JPEG decoder, each record from an allocation of
// exactly its size: the whole decode and the coefficient / pixel split must agree.  Prints "ok" or "refused" per record.
#include <cstdio>
#include <cstring>
#include <vector>
#include "jpeg_decode.h"
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  for (;;) {
    uint8_t l[4];
    if (fread(l, 1, 4, f) != 4) break;
    const size_t n = (size_t)l[0] | ((size_t)l[1] << 8) | ((size_t)l[2] << 16) | ((size_t)l[3] << 24);
    uint8_t* exact = new uint8_t[n ? n : 1];
    if (n && fread(exact, 1, n, f) != n) return 2;
    std::vector<uint8_t> bgr, bgr2;
    int rows = 0, cols = 0, rows2 = 0, cols2 = 0;
    PaddleOCR::jpeg::Decoder whole, half;
    const bool ok = whole.decode(exact, n, bgr, rows, cols);
    PaddleOCR::jpeg::Coefs c;
    const bool ok2 = half.decode_coefficients(exact, n, c) && PaddleOCR::jpeg::Decoder::pixels(c, bgr2, rows2, cols2);
    delete[] exact;
    if (ok != ok2 || (ok && (rows != rows2 || cols != cols2 || bgr != bgr2))) { fprintf(stderr, "the two paths differ\n"); return 3; }
    puts(ok ? "ok" : "refused");
  }
  fclose(f);
  return 0;
}
"""


def test_hostile_bytes_under_sanitizers(tmp_path):
    """The decoder parses network bytes.  A stand-alone program that includes only host/jpeg_decode.h, built with
    AddressSanitizer + UBSan (no recovery), decodes three small files of the new kinds cut at every 7th byte and with each
    of their first 700 bytes inverted, one at a time: every run ends in "ok" or "refused", no report, no read past the
    buffer (each record sits in an allocation of exactly its size)."""
    src, exe = tmp_path / "formats_probe.cpp", tmp_path / "formats_probe"
    src.write_text(PROBE)
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-g", "-O1", "-I", HOST, str(src), "-o", str(exe)])
    files = [jw.write_jpeg(planes(24, 16, 3), FAMILIES["1x2,1x1,1x1"], jfif=True, segments=[exif(6)]),
             jw.write_jpeg(planes(24, 16, 4), [(2, 2), (1, 1), (1, 1), (2, 2)], adobe=2, restart=1),
             pillow_bytes(np.stack(planes(24, 16, 4), -1), "CMYK", quality=75, progressive=True)]
    records = []
    for data in files:
        records.append(data)
        records += [data[:n] for n in range(0, len(data), 7)]
        for i in range(min(700, len(data))):
            b = bytearray(data)
            b[i] ^= 0xFF
            records.append(bytes(b))
    corpus = tmp_path / "corpus.bin"
    corpus.write_bytes(b"".join(len(r).to_bytes(4, "little") + r for r in records))
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([str(exe), str(corpus)], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
    lines = r.stdout.split()
    assert len(lines) == len(records) and set(lines) <= {"ok", "refused"}
    whole = [i for i, rec in enumerate(records) if rec in files]
    assert all(lines[i] == "ok" for i in whole) and "refused" in lines
