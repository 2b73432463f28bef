"""TIFF requests before the expansion, device half (csrc/kernels_tiff_lzw.hip through ocr_tiff_expand / ocr_tiff_decode_coded /
ocr_pipe_stage_batch) and through the service with OCR_DEVICE_TIFF=2.  The yardstick is the host's tiff::expand (run by
host/tiff_check --expand over the same coded frames), which tests/test_tiff_coded.py ties to tiff::parse and
tests/test_tiff_decode.py to libtiff.  Equality is exact."""
import base64
import json
import math
import os
import shutil
import struct
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiff_coded as tc  # noqa: E402
import tiff_writer as tw  # noqa: E402
from test_ipc_service import Client, _start  # noqa: E402
from test_raw_decode import TOOL, read_ppm  # noqa: E402
from test_tiff_decode import HOST, build_check  # noqa: E402
from test_tiff_coded import test_coded_rules_are_refused_before_any_device_call as _coded_rules  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BY_NAME = {f[0]: f for f in tw.FORMS}


@pytest.fixture(scope="module")
def tool(built):
    subprocess.check_call(["make", "-s", "-C", HOST])
    return TOOL


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """host/tiff_check.cpp, a plain host program: tiff::expand and tiff::pixels"""
    d = tmp_path_factory.mktemp("tiffexpand")
    return build_check(d), d


def check_expansion(pkg, checker, codeds, tag):
    exe, d = checker
    for c, ref in zip(codeds, tc.host_expand(exe, codeds, d, tag)):
        got = tc.to_pkg(pkg, c).expand(fill=0x5A)
        assert got.shape == ref.shape and np.array_equal(got, ref), (c.get("name"), len(ref), int((got != ref).sum()), np.nonzero(got != ref)[0][:4])


@pytest.mark.gpu
def test_hand_built_lzw_streams(built, pkg, checker):
    """one chunk each: code == next from the first possible code on (aaaa...), with period 2 and 3 (the overlapping copy), at
    1 .. 300 output bytes; strings longer than 64 and 128 bytes (the lane loop wraps); a clear in mid-stream; streams that cross
    511, 1023 and 2047 entries (random bytes of 600, 1400 and 3000) and one that fills the table and clears; the end code exactly
    at `need` and no end code at all; a surplus behind `need`; the last string cut by the chunk's end at every place"""
    rs = np.random.RandomState(21)
    cases = []

    def add(name, data, need=None, codes=None):
        stream = tc.pack_codes(codes if codes is not None else tc.lzw_codes(data))
        cases.append(dict(tc.grey_strip(stream, len(data) if need is None else need), name=name))

    for n in (1, 2, 3, 4, 5, 6, 63, 64, 65, 127, 128, 129, 299, 300):
        add("a x %d" % n, b"a" * n)
        add("ab x %d" % n, (b"ab" * n)[:n])
        add("abc x %d" % n, (b"abc" * n)[:n])
    add("a x 9000: strings up to 133 bytes", b"a" * 9000)
    add("ab x 20000: strings up to 200 bytes", b"ab" * 10000)
    part = rs.randint(0, 4, 150).astype(np.uint8).tobytes()
    add("a clear in mid-stream", part + part, codes=tc.lzw_codes(part, end=False) + tc.lzw_codes(part))
    for n in (600, 1400, 3000, 9000):
        add("random %d" % n, rs.randint(0, 256, n).astype(np.uint8).tobytes())
    text = (b"the quick brown fox jumps over the lazy dog. " * 7)[:300]
    add("no end code", text, codes=tc.lzw_codes(text, end=False))
    add("a surplus behind need", text, need=200)
    for need in range(280, 300):
        add("the last string cut at %d" % need, (b"ab" * 150), need=need)
        add("the last string cut at %d, period 1" % need, (b"a" * 300), need=need)
    check_expansion(pkg, checker, cases, "lzw")


@pytest.mark.gpu
def test_hand_built_packbits_streams(built, pkg, checker):
    """literal runs of 1 and 128, repeat runs of 2 and 128, -128 no-ops between and behind them, a repeat and a literal run cut by
    the chunk's end, a stream of 3000 bytes (the window in LDS is refilled), and stored chunks"""
    rs = np.random.RandomState(22)
    lit = rs.randint(0, 256, 128).astype(np.uint8).tobytes()
    streams = [("literal 1", b"\x00\x41", 1), ("literal 128", b"\x7f" + lit, 128), ("repeat 2", b"\xff\x42", 2), ("repeat 128", b"\x81\x43", 128),
               ("no-ops", b"\x80\x80\x00\x41\x80\xff\x42\x80\x7f" + lit + b"\x80\x81\x43\x80", 259), ("repeat cut", b"\x00\x41\x81\x43", 100),
               ("literal cut", b"\xff\x42\x7f" + lit, 71), ("literal cut by the stream's end and need", b"\x7f" + lit[:50], 50), ("surplus", b"\x81\x43\x81\x44", 128)]
    cases = [dict(tc.grey_strip(s, need, tw.PACKBITS), name=name) for name, s, need in streams]
    rows = np.repeat(rs.randint(0, 256, 3000), rs.randint(1, 6, 3000))[:3000].astype(np.uint8).tobytes()
    cases.append(dict(tc.grey_strip(tw.packbits_encode(rows, 3000), 3000, tw.PACKBITS), name="3000 bytes"))
    for n in (1, 15, 16, 17, 64, 65, 3000):
        cases.append(dict(tc.grey_strip(rows[:n], n, tw.NONE), name="stored %d" % n))
    check_expansion(pkg, checker, cases, "packbits")


def geometry_cases(rs):
    out = []
    for comp in (tw.LZW, tw.PACKBITS, tw.NONE):
        for w in (1, 3, 17, 257):
            out.append(("rgb8", 5, w, dict(compression=comp, rows_per_strip=2)))
        out.append(("rgb8", 9, 33, dict(compression=comp, rows_per_strip=8)))   # a last strip of 1 row
        out.append(("rgb8", 17, 33, dict(compression=comp, tile=(16, 16))))
        out.append(("rgba8", 17, 33, dict(compression=comp, planar=2, rows_per_strip=4)))
        out.append(("rgb16", 17, 33, dict(compression=comp, planar=2, tile=(16, 16), big_endian=True)))
        out.append(("black1", 9, 33, dict(compression=comp, rows_per_strip=8)))
        out.append(("pal4", 17, 33, dict(compression=comp, tile=(16, 16))))
    out.append(("rgb16", 9, 33, dict(compression=tw.LZW, predictor=2, big_endian=True, rows_per_strip=8)))
    out.append(("rgba16", 17, 33, dict(compression=tw.LZW, predictor=2, big_endian=True, planar=2, tile=(32, 16))))
    out.append(("rgb8", 9, 257, dict(compression=tw.LZW, predictor=2, rows_per_strip=8)))
    res = []
    for name, h, w, kw in out:
        form = BY_NAME[name]
        samples, cm = tw.random_case(rs, form, h, w)
        if name == "rgb8":  # (runs and repeats, so that LZW strings and PackBits repeats occur)
            samples = np.repeat(samples[:, :(w + 3) // 4], 4, 1)[:, :w]
        comp = kw.pop("compression")
        c, expanded = tc.make_coded(samples, form, comp, colormap=cm, rs=rs, **kw)
        c["name"] = "%s %dx%d %d %s" % (name, w, h, comp, kw)
        res.append((c, expanded, tw.convert(samples, form[2], form[1], kw.get("planar", 1), form[4], cm)))
    return res


@pytest.mark.gpu
def test_geometry(built, pkg, checker):
    """widths 1, 3, 17 and 257, a last strip of 1 row under 8 rows a strip (zero rows behind it), 16 x 16 tiles on 33 x 17, planar
    2, 16 bits big-endian with the predictor, 1-bit grey and a 4-bit palette, each with LZW, PackBits and stored chunks:
    ocr_tiff_expand == tiff::expand == the chunks the writer stored, and ocr_tiff_decode_coded == tiff::pixels == the numpy rules"""
    exe, d = checker
    cases = geometry_cases(np.random.RandomState(23))
    check_expansion(pkg, checker, [c for c, _, _ in cases], "geo")
    src, out = d / "frames.bin", d / "pixels.bin"
    with open(src, "wb") as f:
        for c, expanded, _ in cases:
            assert np.array_equal(tc.to_pkg(pkg, c).expand(), np.frombuffer(expanded, np.uint8)), c["name"]
            f.write(tc.head(c) + struct.pack("<Q", len(expanded)) + expanded)
    subprocess.check_call([exe, "--pixels", str(src), str(out)])
    flat, pos = np.fromfile(out, np.uint8), 0
    for c, _, model in cases:
        ref = flat[pos:pos + model.size].reshape(model.shape)
        pos += model.size
        assert np.array_equal(ref, model), ("tiff::pixels differs from the numpy rules", c["name"])
        got = tc.to_pkg(pkg, c).decode()
        assert np.array_equal(got, ref), (c["name"], int((got != ref).sum()))
    assert pos == len(flat)


@pytest.mark.gpu
def test_64_chunks_of_different_lengths_in_one_frame(built, pkg, checker):
    """64 strips whose streams run from a few bytes to the whole row, LZW and PackBits: one workgroup each, in one launch"""
    rs = np.random.RandomState(24)
    w = 700
    rows = np.zeros((64, w, 1), np.int64)
    for y in range(64):
        k = 1 + y * 11
        rows[y, :k, 0] = rs.randint(0, 256, k)
        rows[y, k:, 0] = y
    cases = []
    for comp in (tw.LZW, tw.PACKBITS):
        c, _ = tc.make_coded(rows, BY_NAME["black8"], comp, rows_per_strip=1)
        assert len(c["chunks"]) == 64 and len({k[1] for k in c["chunks"]}) > 40
        cases.append(dict(c, name="64 chunks %d" % comp))
    check_expansion(pkg, checker, cases, "many")


def _jpeg(arr, **kw):
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="JPEG", **kw)
    return buf.getvalue()


@pytest.mark.gpu
def test_one_stage_call_with_coded_tiffs_a_jpeg_and_a_png(tool, tmp_path):
    """One ocr_pipe_stage_batch call (decode_tool --stage) with 8 coded TIFF frames ("coded:<file>": OCR_FRAME_TIFF_CODED) of
    several forms and compressions, a JPEG and a PNG between them: every ocr_pipe_slot_image equals the =1 route's (the same
    files without the prefix: expanded on the host, OCR_FRAME_TIFF), the host decode and the numpy rules; --device under
    OCR_DEVICE_TIFF=2 (ocr_tiff_decode_coded) gives the same"""
    import png_writer as pw
    rs = np.random.RandomState(25)
    rgb = rs.randint(0, 256, (53, 37, 3)).astype(np.uint8)
    s = pw.random_samples(rs, 53, 37, 6, 8)

    def tiff(name, h, w, **kw):
        form = BY_NAME[name]
        samples, cm = tw.random_case(rs, form, h, w)
        return ("tiff " + name, tw.write_tiff(samples, form[2], form[1], extra=form[4], colormap=cm, rs=rs, **kw), tw.convert(samples, form[2], form[1], kw.get("planar", 1), form[4], cm), True)

    tiffs = [tiff("rgb8", 53, 37, compression=tw.LZW, predictor=2, rows_per_strip=8), tiff("pal8", 53, 37, compression=tw.LZW, tile=(16, 16)),
             tiff("pal4", 17, 33, compression=tw.PACKBITS), tiff("rgba16", 53, 37, compression=tw.LZW, predictor=2, big_endian=True, planar=2, tile=(32, 16)),
             tiff("white1", 70, 200, compression=tw.PACKBITS, rows_per_strip=16), tiff("cmyk8", 53, 37), tiff("black16", 300, 5, compression=tw.LZW, rows_per_strip=1),
             tiff("rgb8", 9, 257, compression=tw.LZW, fill_order=2, rows_per_strip=8)]
    others = [("4:2:0 37x53", _jpeg(rgb, quality=90, subsampling=2), None, False),
              ("RGBA 8 interlaced 37x53", pw.write_png(s, 6, 8, 1, [3, 4, 0, 1, 2]), pw.expected_bgr(s, 6, 8), False)]
    cases = tiffs[:3] + others[:1] + tiffs[3:6] + others[1:] + tiffs[6:]

    def run(flags, coded_prefix, env=None):
        args = []
        for i, (_, data, _, coded) in enumerate(cases):
            src = tmp_path / ("r%04d.bin" % i)
            src.write_bytes(data)
            args += [("coded:" if coded and coded_prefix else "") + str(src), str(tmp_path / ("r%04d.ppm" % i))]
        r = subprocess.run([TOOL, *flags] + args, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        return [read_ppm(tmp_path / ("r%04d.ppm" % i)) for i in range(len(cases))]

    models = os.path.join(ROOT, "models")
    host = run([], False, {"OCR_DEVICE_TIFF": "0"})
    coded = run(["--stage", models], True)
    plain = run(["--stage", models], False, {"OCR_DEVICE_TIFF": "1"})
    switched = run(["--stage", models], False, {"OCR_DEVICE_TIFF": "2"})
    single = run(["--device"], False, {"OCR_DEVICE_TIFF": "2"})
    for (name, _, want, _), a, b, c, d, e in zip(cases, coded, plain, host, switched, single):
        assert a.shape == b.shape and np.array_equal(a, b), name
        assert np.array_equal(a, c) and np.array_equal(a, d) and np.array_equal(a, e), name
        if want is not None:
            assert np.array_equal(a, want), name


@pytest.mark.gpu
def test_coded_rules_reach_no_launch(built, pkg):
    """every coded_fault rule -> OCR_ERR_ARG with its message and the output buffer untouched (the CPU test, on the machine that
    could launch); a sound frame decodes"""
    _coded_rules(built, pkg)
    samples = np.random.RandomState(7).randint(0, 256, (5, 4, 3))
    c, _ = tc.make_coded(samples, BY_NAME["rgb8"], tw.LZW, rows_per_strip=3)
    assert np.array_equal(tc.to_pkg(pkg, c).decode(), samples[:, :, ::-1])


@pytest.mark.gpu
def test_timing_entry_points_run(built, pkg, tool, tmp_path):
    """ocr_tiff_time_coded and ocr_tiff_time_coded_batch, through the binding and through decode_tool --time: three finite
    positive figures"""
    rs = np.random.RandomState(51)
    samples = np.repeat(rs.randint(0, 256, (70, 50, 3)), 4, 1)
    c, _ = tc.make_coded(samples, BY_NAME["rgb8"], tw.LZW, predictor=1, rows_per_strip=16)
    t = tc.to_pkg(pkg, c)
    for ms in (t.time(2), pkg.time_tiff_coded([t, t, t], 2)):
        assert len(ms) == 3 and all(math.isfinite(v) and v > 0 for v in ms), ms
    src = tmp_path / "t.tif"
    src.write_bytes(tw.write_tiff(samples, 8, tw.RGB, compression=tw.LZW, predictor=2, rows_per_strip=16))
    for extra, batch in (([], 1), (["3"], 3)):
        r = subprocess.run([tool, "--time", "2", str(src)] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-1000:]
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        assert rec["batch"] == batch and rec["compression"] == 5 and rec["chunks"] == 5 and rec["coded_bytes"] > 0
        for key in ("coded_upload_ms", "expand_stage_ms", "coded_pixel_stage_ms", "host_scan_ms_per_image", "host_expand_ms_per_image"):
            assert math.isfinite(rec[key]) and rec[key] > 0, rec


def _same_reply(got, want):
    assert got["success"] is True and want["success"] is True, (got.get("error"), want.get("error"))
    assert got["width"] == want["width"] and got["height"] == want["height"]
    assert len(got["words"]) == len(want["words"])
    for g, w in zip(got["words"], want["words"]):
        assert g["box"] == w["box"] and g["text"] == w["text"] and g["confidence"] == w["confidence"]


@pytest.fixture(scope="module")
def service(built):
    """the service with the TIFF expansion and pixel stage on the device (OCR_DEVICE_TIFF=2)"""
    d = tempfile.mkdtemp(prefix="ocr", dir="/tmp")
    before = os.environ.get("OCR_DEVICE_TIFF")
    os.environ["OCR_DEVICE_TIFF"] = "2"
    try:
        proc, sock = _start(d, 1)
    finally:
        if before is None:
            os.environ.pop("OCR_DEVICE_TIFF", None)
        else:
            os.environ["OCR_DEVICE_TIFF"] = before
    try:
        yield sock
        Client(sock).call({"command": "shutdown"})
        assert proc.wait(timeout=30) == 0
    finally:
        if proc.poll() is None:
            proc.kill()
        shutil.rmtree(d, ignore_errors=True)


@pytest.mark.gpu
def test_service_answers_coded_tiffs_like_the_same_pixels_as_png(built, card, tmp_path, service):
    """TIFF `recognize` requests under OCR_DEVICE_TIFF=2 - LZW strips, LZW tiles, PackBits planes and a Deflate file (which takes
    the =1 route) - by image_path and base64: "success":true and the reply the same pixels get as a PNG"""
    import png_writer as pw
    c = Client(service)
    rgb = card[:, :, ::-1].astype(np.int64)
    h, w = rgb.shape[:2]
    rgba = np.concatenate([rgb, np.full((h, w, 1), 255)], 2)
    files = {"strips lzw predictor": tw.write_tiff(rgb, 8, tw.RGB, compression=tw.LZW, predictor=2, rows_per_strip=16),
             "tiles lzw big-endian": tw.write_tiff(rgb, 8, tw.RGB, big_endian=True, compression=tw.LZW, predictor=2, tile=(64, 32)),
             "planes packbits opaque alpha": tw.write_tiff(rgba, 8, tw.RGB, compression=tw.PACKBITS, planar=2, extra=[2], rows_per_strip=50),
             "strips deflate": tw.write_tiff(rgb, 8, tw.RGB, compression=tw.ADOBE_DEFLATE, predictor=2, rows_per_strip=16),
             "png": pw.write_png(rgb.reshape(h, w, 3), 2, 8, 0, [0] * h)}
    paths = {}
    for name, data in files.items():
        p = tmp_path / (name.replace(" ", "_") + ".bin")
        p.write_bytes(data)
        paths[name] = str(p)
    want = c.call({"command": "recognize", "image_path": paths["png"]})
    assert want["success"] is True and (want["width"], want["height"]) == (w, h) and len(want["words"]) > 0
    for name, data in files.items():
        if name == "png":
            continue
        _same_reply(c.call({"command": "recognize", "image_path": paths[name]}), want)
        if len(data) * 4 // 3 < 1000000:
            _same_reply(c.call({"command": "recognize", "image_data": base64.b64encode(data).decode()}), want)
    bad = tmp_path / "short.tif"
    bad.write_bytes(tw.write_tiff(rgb[:8, :8], 8, tw.RGB, compression=tw.LZW, streams=[tw.lzw_encode(bytes(100))]))
    reply = c.call({"command": "recognize", "image_path": str(bad)})
    assert reply["success"] is False and "Failed to" in reply["error"]  # (a stream that ends early: found by the host's scan)
