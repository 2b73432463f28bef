"""PNG requests, device half (csrc/kernels_png.hip through ocr_png_decode / ocr_pipe_stage_frames) and through the service.
Same case table and expectation as the host half, tests/test_png_decode.py: the pixels that cv::imdecode's conversion
rules give for the samples the file was written from, byte for byte."""
import base64
import io
import os
import shutil
import subprocess
import sys
import tempfile
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_writer as pw  # noqa: E402
from test_ipc_service import Client, _start  # noqa: E402
from test_png_decode import FILTER_CHOICES, HOST, MIXED, TOOL, check_cases, decode_files, make_case  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (width, height): 1x1, 3x2, 5x9 - Adam7 passes without pixels; 7x65, 33x130 - a segment crosses one and two band
# boundaries (kPngBand = 64 rows; the later bands take 63), the row above comes from memory; 200x70 - wider than the LDS
# store tile (kPngTile = 64 units), ragged last tile
SIZES = [(1, 1), (3, 2), (5, 9), (7, 65), (33, 130), (200, 70)]
# one (colour type, depth) per kernel instantiation (bpp 1, 2, 3, 4, 6, 8) and per conversion inside it
KINDS = [(0, 1), (3, 4), (0, 8), (0, 16), (4, 8), (2, 8), (6, 8), (4, 16), (2, 16), (6, 16)]


@pytest.fixture(scope="module")
def tool(built):
    subprocess.check_call(["make", "-s", "-C", HOST])
    return TOOL


@pytest.mark.gpu
def test_device_decode_against_construction(tool, tmp_path):
    """ocr_png_decode (decode_tool --device) == the construction, on all 15 (type, depth) pairs x interlace x the five
    filters and the two mixed patterns over the sizes above; and every kernel instantiation at the band- and
    tile-crossing sizes with all-Paeth rows (no None / Sub row after the first: ONE segment), a None row every third row
    (many short segments) and a mixed pattern"""
    rs = np.random.RandomState(3)
    cases, k = [], 0
    for ct, depth in pw.LEGAL:
        for interlace in (0, 1):
            for filters in FILTER_CHOICES:
                w, h = SIZES[k % len(SIZES)]
                k += 1
                cases.append(make_case(rs, h, w, ct, depth, interlace, filters))
    for ct, depth in KINDS:
        for interlace in (0, 1):
            for w, h in SIZES[3:]:
                for filters in (4, [0, 4, 3], MIXED[0]):
                    cases.append(make_case(rs, h, w, ct, depth, interlace, filters))
    check_cases(cases, tmp_path, "--device")


@pytest.mark.gpu
def test_device_equals_host_pixel_stage_on_random_files(tool, tmp_path):
    """200 seeded random files (type, depth, interlace, size up to 96 x 150, a random filter on every row, random
    samples): the device pixel stage == the host pixel stage of png_decode.h, and both == the construction"""
    rs = np.random.RandomState(2024)
    cases = []
    for _ in range(200):
        ct, depth = pw.LEGAL[rs.randint(len(pw.LEGAL))]
        w, h = int(rs.randint(1, 97)), int(rs.randint(1, 151))
        kinds = rs.randint(0, 5, 151).tolist()
        cases.append(make_case(rs, h, w, ct, depth, int(rs.randint(2)), lambda p, r, kinds=kinds: kinds[(r + 3 * p) % len(kinds)],
                               name="random type %d depth %d %dx%d" % (ct, depth, w, h)))
    dev = decode_files(cases, tmp_path, "--device")
    host = decode_files(cases, tmp_path, env={"OCR_DEVICE_PNG": "0"})
    for (name, _, want), a, b in zip(cases, dev, host):
        assert a.shape == b.shape and np.array_equal(a, b), name
        assert np.array_equal(a, want), name


def _segments(stream, height, width, ct, depth, interlace):
    """the segment table of a scanline stream, as png_decode.h scan() cuts it"""
    bits = pw.CHANNELS[ct] * depth
    segs, pos = [], 0
    for pi, (x0, y0, dx, dy) in enumerate(p for p in (pw.ADAM7 if interlace else [(0, 0, 1, 1)])):
        cols = (width - x0 + dx - 1) // dx if width > x0 else 0
        rows = (height - y0 + dy - 1) // dy if height > y0 else 0
        if not cols or not rows:
            continue
        rowbytes = (cols * bits + 7) // 8
        for r in range(rows):
            if r == 0 or stream[pos] <= 1:
                segs.append([pi, r, 1])
            else:
                segs[-1][2] += 1
            pos += 1 + rowbytes
    assert pos == len(stream)
    return [tuple(s) for s in segs]


@pytest.mark.gpu
def test_descriptor_validation(built, pkg):
    """ocr_png_frame is checked field by field on the host before anything is launched: a sound descriptor decodes to the
    construction; the same descriptor with its length short by one, with a filter byte 7, with a segment table that skips
    a row, starts a segment at a row that needs the row above, or claims another size is OCR_ERR_ARG with a message"""
    rs = np.random.RandomState(9)
    h, w, ct, depth = 70, 21, 6, 8
    s = pw.random_samples(rs, h, w, ct, depth)
    stream = pw.scanlines(s, ct, depth, 0, [1, 4, 3, 2, 0, 4, 4])
    segs = _segments(stream, h, w, ct, depth, 0)
    assert len(segs) > 4

    def frame(stream=stream, segs=segs, **kw):
        return pkg.PngFrame(kw.get("w", w), kw.get("h", h), depth, ct, 0, stream, segs)

    assert np.array_equal(frame().decode(), pw.expected_bgr(s, ct, depth))

    def refused(f, what):
        with pytest.raises(pkg.OcrError, match=what) as e:
            f.decode()
        assert e.value.code == -1  # OCR_ERR_ARG

    f = frame()
    f.c.data_len -= 1
    refused(f, "data_len")
    refused(frame(stream=stream + b"\0"), "data_len")
    bad = bytearray(stream)
    bad[3 * (1 + 4 * w)] = 7
    refused(frame(stream=bytes(bad)), "filter byte")
    skip = list(segs)
    skip[2] = (0, skip[2][1] + 1, skip[2][2] - 1) if skip[2][2] > 1 else (0, skip[2][1] + 1, 1)
    refused(frame(segs=skip), "tile the rows|cover every row")
    refused(frame(segs=segs[:-1]), "cover every row")
    refused(frame(segs=segs + [(0, h, 1)]), "beyond the last row")
    split = [(0, 0, 2), (0, 2, h - 2)]  # row 2 is Average here: it needs row 1
    refused(frame(segs=split), "needs the row above")
    refused(frame(w=w + 1), "data_len")
    f = frame()
    f.c.bit_depth = 3
    refused(f, "bit depth")
    f = frame()
    f.c.width, f.c.height = 70000, 70000
    refused(f, "64 Mpixel")
    f = frame()
    f.c.segments = None
    refused(f, "segment table")


@pytest.mark.gpu
def test_one_stage_call_with_jpeg_and_png_frames(tool, tmp_path):
    """One ocr_pipe_stage_frames call (decode_tool --stage) with two JPEG frames and three PNG frames of different bpp
    kinds, two of the images of one size and not adjacent: every staged image, read back with ocr_pipe_slot_image, equals
    the bytes the single-image calls (ocr_jpeg_decode*, ocr_png_decode) give - for the PNGs, the construction"""
    from PIL import Image
    rs = np.random.RandomState(41)

    def jpeg(arr, **kw):
        buf = io.BytesIO()
        Image.fromarray(arr).save(buf, format="JPEG", **kw)
        return buf.getvalue()

    rgb = rs.randint(0, 256, (53, 37, 3)).astype(np.uint8)
    cases = [make_case(rs, 53, 37, 6, 8, 1, MIXED[0], name="RGBA 8 interlaced 37x53"),
             ("4:2:0 37x53", jpeg(rgb, quality=90, subsampling=2), None),
             make_case(rs, 130, 33, 3, 2, 0, [0, 4, 3], name="palette 2 33x130"),
             ("grey 5x17", jpeg(np.array(Image.fromarray(rgb[:17, :5]).convert("L")), quality=90), None),
             make_case(rs, 70, 200, 2, 16, 0, 4, name="RGB 16 200x70")]
    each = decode_files(cases, tmp_path, "--device")
    staged = decode_files(cases, tmp_path, "--stage", os.path.join(ROOT, "models"))
    for (name, _, want), a, b in zip(cases, staged, each):
        assert a.shape == b.shape and np.array_equal(a, b), name
        if want is not None:
            assert np.array_equal(a, want), name


@pytest.mark.gpu
def test_timing_entry_points_run(tool, tmp_path):
    """ocr_png_time (decode_tool --time <iters> <png>) and ocr_png_time_batch (... <batch>): OCR_OK, and finite positive
    times for the upload and for the pixel stage"""
    import json
    import math
    rs = np.random.RandomState(51)
    src = tmp_path / "t.png"
    src.write_bytes(make_case(rs, 70, 200, 6, 8, 0, MIXED[0])[1])
    for extra, batch in (([], 1), (["3"], 3)):
        r = subprocess.run([tool, "--time", "2", str(src)] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-1000:]
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        assert rec["batch"] == batch and rec["iters"] == 2 and rec["size"] == [70, 200]
        for key in ("upload_ms", "pixel_stage_ms"):
            assert math.isfinite(rec[key]) and rec[key] > 0, rec


def _ppm_bytes(bgr):
    return b"P6\n%d %d\n255\n" % (bgr.shape[1], bgr.shape[0]) + np.ascontiguousarray(bgr[:, :, ::-1]).tobytes()


def _same_reply(got, want):
    assert got["success"] is True and want["success"] is True, (got.get("error"), want.get("error"))
    assert got["width"] == want["width"] and got["height"] == want["height"]
    assert len(got["words"]) == len(want["words"])
    for g, w in zip(got["words"], want["words"]):
        assert g["box"] == w["box"] and g["text"] == w["text"] and g["confidence"] == w["confidence"]


def card_pngs(card):
    """{name: (file bytes, expected BGR)}: the card as RGB, as RGBA with a translucent band, through a palette, and as an
    interlaced 16-bit file whose low bytes are noise"""
    from PIL import Image
    rs = np.random.RandomState(77)
    rgb = card[:, :, ::-1].astype(np.uint16)
    h, w = rgb.shape[:2]
    adaptive = lambda p, r: (1, 2, 4, 3, 4, 4, 0)[(r * 7 + p) % 7]  # noqa: E731
    alpha = np.full((h, w, 1), 255, np.uint16)
    alpha[h // 3:h // 2] = 128
    alpha[:4] = 0
    rgba = np.concatenate([rgb, alpha], 2)
    pim = Image.fromarray(rgb.astype(np.uint8)).quantize(200)
    pal = np.array(pim.getpalette()[:600]).reshape(-1, 3)
    idx = np.array(pim).astype(np.uint16)[:, :, None]
    deep = (rgb << 8) | rs.randint(0, 256, rgb.shape).astype(np.uint16)
    return {"rgb": (pw.write_png(rgb, 2, 8, 0, adaptive), pw.expected_bgr(rgb, 2, 8)),
            "rgba": (pw.write_png(rgba, 6, 8, 0, adaptive), pw.expected_bgr(rgba, 6, 8)),
            "palette": (pw.write_png(idx, 3, 8, 0, adaptive, palette=pal), pw.expected_bgr(idx, 3, 8, pal)),
            "rgb16 interlaced": (pw.write_png(deep, 2, 16, 1, adaptive), pw.expected_bgr(deep, 2, 16))}


@pytest.fixture(scope="module", params=["device", "host"])
def service(request, built):
    """the service with the PNG pixel stage on the device (OCR_DEVICE_PNG=1) and on the host (=0, the default)"""
    d = tempfile.mkdtemp(prefix="ocr", dir="/tmp")
    before = os.environ.get("OCR_DEVICE_PNG")
    os.environ["OCR_DEVICE_PNG"] = "1" if request.param == "device" else "0"
    try:
        proc, sock = _start(d, 1)
    finally:
        if before is None:
            os.environ.pop("OCR_DEVICE_PNG", None)
        else:
            os.environ["OCR_DEVICE_PNG"] = before
    try:
        yield sock
        Client(sock).call({"command": "shutdown"})
        assert proc.wait(timeout=30) == 0
    finally:
        if proc.poll() is None:
            proc.kill()
        shutil.rmtree(d, ignore_errors=True)


@pytest.mark.gpu
def test_service_answers_png_requests_like_their_pixels(built, card, tmp_path, service):
    """The card as RGB, RGBA with a translucent band, palette and interlaced 16-bit PNG, as image_path and as base64: each
    reply equals the reply to a PPM request that carries exactly the expected pixels (which for the card are the card)"""
    c = Client(service)
    found_words = False
    for name, (data, want_bgr) in card_pngs(card).items():
        if name != "palette":
            assert np.array_equal(want_bgr, card), name
        ppm, png = tmp_path / "want.ppm", tmp_path / (name.replace(" ", "_") + ".png")
        ppm.write_bytes(_ppm_bytes(want_bgr))
        png.write_bytes(data)
        want = c.call({"command": "recognize", "image_path": str(ppm)})
        assert want["success"] is True and (want["width"], want["height"]) == (card.shape[1], card.shape[0])
        found_words = found_words or len(want["words"]) > 0
        _same_reply(c.call({"command": "recognize", "image_path": str(png)}), want)
        if len(data) * 4 // 3 < 1000000:
            _same_reply(c.call({"command": "recognize", "image_data": base64.b64encode(data).decode()}), want)
    assert found_words


@pytest.mark.gpu
def test_concurrent_clients_mix_png_and_jpeg(built, card, tmp_path, service):
    """Eight concurrent requests that mix the four PNG files with two JPEG files (one batch on the device:
    OCRWorker::processBatch -> ocr_pipe_stage_frames): every reply equals the reply the same file gets alone"""
    from PIL import Image
    paths = []
    for name, (data, _) in card_pngs(card).items():
        p = tmp_path / (name.replace(" ", "_") + ".png")
        p.write_bytes(data)
        paths.append(str(p))
    for name, kw in (("420", dict(quality=90, subsampling=2)), ("444", dict(quality=92, subsampling=0))):
        buf = io.BytesIO()
        Image.fromarray(card[:, :, ::-1].copy()).save(buf, format="JPEG", **kw)
        p = tmp_path / (name + ".jpg")
        p.write_bytes(buf.getvalue())
        paths.append(str(p))
    c0 = Client(service)
    alone = [c0.call({"command": "recognize", "image_path": p}) for p in paths]
    assert all(a["success"] for a in alone) and len(alone[0]["words"]) > 0
    nthreads = 8
    out = [None] * nthreads
    go = threading.Barrier(nthreads)

    def work(t):
        c = Client(service)
        go.wait(timeout=60)  # connected clients send together: the worker finds the others queued behind the first request
        k = t % len(paths)
        out[t] = (k, c.call({"command": "recognize", "image_path": paths[k]}))

    th = [threading.Thread(target=work, args=(t,)) for t in range(nthreads)]
    [t.start() for t in th]
    [t.join() for t in th]
    for t in range(nthreads):
        k, got = out[t]
        _same_reply(got, alone[k])
