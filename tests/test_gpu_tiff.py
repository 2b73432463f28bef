"""TIFF requests, device half (csrc/kernels_tiff.hip through ocr_tiff_decode / ocr_pipe_stage_batch) and through the
service.  The yardstick is the host pixel stage, tiff::pixels of host/tiff_decode.h (run by host/tiff_check --pixels over the
same descriptors), which tests/test_tiff_decode.py pins against libtiff and Pillow; the numpy statement of the rules
(tests/tiff_writer.py convert) is asserted beside it.  Neither libtiff nor Pillow's TIFF reader is needed here."""
import base64
import io
import json
import math
import os
import shutil
import struct
import subprocess
import sys
import tempfile
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiff_writer as tw  # noqa: E402
from test_ipc_service import Client, _start  # noqa: E402
from test_raw_decode import TOOL, decode_files  # noqa: E402
from test_tiff_decode import HOST, build_check  # noqa: E402
from test_tiff_decode import test_descriptor_rules_are_refused_before_any_device_call as _descriptor_rules  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = [1, 3, 4, 5, 31, 32, 33, 65, 257]
HEIGHTS = [1, 2, 5]


@pytest.fixture(scope="module")
def tool(built):
    subprocess.check_call(["make", "-s", "-C", HOST])
    return TOOL


@pytest.fixture(scope="module")
def host_pixels(tmp_path_factory):
    """tiff::pixels over a list of descriptors: host/tiff_check.cpp --pixels, a plain host program"""
    d = tmp_path_factory.mktemp("tiffpixels")
    exe = build_check(d)

    def run(frames):
        src, out = d / "frames.bin", d / "pixels.bin"
        with open(src, "wb") as f:
            for fr in frames:
                f.write(struct.pack("<11i", fr["w"], fr["h"], fr["photometric"], fr["bits"], fr["samples"], fr["planar"], fr["predictor"],
                                    fr["big_endian"], fr["premultiply"], *fr["tile"]) + fr["palette"].tobytes() + struct.pack("<Q", len(fr["data"])) + fr["data"])
        subprocess.check_call([exe, "--pixels", str(src), str(out)])
        flat = np.fromfile(out, np.uint8)
        res, pos = [], 0
        for fr in frames:
            n = 3 * fr["w"] * fr["h"]
            res.append(flat[pos:pos + n].reshape(fr["h"], fr["w"], 3))
            pos += n
        assert pos == len(flat)
        return res

    return run


def make_frame(rs, form, w, h, planar=1, predictor=1, big_endian=False, tile=None, rows_per_strip=None, samples=None):
    """a descriptor (what tiff::parse would hand over) and the numpy model of its pixels"""
    name, photometric, bits, spp, extra = form
    if samples is None:
        samples, colormap = tw.random_case(rs, form, h, w)
    else:
        colormap = rs.randint(256, 65536, (3, 1 << bits)) if photometric == tw.PALETTE else None
    data, (tw_, th_) = tw.frame_data(samples, bits, planar=planar, predictor=predictor, tile=tile, rows_per_strip=rows_per_strip, big_endian=big_endian, rs=rs)
    palette = np.zeros((256, 4), np.uint8)
    if colormap is not None:
        palette[:1 << bits, :3] = tw.reduce_colormap(colormap)
    frame = dict(w=w, h=h, photometric=photometric, bits=bits, samples=spp, planar=planar if spp > 1 else 1, predictor=predictor, big_endian=int(big_endian),
                 premultiply=tw.premultiplies(photometric, planar, extra, spp), tile=(tw_, th_), palette=palette, data=data, name=name)
    return frame, tw.convert(samples, bits, photometric, planar, extra, colormap)


def device_decode(pkg, fr):
    return pkg.TiffFrame(fr["w"], fr["h"], fr["photometric"], fr["bits"], fr["samples"], fr["data"], tile=fr["tile"], planar=fr["planar"],
                         predictor=fr["predictor"], big_endian=fr["big_endian"], premultiply=fr["premultiply"], palette=fr["palette"]).decode()


def describe(fr):
    return {k: v for k, v in fr.items() if k not in ("data", "palette")}


def check_frames(pkg, host_pixels, frames_and_models):
    host = host_pixels([f for f, _ in frames_and_models])
    for (fr, model), ref in zip(frames_and_models, host):
        assert np.array_equal(ref, model), ("tiff::pixels differs from the numpy rules", describe(fr))
        got = device_decode(pkg, fr)
        assert np.array_equal(got, ref), (describe(fr), int((got != ref).sum()))


def planars(form):
    _, photometric, bits, spp, _ = form
    return (1, 2) if bits >= 8 and (photometric == tw.RGB or (photometric <= 1 and spp >= 2)) else (1,)


@pytest.mark.gpu
@pytest.mark.parametrize("form", tw.FORMS, ids=[f[0] for f in tw.FORMS])
def test_device_equals_host_pixel_stage(built, pkg, host_pixels, form):
    """ocr_tiff_decode == tiff::pixels byte for byte: widths {1, 3, 4, 5, 31, 32, 33, 65, 257} x heights {1, 2, 5} x RowsPerStrip
    {1, 2, above the height}, with predictor {off, on}, byte order {little, big} and planar {1, 2} taken in turn so that every
    combination in scope for the form occurs; then 16 x 16 and 32 x 16 tiles on 33 x 17 (clipped right and bottom tiles) with
    every such combination"""
    bits = form[2]
    rs = np.random.RandomState(300 + tw.FORMS.index(form))
    preds = (1, 2) if bits >= 8 else (1,)
    orders = (False, True) if bits == 16 else (False,)
    combos = [(pr, be, pl) for pr in preds for be in orders for pl in planars(form)]
    cases, k = [], 0
    for w in WIDTHS:
        for h in HEIGHTS:
            for rps in (1, 2, h + 3):
                pr, be, pl = combos[k % len(combos)]
                k += 1
                cases.append(make_frame(rs, form, w, h, planar=pl, predictor=pr, big_endian=be, rows_per_strip=rps))
    assert k >= 4 * len(combos)
    for tile in ((16, 16), (32, 16)):
        for pr, be, pl in combos:
            cases.append(make_frame(rs, form, 33, 17, planar=pl, predictor=pr, big_endian=be, tile=tile))
    check_frames(pkg, host_pixels, cases)


@pytest.mark.gpu
def test_the_scan_carries_across_spans_and_does_not_depend_on_the_split(built, pkg, host_pixels):
    """One row of 5000 pixels and two rows of 70 000 with the predictor on, 8- and 16-bit RGB: a row is 20 and 274 spans of a
    wave, the carry crosses every seam.  The same rows stored
    as one strip and as strips of one row give identical bytes.  9000 rows of 5 pixels in one-row strips: more units than the
    launch has waves (the grid stride)."""
    rs = np.random.RandomState(77)
    by_name = {f[0]: f for f in tw.FORMS}
    cases = []
    for name in ("rgb8", "rgb16"):
        form = by_name[name]
        for h, w in ((1, 5000), (2, 70000)):
            samples, _ = tw.random_case(rs, form, h, w)
            for rps in (h, 1):
                cases.append(make_frame(rs, form, w, h, predictor=2, big_endian=name == "rgb16" and h == 2, rows_per_strip=rps, samples=samples))
        cases.append(make_frame(rs, form, 5, 9000, predictor=2, rows_per_strip=1))
    cases.append(make_frame(rs, by_name["rgba16"], 2500, 3, predictor=2, planar=2, tile=(1024, 16)))
    cases.append(make_frame(rs, by_name["black1"], 2100, 3))
    check_frames(pkg, host_pixels, cases)
    for a, b in ((0, 1), (2, 3), (5, 6), (7, 8)):
        assert np.array_equal(device_decode(pkg, cases[a][0]), device_decode(pkg, cases[b][0]))


@pytest.mark.gpu
def test_descriptor_rules_reach_no_launch(built, pkg):
    """every descriptor rule -> OCR_ERR_ARG with its message (the CPU test, on the machine that could launch); a sound
    descriptor decodes"""
    _descriptor_rules(built, pkg)
    rs = np.random.RandomState(7)
    frame, model = make_frame(rs, tw.FORMS[15], 4, 5)
    assert np.array_equal(device_decode(pkg, frame), model)


def _jpeg(arr, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="JPEG", **kw)
    return buf.getvalue()


@pytest.mark.gpu
def test_one_stage_call_with_jpeg_png_raw_and_tiff_frames(tool, tmp_path):
    """One ocr_pipe_stage_batch call (decode_tool --stage) with a JPEG, a PNG, a raw frame and TIFFs of several forms - two
    paletted ones with different palettes, strips and tiles, 8 and 16 bits, a predictor: every ocr_pipe_slot_image equals the
    single decode of the same file.  The JPEG, PNG and raw images alone through ocr_pipe_stage_frames (--stage-frames) and
    through the new entry point leave the same bytes in the slot."""
    import png_writer as pw
    import raw_writer as rw
    rs = np.random.RandomState(43)
    by_name = {f[0]: f for f in tw.FORMS}
    rgb = rs.randint(0, 256, (53, 37, 3)).astype(np.uint8)
    s = pw.random_samples(rs, 53, 37, 6, 8)
    idx = rs.randint(0, 256, (53, 37))
    pal = rs.randint(0, 256, (256, 3))

    def tiff(name, h, w, **kw):
        form = by_name[name]
        samples, cm = tw.random_case(rs, form, h, w)
        return ("tiff " + name, tw.write_tiff(samples, form[2], form[1], extra=form[4], colormap=cm, rs=rs, **kw), tw.convert(samples, form[2], form[1], kw.get("planar", 1), form[4], cm))

    others = [("4:2:0 37x53", _jpeg(rgb, quality=90, subsampling=2), None),
              ("RGBA 8 interlaced 37x53", pw.write_png(s, 6, 8, 1, [3, 4, 0, 1, 2]), pw.expected_bgr(s, 6, 8)),
              ("bmp8 37x53", rw.write_bmp(idx, 8, palette=pal), rw.lookup(idx, pal))]
    tiffs = [tiff("rgb8", 53, 37, compression=tw.LZW, predictor=2, rows_per_strip=8), tiff("pal8", 53, 37, tile=(16, 16)), tiff("pal4", 17, 33, compression=tw.PACKBITS),
             tiff("rgba16", 53, 37, compression=tw.ADOBE_DEFLATE, predictor=2, big_endian=True, planar=2, tile=(32, 16)), tiff("white1", 70, 200),
             tiff("cmyk8", 53, 37), tiff("black16", 9000, 5, rows_per_strip=1)]
    cases = [tiffs[0], others[0], tiffs[1], others[1], tiffs[2], tiffs[3], others[2], tiffs[4], tiffs[5], tiffs[6]]
    models = os.path.join(ROOT, "models")
    host = decode_files(cases, tmp_path)
    single = decode_files(cases, tmp_path, "--device")
    staged = decode_files(cases, tmp_path, "--stage", models)
    for (name, _, want), a, b, c in zip(cases, staged, single, host):
        assert a.shape == b.shape and np.array_equal(a, b), name
        assert np.array_equal(a, c), name
        if want is not None:
            assert np.array_equal(a, want), name
    new = decode_files(others, tmp_path, "--stage", models)
    old = decode_files(others, tmp_path, "--stage-frames", models)
    for (name, _, _), a, b in zip(others, new, old):
        assert np.array_equal(a, b), name


@pytest.mark.gpu
def test_timing_entry_points_run(tool, tmp_path):
    """ocr_tiff_time (decode_tool --time <iters> <file>) and ocr_tiff_time_batch (... <batch>): OCR_OK and finite positive times"""
    rs = np.random.RandomState(51)
    src = tmp_path / "t.tif"
    src.write_bytes(tw.write_tiff(rs.randint(0, 256, (70, 200, 3)), 8, tw.RGB, compression=tw.LZW, predictor=2))
    for extra, batch in (([], 1), (["3"], 3)):
        r = subprocess.run([tool, "--time", "2", str(src)] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-1000:]
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        assert rec["batch"] == batch and rec["iters"] == 2 and rec["size"] == [70, 200] and rec["predictor"] == 2
        assert rec["bytes_in"] == 70 * 200 * 3 * batch and rec["bytes_out"] == 70 * 200 * 3 * batch
        for key in ("upload_ms", "pixel_stage_ms", "host_pixels_ms", "copy_ms"):
            assert math.isfinite(rec[key]) and rec[key] > 0, rec


def _same_reply(got, want):
    assert got["success"] is True and want["success"] is True, (got.get("error"), want.get("error"))
    assert got["width"] == want["width"] and got["height"] == want["height"]
    assert len(got["words"]) == len(want["words"])
    for g, w in zip(got["words"], want["words"]):
        assert g["box"] == w["box"] and g["text"] == w["text"] and g["confidence"] == w["confidence"]


@pytest.fixture(scope="module", params=["device", "host"])
def service(request, built):
    """the service with the TIFF pixel stage on the device (OCR_DEVICE_TIFF=1) and on the host (unset, the default)"""
    d = tempfile.mkdtemp(prefix="ocr", dir="/tmp")
    before = os.environ.get("OCR_DEVICE_TIFF")
    if request.param == "device":
        os.environ["OCR_DEVICE_TIFF"] = "1"
    else:
        os.environ.pop("OCR_DEVICE_TIFF", None)
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


def card_tiffs(card):
    """the test card (BGR) as TIFFs whose pixels ARE the card's, and as a PNG: {name: bytes}"""
    import png_writer as pw
    rgb = card[:, :, ::-1].astype(np.int64)
    h, w = rgb.shape[:2]
    rgba = np.concatenate([rgb, np.full((h, w, 1), 255)], 2)
    files = {"strips lzw predictor": tw.write_tiff(rgb, 8, tw.RGB, compression=tw.LZW, predictor=2, rows_per_strip=16),
             "tiles deflate big-endian": tw.write_tiff(rgb, 8, tw.RGB, big_endian=True, compression=tw.ADOBE_DEFLATE, predictor=2, tile=(64, 32)),
             "planes packbits opaque alpha": tw.write_tiff(rgba, 8, tw.RGB, compression=tw.PACKBITS, planar=2, extra=[2], rows_per_strip=50)}
    files["png"] = pw.write_png(rgba[:, :, :3].reshape(h, w, 3), 2, 8, 0, [0] * h)
    return files


@pytest.mark.gpu
def test_service_answers_tiffs_like_the_same_pixels_as_png(built, card, tmp_path, service):
    """TIFF `recognize` requests (image_path and base64): "success":true and the reply the same pixels get as a PNG"""
    c = Client(service)
    files = card_tiffs(card)
    paths = {}
    for name, data in files.items():
        p = tmp_path / (name.replace(" ", "_") + ".bin")
        p.write_bytes(data)
        paths[name] = str(p)
    want = c.call({"command": "recognize", "image_path": paths["png"]})
    assert want["success"] is True and (want["width"], want["height"]) == (card.shape[1], card.shape[0]) and len(want["words"]) > 0
    for name, data in files.items():
        if name == "png":
            continue
        _same_reply(c.call({"command": "recognize", "image_path": paths[name]}), want)
        if len(data) * 4 // 3 < 1000000:
            _same_reply(c.call({"command": "recognize", "image_data": base64.b64encode(data).decode()}), want)
    bad = tmp_path / "ccitt.tif"
    bad.write_bytes(tw.write_tiff(np.zeros((4, 4, 1), int), 1, tw.MINISWHITE, drop=(259,), more_tags=[(259, tw.SHORT, [4])]))
    reply = c.call({"command": "recognize", "image_path": str(bad)})
    assert reply["success"] is False and "Failed to" in reply["error"]  # (the answer an unreadable file got before)


@pytest.mark.gpu
def test_concurrent_clients_mix_tiff_and_the_other_formats(built, card, tmp_path, service):
    """Eight concurrent requests that mix the TIFFs with a PNG, a JPEG and a BMP (one batch: OCRWorker::processBatch ->
    ocr_pipe_stage_batch with OCR_DEVICE_TIFF=1; the host pixel path without): every reply equals the reply the same file
    gets alone"""
    import raw_writer as rw
    paths = []
    for name, data in card_tiffs(card).items():
        p = tmp_path / (name.replace(" ", "_") + ".bin")
        p.write_bytes(data)
        paths.append(str(p))
    for name, data in (("card.jpg", _jpeg(card[:, :, ::-1].copy(), quality=90, subsampling=2)), ("card.bmp", rw.write_bmp(card, 24))):
        p = tmp_path / name
        p.write_bytes(data)
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
