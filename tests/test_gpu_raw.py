"""BMP and PNM requests, device half (csrc/kernels_raw.hip through ocr_raw_decode / ocr_pipe_stage_frames) and through
the service.  The yardstick is the host pixel stage, raw::pixels of host/raw_decode.h (run by host/raw_check --pixels over
the same descriptors), which tests/test_raw_decode.py pins against files written sample by sample; the numpy statement of
the rules (tests/raw_writer.py convert_rows) is asserted beside it."""
import base64
import io
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
import raw_writer as rw  # noqa: E402
from test_ipc_service import Client, _start  # noqa: E402
from test_raw_decode import HOST, TOOL, card_files, check_cases, decode_files  # noqa: E402
from test_raw_decode import test_descriptor_rules_are_refused_before_any_device_call as _descriptor_rules  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = [1, 3, 4, 5, 31, 32, 33, 65, 257]
HEIGHTS = [1, 2, 5]


@pytest.fixture(scope="module")
def tool(built):
    subprocess.check_call(["make", "-s", "-C", HOST])
    return TOOL


@pytest.fixture(scope="module")
def host_pixels(tmp_path_factory):
    """raw::pixels over a list of descriptors: host/raw_check.cpp --pixels, a plain host program"""
    d = tmp_path_factory.mktemp("rawpixels")
    exe = str(d / "raw_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(HOST, "raw_check.cpp")])

    def run(frames):
        """frames: [(w, h, kind, bottom_up, stride, palette (256, 4), rows bytes)] -> [(h, w, 3) BGR]"""
        src, out = d / "frames.bin", d / "pixels.bin"
        with open(src, "wb") as f:
            for w, h, kind, bu, stride, pal, rows in frames:
                f.write(struct.pack("<iiiiQ", w, h, kind, bu, stride) + np.asarray(pal, np.uint8).tobytes() + struct.pack("<Q", len(rows)) + rows)
        subprocess.check_call([exe, "--pixels", str(src), str(out)])
        flat = np.fromfile(out, np.uint8)
        res, pos = [], 0
        for w, h, *_ in frames:
            res.append(flat[pos:pos + 3 * w * h].reshape(h, w, 3))
            pos += 3 * w * h
        assert pos == len(flat)
        return res

    return run


def make_frame(rs, kind, w, h, bottom_up, pad):
    rb = rw.row_bytes(kind, w)
    stride = rb + pad
    rows = rs.randint(0, 256, (h, stride)).astype(np.uint8)
    pal = rs.randint(0, 256, (256, 4)).astype(np.uint8)
    data = rows.tobytes()
    if pad:
        data = data[:len(data) - pad]  # the last row may lack its padding: data_len is exactly what the descriptor needs
    return (w, h, kind, bottom_up, stride, pal, data), rw.convert_rows(kind, rows, w, pal, bottom_up)


def check_frames(pkg, host_pixels, frames_and_models):
    frames = [f for f, _ in frames_and_models]
    host = host_pixels(frames)
    for (frame, model), ref in zip(frames_and_models, host):
        w, h, kind, bu, stride, pal, data = frame
        assert np.array_equal(ref, model), ("raw::pixels differs from the numpy rules", rw.KINDS[kind], w, h, bu, stride)
        got = pkg.RawFrame(w, h, kind, bu, stride, data, pal).decode()
        assert np.array_equal(got, ref), (rw.KINDS[kind], w, h, bu, stride, int((got != ref).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", range(len(rw.KINDS)), ids=rw.KINDS)
def test_device_equals_host_pixel_stage(built, pkg, host_pixels, kind):
    """ocr_raw_decode == raw::pixels byte for byte at widths {1, 3, 4, 5, 31, 32, 33, 65, 257} x heights {1, 2, 5}, both row
    orders, row_stride exact and padded (by 1, 2, 3 and 7 bytes in turn: every alignment of a row start)"""
    rs = np.random.RandomState(100 + kind)
    cases, k = [], 0
    for w in WIDTHS:
        for h in HEIGHTS:
            for bottom_up in (0, 1):
                cases.append(make_frame(rs, kind, w, h, bottom_up, 0))
                cases.append(make_frame(rs, kind, w, h, bottom_up, (1, 2, 3, 7)[k % 4]))
                k += 1
    check_frames(pkg, host_pixels, cases)


@pytest.mark.gpu
def test_rows_wider_than_a_workgroup_and_more_units_than_the_grid(built, pkg, host_pixels):
    """300 x 200 of each kind; 2100 x 3 (a workgroup owns 1024 pixels of a row: three spans, the last ragged) and 5 x 9000
    (more units than the launch has workgroups: the grid stride) of each kind"""
    rs = np.random.RandomState(200)
    cases = []
    for kind in range(len(rw.KINDS)):
        cases.append(make_frame(rs, kind, 300, 200, kind % 2, 0))
        cases.append(make_frame(rs, kind, 2100, 3, 1 - kind % 2, 1))
        cases.append(make_frame(rs, kind, 5, 9000, kind % 2, 0))
    check_frames(pkg, host_pixels, cases)


@pytest.mark.gpu
def test_descriptor_rules_reach_no_launch(built, pkg):
    """every descriptor rule -> OCR_ERR_ARG with its message (the CPU test, on the machine that could launch); a sound
    descriptor decodes"""
    _descriptor_rules(built, pkg)
    rs = np.random.RandomState(7)
    frame, model = make_frame(rs, 5, 4, 5, 1, 0)
    assert np.array_equal(pkg.RawFrame(*frame[:5], frame[6], frame[5]).decode(), model)


def _jpeg(arr, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="JPEG", **kw)
    return buf.getvalue()


@pytest.mark.gpu
def test_one_stage_call_with_jpeg_png_and_raw_frames(tool, tmp_path):
    """One ocr_pipe_stage_frames call (decode_tool --stage) with a JPEG frame, a PNG frame and raw frames of different kinds -
    two paletted ones with different palettes, so that a workgroup's palette changes inside a launch, and a 5 x 9000 one whose
    units outnumber the grid: every ocr_pipe_slot_image equals the host decode of the same file"""
    import png_writer as pw
    rs = np.random.RandomState(41)
    rgb = rs.randint(0, 256, (53, 37, 3)).astype(np.uint8)
    s = pw.random_samples(rs, 53, 37, 6, 8)
    idx = rs.randint(0, 256, (53, 37))
    pal1, pal2 = rs.randint(0, 256, (256, 3)), rs.randint(0, 256, (256, 3))
    tall = rs.randint(0, 256, (9000, 5))
    grey16 = rs.randint(0, 65536, (17, 5, 1))
    bits = rs.randint(0, 2, (70, 200, 1))
    cases = [("bmp8 37x53", rw.write_bmp(idx, 8, palette=pal1), rw.lookup(idx, pal1)),
             ("4:2:0 37x53", _jpeg(rgb, quality=90, subsampling=2), None),
             ("P4 200x70", rw.write_pnm(4, bits), rw.expected_pnm(4, bits)),
             ("RGBA 8 interlaced 37x53", pw.write_png(s, 6, 8, 1, [3, 4, 0, 1, 2]), pw.expected_bgr(s, 6, 8)),
             ("bmp8 tall 5x9000", rw.write_bmp(tall, 8, palette=pal2, top_down=True), rw.lookup(tall, pal2)),
             ("P5 16-bit 5x17", rw.write_pnm(5, grey16, 65535), rw.expected_pnm(5, grey16, 65535)),
             ("bmp24 37x53", rw.write_bmp(rgb, 24), rgb)]
    host = decode_files(cases, tmp_path)
    staged = decode_files(cases, tmp_path, "--stage", os.path.join(ROOT, "models"))
    for (name, _, want), a, b in zip(cases, staged, host):
        assert a.shape == b.shape and np.array_equal(a, b), name
        if want is not None:
            assert np.array_equal(a, want), name


@pytest.mark.gpu
def test_device_decode_of_files(tool, tmp_path):
    """decode_tool --device (ocr_raw_decode behind the container parser) on run-length, ASCII and 16-bit files"""
    from test_raw_decode import bmp_matrix, pnm_matrix, rle_cases
    check_cases(bmp_matrix(seed=21)[::2] + pnm_matrix(seed=22)[::2] + rle_cases(seed=23)[::4], tmp_path, "--device")


@pytest.mark.gpu
def test_timing_entry_points_run(tool, tmp_path):
    """ocr_raw_time (decode_tool --time <iters> <file>) and ocr_raw_time_batch (... <batch>): OCR_OK and finite positive times"""
    import json
    import math
    rs = np.random.RandomState(51)
    src = tmp_path / "t.bmp"
    src.write_bytes(rw.write_bmp(rs.randint(0, 256, (70, 200)), 8, palette=rs.randint(0, 256, (256, 3))))
    for extra, batch in (([], 1), (["3"], 3)):
        r = subprocess.run([tool, "--time", "2", str(src)] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-1000:]
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        assert rec["batch"] == batch and rec["iters"] == 2 and rec["size"] == [70, 200] and rec["kind"] == 2
        for key in ("upload_ms", "pixel_stage_ms", "host_pixels_ms"):
            assert math.isfinite(rec[key]) and rec[key] > 0, rec


def _same_reply(got, want):
    assert got["success"] is True and want["success"] is True, (got.get("error"), want.get("error"))
    assert got["width"] == want["width"] and got["height"] == want["height"]
    assert len(got["words"]) == len(want["words"])
    for g, w in zip(got["words"], want["words"]):
        assert g["box"] == w["box"] and g["text"] == w["text"] and g["confidence"] == w["confidence"]


@pytest.fixture(scope="module", params=["device", "host"])
def service(request, built):
    """the service with the BMP / PNM pixel stage on the device (OCR_DEVICE_RAW=1) and on the host (unset, the default)"""
    d = tempfile.mkdtemp(prefix="ocr", dir="/tmp")
    before = os.environ.get("OCR_DEVICE_RAW")
    if request.param == "device":
        os.environ["OCR_DEVICE_RAW"] = "1"
    else:
        os.environ.pop("OCR_DEVICE_RAW", None)
    try:
        proc, sock = _start(d, 1)
    finally:
        if before is None:
            os.environ.pop("OCR_DEVICE_RAW", None)
        else:
            os.environ["OCR_DEVICE_RAW"] = before
    try:
        yield sock
        Client(sock).call({"command": "shutdown"})
        assert proc.wait(timeout=30) == 0
    finally:
        if proc.poll() is None:
            proc.kill()
        shutil.rmtree(d, ignore_errors=True)


@pytest.mark.gpu
def test_service_answers_paletted_bmp_and_p5_like_the_same_picture_as_bmp24(built, card, tmp_path, service):
    """an 8-bit paletted BMP and a P5 file as `recognize` requests (image_path and base64): "success":true, and the words
    of the same picture sent as a 24-bit BMP"""
    c = Client(service)
    files = card_files(card)
    paths = {}
    for name, (data, _) in files.items():
        p = tmp_path / (name.replace(" ", "_") + ".bin")
        p.write_bytes(data)
        paths[name] = str(p)
    found_words = False
    for name in ("bmp8", "p5"):
        want = c.call({"command": "recognize", "image_path": paths[name + " as bmp24"]})
        assert want["success"] is True and (want["width"], want["height"]) == (card.shape[1], card.shape[0])
        found_words = found_words or len(want["words"]) > 0
        _same_reply(c.call({"command": "recognize", "image_path": paths[name]}), want)
        data = files[name][0]
        if len(data) * 4 // 3 < 1000000:
            _same_reply(c.call({"command": "recognize", "image_data": base64.b64encode(data).decode()}), want)
    assert found_words


@pytest.mark.gpu
def test_concurrent_clients_mix_raw_and_jpeg(built, card, tmp_path, service):
    """Eight concurrent requests that mix the BMP / PNM files with two JPEGs (one batch: OCRWorker::processBatch ->
    ocr_pipe_stage_frames with OCR_DEVICE_RAW=1 - the JPEGs stay on the device decode; the host pixel path without): every
    reply equals the reply the same file gets alone"""
    from PIL import Image
    paths = []
    for name, (data, _) in card_files(card).items():
        p = tmp_path / (name.replace(" ", "_") + ".bin")
        p.write_bytes(data)
        paths.append(str(p))
    for ext, kw in (("420.jpg", dict(quality=90, subsampling=2)), ("444.jpg", dict(quality=92, subsampling=0))):
        buf = io.BytesIO()
        Image.fromarray(card[:, :, ::-1].copy()).save(buf, format="JPEG", **kw)
        p = tmp_path / ("card" + ext)
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
