"""Lossy WebP requests, device half (csrc/kernels_vp8.hip through ocr_vp8_decode / ocr_pipe_stage_batch) and through the
service.  The yardstick is the host pixel stage, vp8::pixels of host/vp8_decode.h (run by host/vp8_check --pixels over the same
descriptors), which tests/test_vp8_decode.py pins against libwebp on the golden files and on 315 streams of tests/vp8_writer.py.  Neither libwebp nor Pillow's WebP
support is needed here."""
import base64
import glob
import io
import json
import math
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vp8_frames as vf  # noqa: E402
from test_ipc_service import Client, _start  # noqa: E402
from test_raw_decode import TOOL, decode_files  # noqa: E402
from test_vp8_decode import test_descriptor_rules_are_refused_before_any_device_call as _descriptor_rules  # noqa: E402

ROOT = vf.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "webp_lossy")
PRED = ["i16_%d" % m for m in range(4)] + ["b_%d" % m for m in range(10)] + ["mix"]
FILT = ["none", "simple", "normal1", "normal63", "sharp7", "deltas"]
COEF = ["skipped", "dc", "dense", "extreme"]


@pytest.fixture(scope="module")
def tool(built):
    subprocess.check_call(["make", "-s", "-C", vf.HOST])
    return TOOL


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("vp8pixels")
    return d, vf.build_check(d)


def device_decode(pkg, fr):
    return pkg.Vp8Frame(fr["width"], fr["height"], fr["filter_type"], fr["mbs"], fr["coeffs"]).decode()


def check_frames(pkg, checker, frames, names):
    d, exe = checker
    for fr, want, name in zip(frames, vf.host_pixels(exe, d, frames), names):
        got = device_decode(pkg, fr)
        assert got.shape == want.shape and np.array_equal(got, want), (name, fr["width"], fr["height"])


@pytest.mark.gpu
@pytest.mark.parametrize("pred", PRED)
def test_device_equals_host_pixels_per_prediction_form(built, pkg, checker, pred):
    """ocr_vp8_decode == vp8::pixels byte for byte over random descriptors of every width x height of the grid (macroblock grids
    1 x 1 .. 17 x 4: diagonals shorter than, equal to and longer than the workgroup's waves, a single column, a single row),
    with this prediction form and the filter and coefficient forms going round"""
    rs = np.random.RandomState(PRED.index(pred))
    frames, names, k = [], [], 0
    for w in vf.WIDTHS:
        for h in vf.HEIGHTS:
            filt, coef = FILT[k % len(FILT)], COEF[(k // len(FILT) + k) % len(COEF)]
            frames.append(vf.random_frame(rs, w, h, pred, filt, coef))
            names.append((pred, filt, coef))
            k += 1
    frames.append(vf.random_frame(rs, 33, 257, pred, FILT[k % len(FILT)], "dense"))  # 17 rows: a diagonal longer than the workgroup's waves
    names.append((pred, "tall"))
    check_frames(pkg, checker, frames, names)


@pytest.mark.gpu
@pytest.mark.parametrize("filt", FILT)
def test_device_equals_host_pixels_per_filter_form(built, pkg, checker, filt):
    """the same with this filter form over every coefficient form, on the grids where a filtered edge has neighbours on every
    side, one row and one column"""
    rs = np.random.RandomState(100 + FILT.index(filt))
    frames, names = [], []
    for (w, h) in [(257, 49), (65, 33), (257, 16), (16, 49), (33, 17), (1, 1), (33, 257), (300, 290)]:
        for coef in COEF:
            frames.append(vf.random_frame(rs, w, h, "mix", filt, coef))
            names.append(("mix", filt, coef))
    check_frames(pkg, checker, frames, names)


def stream_frames(checker, tmp_path, plan, seed):
    """writer streams (tests/vp8_writer.py) -> their files and, through vp8::parse (vp8_check --frame), their descriptors"""
    import vp8_writer as vw
    d, exe = checker
    rs = np.random.RandomState(seed)
    files, args = [], []
    for k, (w, h, pred, filt, coef, container) in enumerate(plan):
        data = vw.write_webp(vw.random_description(rs, w, h, pred, filt, coef, parts=k % 4, segments=bool((k // 4) % 2)), container)
        src = tmp_path / ("s%03d.webp" % k)
        src.write_bytes(data)
        files.append(data)
        args += [str(src), str(tmp_path / ("s%03d.frame" % k))]
    subprocess.check_call([exe, "--frame"] + args)
    return files, [vf.read_frames(args[2 * k + 1])[0] for k in range(len(plan))]


@pytest.mark.gpu
@pytest.mark.parametrize("turn", [0, 1, 2])
def test_device_equals_host_pixels_on_writer_streams(built, pkg, checker, tmp_path, turn):
    """ocr_vp8_decode == vp8::pixels on key frames written bit by bit, parsed by vp8::parse: every size of the grid, with
    partitions, segments, filter headers (simple, sharpness, deltas), probability updates and coefficients up to the largest
    token - the descriptor fields as a real header and real tokens make them"""
    from test_vp8_decode import stream_plan
    plan = stream_plan(315)[63 * turn:63 * turn + 63]
    _, frames = stream_frames(checker, tmp_path, plan, 20 + turn)
    check_frames(pkg, checker, frames, plan)


@pytest.mark.gpu
def test_one_stage_call_with_frames_of_different_grids(tool, checker, tmp_path):
    """One ocr_pipe_stage_batch call (decode_tool --stage) with seven lossy frames of different macroblock grids - 1 x 1, a row, a
    column, 3 x 17 (a diagonal longer than the workgroup's waves), odd widths: every image equals its single device decode and
    its host decode, so no frame's walk leaks into its neighbour in the batch"""
    plan = [(1, 1, "mix", "deltas", "dense", "bare"), (257, 16, "mix", "normal63", "extreme", "vp8x"), (15, 49, "b_6", "simple", "dense", "bare"),
            (33, 257, "mix", "deltas", "dense", "bare"), (65, 33, "i16_1", "sharp7", "dc", "vp8x"), (31, 17, "mix", "none", "dense", "bare"),
            (257, 49, "mix", "deltas", "extreme", "bare")]
    files, _ = stream_frames(checker, tmp_path, plan, 77)
    cases = [(str(p), data, None) for p, data in zip(plan, files)]
    host = decode_files(cases, tmp_path)
    single = decode_files(cases, tmp_path, "--device")
    staged = decode_files(cases, tmp_path, "--stage", os.path.join(ROOT, "models"))
    for (name, _, _), a, b, c in zip(cases, staged, single, host):
        assert a.shape == b.shape and np.array_equal(a, b), name
        assert np.array_equal(a, c), name


def golden_frames(checker):
    d, exe = checker
    files = sorted(glob.glob(os.path.join(GOLDEN, "*.webp")))
    frames, wants = [], []
    for path in files:
        dump = d / "golden.bin"
        subprocess.check_call([exe, "--frame", path, str(dump)])
        frames.append(vf.read_frames(dump)[0])
        npy = path[:-5] + ".npy"
        wants.append(np.load(npy if os.path.exists(npy) else os.path.join(GOLDEN, "card_q90.npy")))
    return files, frames, wants


@pytest.mark.gpu
def test_golden_files_of_libwebps_encoder(built, pkg, checker):
    """tests/golden/webp_lossy: vp8::parse (vp8_check --frame) -> ocr_vp8_decode equals the stored WebPDecodeBGR pixels"""
    files, frames, wants = golden_frames(checker)
    assert len(files) >= 24
    for path, fr, want in zip(files, frames, wants):
        got = device_decode(pkg, fr)
        assert got.shape == want.shape and np.array_equal(got, want), os.path.basename(path)


@pytest.mark.gpu
def test_descriptor_rules_reach_no_launch(built, pkg, checker):
    """every descriptor rule -> OCR_ERR_ARG with its message and the 0xA5-filled output untouched (the CPU test, on the machine
    that could launch); a sound descriptor decodes"""
    _descriptor_rules(built, pkg)
    rs = np.random.RandomState(7)
    check_frames(pkg, checker, [vf.random_frame(rs, 20, 17, "mix", "deltas", "dense")], ["sound"])


def golden(name):
    stem = os.path.join(GOLDEN, name)
    return open(stem + ".webp", "rb").read(), np.load(stem + ".npy")


def _jpeg(arr, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="JPEG", **kw)
    return buf.getvalue()


@pytest.mark.gpu
def test_one_stage_call_with_jpeg_png_lossless_and_lossy_webp_frames(tool, tmp_path):
    """One ocr_pipe_stage_batch call (decode_tool --stage) with a JPEG, a PNG, a lossless WebP and lossy WebPs of different
    macroblock grids - one of an odd width, one with ALPH in VP8X: every ocr_pipe_slot_image equals the single device decode
    and the host decode of the same file, and the stored libwebp pixels"""
    import png_writer as pw
    rs = np.random.RandomState(43)
    rgb = rs.randint(0, 256, (53, 37, 3)).astype(np.uint8)
    s = pw.random_samples(rs, 53, 37, 6, 8)
    lossless = os.path.join(ROOT, "tests", "golden", "webp", "rgb_65x66_m4")
    cases = [("lossy text 65x66", *golden("text_65x66_q90_m6")),
             ("4:2:0 37x53", _jpeg(rgb, quality=90, subsampling=2), None),
             ("RGBA 8 interlaced 37x53", pw.write_png(s, 6, 8, 1, [3, 4, 0, 1, 2]), pw.expected_bgr(s, 6, 8)),
             ("lossless", open(lossless + ".webp", "rb").read(), np.load(lossless + ".npy")),
             ("lossy flat 257x49", *golden("flat_257x49_q100_m6")),
             ("lossy 1x1", *golden("flat_1x1_q50_m4")),
             ("lossy rgba", *golden("text_rgba_130x33_q50_m4")),
             ("lossy photo 17x33", *golden("photo_17x33_q50_m6"))]
    models = os.path.join(ROOT, "models")
    host = decode_files(cases, tmp_path)
    single = decode_files(cases, tmp_path, "--device")
    staged = decode_files(cases, tmp_path, "--stage", models)
    for (name, _, want), a, b, c in zip(cases, staged, single, host):
        assert a.shape == b.shape and np.array_equal(a, b), name
        assert np.array_equal(a, c), name
        if want is not None:
            assert np.array_equal(a, want), name


@pytest.mark.gpu
def test_timing_entry_points_run(tool, tmp_path):
    """ocr_vp8_time (decode_tool --time <iters> <file>) and ocr_vp8_time_batch (... <batch>): OCR_OK and finite positive times"""
    src = tmp_path / "t.webp"
    src.write_bytes(golden("text_65x66_q90_m6")[0])
    for extra, batch in (([], 1), (["3"], 3)):
        r = subprocess.run([tool, "--time", "2", str(src)] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-1000:]
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        assert rec["lossy"] is True and rec["batch"] == batch and rec["iters"] == 2 and rec["size"] == [66, 65] and rec["bytes_out"] == 66 * 65 * 3 * batch
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
    """the service with the WebP pixel stage on the device (OCR_DEVICE_WEBP=1) and on the host (unset, the default)"""
    d = tempfile.mkdtemp(prefix="ocr", dir="/tmp")
    before = os.environ.get("OCR_DEVICE_WEBP")
    if request.param == "device":
        os.environ["OCR_DEVICE_WEBP"] = "1"
    else:
        os.environ.pop("OCR_DEVICE_WEBP", None)
    try:
        proc, sock = _start(d, 1)
    finally:
        if before is None:
            os.environ.pop("OCR_DEVICE_WEBP", None)
        else:
            os.environ["OCR_DEVICE_WEBP"] = before
    try:
        yield sock
        Client(sock).call({"command": "shutdown"})
        assert proc.wait(timeout=30) == 0
    finally:
        if proc.poll() is None:
            proc.kill()
        shutil.rmtree(d, ignore_errors=True)


@pytest.mark.gpu
def test_service_answers_lossy_webps_like_their_pixels_as_png(built, tmp_path, service):
    """the lossy card (quality 90, bare and in VP8X) as `recognize` requests by path and by base64: "success": true and the reply
    the stored decoded pixels get when they are sent as a PNG - with OCR_DEVICE_WEBP=1 and without"""
    import png_writer as pw
    c = Client(service)
    pixels = np.load(os.path.join(GOLDEN, "card_q90.npy"))
    h, w = pixels.shape[:2]
    files = {"bare": open(os.path.join(GOLDEN, "card_q90.webp"), "rb").read(), "vp8x": open(os.path.join(GOLDEN, "card_q90_vp8x.webp"), "rb").read(),
             "png": pw.write_png(pixels[:, :, ::-1].astype(np.int64).reshape(h, w, 3), 2, 8, 0, [0] * h)}
    paths = {}
    for name, data in files.items():
        p = tmp_path / (name + ".bin")
        p.write_bytes(data)
        paths[name] = str(p)
    want = c.call({"command": "recognize", "image_path": paths["png"]})
    assert want["success"] is True and (want["width"], want["height"]) == (w, h) and len(want["words"]) > 0
    for name in ("bare", "vp8x"):
        _same_reply(c.call({"command": "recognize", "image_path": paths[name]}), want)
        _same_reply(c.call({"command": "recognize", "image_data": base64.b64encode(files[name]).decode()}), want)
