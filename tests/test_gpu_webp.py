"""Lossless WebP requests, device half (csrc/kernels_webp.hip through ocr_webp_decode / ocr_pipe_stage_batch) and through the
service.  The yardstick is the host pixel stage, webp::pixels of host/webp_decode.h (run by host/webp_check --pixels over the
same descriptors), which tests/test_webp_decode.py pins against libwebp; the numpy statement of the inverse transforms
(tests/webp_writer.py convert) is asserted beside it.  Neither libwebp nor Pillow's WebP support is needed here."""
import base64
import glob
import io
import itertools
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
import webp_writer as ww  # noqa: E402
from test_ipc_service import Client, _start  # noqa: E402
from test_raw_decode import TOOL, decode_files  # noqa: E402
from test_webp_decode import HOST, build_check  # noqa: E402
from test_webp_decode import test_descriptor_rules_are_refused_before_any_device_call as _descriptor_rules  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = [1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 66, 129, 257]
HEIGHTS = [1, 2, 3, 63, 64, 65, 66, 127, 128, 130]
P, X, G, I = ww.PREDICTOR, ww.CROSS_COLOUR, ww.ADD_GREEN, ww.COLOUR_INDEXING
# every order of every subset of predictor, cross-colour and add-green, alone and behind colour indexing: the device scope
ORDERS = [head + order for head in ((), (I,)) for n in range(4) for sub in itertools.combinations((P, X, G), n) for order in itertools.permutations(sub)]
FORMS = ["mode%d" % m for m in range(14)] + ["mix"] + ["orders%d" % k for k in range(4)]


@pytest.fixture(scope="module")
def tool(built):
    subprocess.check_call(["make", "-s", "-C", HOST])
    return TOOL


def write_frames(path, frames):
    with open(path, "wb") as f:
        for fr in frames:
            f.write(struct.pack("<3i", fr["w"], fr["h"], len(fr["transforms"])))
            coded = np.ascontiguousarray(fr["coded"], np.uint32).reshape(-1)
            f.write(struct.pack("<Q", len(coded)) + coded.tobytes())
            for kind, bits, data in fr["transforms"]:
                d = np.zeros(0, np.uint32) if data is None else np.ascontiguousarray(data, np.uint32).reshape(-1)
                f.write(struct.pack("<2iQ", kind, bits, len(d)) + d.tobytes())


def read_frames(path):
    frames, blob, pos = [], open(path, "rb").read(), 0

    def dwords():
        nonlocal pos
        n, = struct.unpack_from("<Q", blob, pos)
        a = np.frombuffer(blob, np.uint32, n, pos + 8)
        pos += 8 + 4 * n
        return a

    while pos < len(blob):
        w, h, nt = struct.unpack_from("<3i", blob, pos)
        pos += 12
        coded = dwords()
        transforms = []
        for _ in range(nt):
            kind, bits = struct.unpack_from("<2i", blob, pos)
            pos += 8
            d = dwords()
            transforms.append((kind, bits, d if len(d) else None))
        frames.append(dict(w=w, h=h, coded=coded, transforms=transforms))
    return frames


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("webppixels")
    return d, build_check(d)


@pytest.fixture(scope="module")
def host_pixels(checker):
    """webp::pixels over a list of descriptors: host/webp_check.cpp --pixels, a plain host program"""
    d, exe = checker

    def run(frames):
        src, out = d / "frames.bin", d / "pixels.bin"
        write_frames(src, frames)
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


def make_frame(rs, w, h, kinds, **kw):
    """a descriptor (what webp::parse would hand over) of random coded data and the numpy model of its pixels"""
    coded, transforms = ww.random_case(rs, w, h, kinds, **kw)
    return dict(w=w, h=h, coded=coded, transforms=transforms), ww.convert(w, h, coded, transforms)


def device_decode(pkg, fr):
    return pkg.WebpFrame(fr["w"], fr["h"], fr["coded"], fr["transforms"]).decode()


def describe(fr):
    return dict(w=fr["w"], h=fr["h"], transforms=[(k, b) for k, b, _ in fr["transforms"]])


def check_frames(pkg, host_pixels, frames_and_models):
    host = host_pixels([f for f, _ in frames_and_models])
    for (fr, model), ref in zip(frames_and_models, host):
        assert np.array_equal(ref, model), ("webp::pixels differs from the numpy rules", describe(fr))
        got = device_decode(pkg, fr)
        assert np.array_equal(got, ref), (describe(fr), int((got != ref).sum()))


def shapes(offset):
    """widths and heights taken in turn: every width once, the heights cycling from `offset` - over the forms every pair of a
    width class and a height class occurs: band seams (64 rows, then 63 new ones, a replayed row: 65, 66, 127, 128, 130), ring-tile
    seams (64, 128 coded pixels), rows shorter than the two-pixel skew, a single column"""
    return [(w, HEIGHTS[(i + offset) % len(HEIGHTS)]) for i, w in enumerate(WIDTHS)]


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_device_equals_host_pixel_stage(built, pkg, host_pixels, form):
    """ocr_webp_decode == webp::pixels byte for byte: the 14 modes each alone, random mode mixes and every transform order in
    device scope, widths {1 .. 257} x heights {1 .. 130} taken in turn, block bits 2 and one value larger than the image"""
    k = FORMS.index(form)
    rs = np.random.RandomState(500 + k)
    cases = []
    if form.startswith("orders"):
        part = ORDERS[int(form[6:])::4]
        assert len(ORDERS) == 32 and len(part) == 8
        sizes = itertools.cycle(shapes(k))
        for order in part:
            for bits in (2, 9, 3):
                w, h = next(sizes)
                cases.append(make_frame(rs, w, h, order, bits=bits, colours=(2, 4, 16, 40)[len(cases) % 4]))
        cases.append(make_frame(rs, 257, 130, part[-1], bits=2, colours=16))
    else:
        modes = None if form == "mix" else int(form[4:])
        for i, (w, h) in enumerate(shapes(k)):
            cases.append(make_frame(rs, w, h, (P,), bits=(2, 9)[i % 2] if modes is not None else 2 + (i % 3), modes=modes))
        cases.append(make_frame(rs, 257, 130, (G, X, P), bits=2, modes=modes))
    check_frames(pkg, host_pixels, cases)


@pytest.mark.gpu
def test_top_right_of_the_last_column_is_the_rows_first_pixel(built, pkg, host_pixels):
    """every block mode 3 (TR) and mode 9 (avg(T, TR)), widths 2 and 65: the right answer differs from the answer with TR = 0 at
    the last column and from the answer with TR clamped to the row above's last pixel - the model tells them apart - and the device
    gives the right one"""
    rs = np.random.RandomState(9)
    cases = []
    for mode in (3, 9):
        for w in (2, 65):
            fr, model = make_frame(rs, w, 7, (P,), bits=2, modes=mode)
            for wrong in ("zero", "past"):
                other = ww.convert(w, 7, fr["coded"], fr["transforms"], tr=wrong)
                assert not np.array_equal(other[1:, -1], model[1:, -1]), (mode, w, wrong)
                assert np.array_equal(other[0], model[0])
            cases.append((fr, model))
    check_frames(pkg, host_pixels, cases)


@pytest.mark.gpu
def test_streaming_kernel(built, pkg, host_pixels):
    """frames without a predictor: palette-only files at every bundling (8 / 4 / 2 / 1 indices a coded pixel), indices beyond the
    palette, add-green, cross-colour and their orders; odd widths, whose rows start at every address & 3, rows wider than one
    span of a workgroup (1024 pixels) and rows of fewer pixels than the head"""
    rs = np.random.RandomState(21)
    cases = []
    for colours in (1, 2, 3, 4, 5, 16, 17, 256):
        for w, h in ((1, 5), (3, 4), (7, 9), (33, 5), (1027, 3), (2051, 2)):
            cases.append(make_frame(rs, w, h, (I,), colours=colours, beyond=w == 33))
    for order in ((), (G,), (X,), (G, X), (X, G), (I, G), (I, X, G)):
        for w, h in ((5, 3), (65, 7), (1029, 2)):
            cases.append(make_frame(rs, w, h, order, bits=3, colours=6))
    check_frames(pkg, host_pixels, cases)


@pytest.mark.gpu
def test_golden_files_of_libwebps_encoder(built, pkg, checker):
    """tests/golden/webp: webp::parse (webp_check --frame) -> ocr_webp_decode equals the stored WebPDecodeBGR pixels"""
    d, exe = checker
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "webp", "*.webp")))
    assert len(files) >= 12
    with_predictor = 0
    for path in files:
        out = d / "golden.bin"
        subprocess.check_call([exe, "--frame", path, str(out)])
        fr, = read_frames(out)
        with_predictor += any(k == P for k, _, _ in fr["transforms"])
        want = np.load(path[:-5] + ".npy")
        coded_w = ww.coded_width(fr["w"], fr["transforms"])
        got = device_decode(pkg, dict(fr, coded=fr["coded"].reshape(fr["h"], coded_w)))
        assert got.shape == want.shape and np.array_equal(got, want), os.path.basename(path)
    assert with_predictor >= 3


@pytest.mark.gpu
def test_descriptor_rules_reach_no_launch(built, pkg):
    """every descriptor rule -> OCR_ERR_ARG with its message (the CPU test, on the machine that could launch); a descriptor
    outside the device scope (colour indexing not first) leaves the output buffer untouched; a sound descriptor decodes"""
    import ctypes as C
    _descriptor_rules(built, pkg)
    rs = np.random.RandomState(7)
    fr, _ = make_frame(rs, 9, 5, (G, I), colours=5)
    f = pkg.WebpFrame(fr["w"], fr["h"], fr["coded"], fr["transforms"])
    L = pkg.lib()
    L.ocr_webp_decode.argtypes = [C.POINTER(pkg.ocr_webp_frame), C.c_int, C.c_void_p, C.c_size_t]
    out = np.full((5, 9, 3), 0xA5, np.uint8)
    assert L.ocr_webp_decode(C.byref(f.c), 0, out.ctypes.data, out.size) == -1
    assert b"colour indexing must be the first" in L.ocr_last_error() and (out == 0xA5).all()
    frame, model = make_frame(rs, 4, 5, (G, P), bits=2)
    assert np.array_equal(device_decode(pkg, frame), model)


def _jpeg(arr, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def golden(name):
    stem = os.path.join(ROOT, "tests", "golden", "webp", name)
    return open(stem + ".webp", "rb").read(), np.load(stem + ".npy")


@pytest.mark.gpu
def test_one_stage_call_with_jpeg_png_bmp_tiff_and_webp_frames(tool, tmp_path):
    """One ocr_pipe_stage_batch call (decode_tool --stage) with a JPEG, a PNG, a BMP, a TIFF and WebPs - one with a predictor
    and one palette-only of an odd width: every ocr_pipe_slot_image equals the single device decode and the host decode of
    the same file, that is, staging the same images as decoded pixels"""
    import png_writer as pw
    import raw_writer as rw
    import tiff_writer as tw
    rs = np.random.RandomState(43)
    rgb = rs.randint(0, 256, (53, 37, 3)).astype(np.uint8)
    s = pw.random_samples(rs, 53, 37, 6, 8)
    idx = rs.randint(0, 256, (53, 37))
    pal = rs.randint(0, 256, (256, 3))
    samples = rs.randint(0, 256, (53, 37, 3))
    coded, transforms = ww.random_case(rs, 37, 53, (I,), colours=3)
    file_a, want_a = golden("rgb_65x66_m4")
    cases = [("webp rgb", file_a, want_a),
             ("4:2:0 37x53", _jpeg(rgb, quality=90, subsampling=2), None),
             ("RGBA 8 interlaced 37x53", pw.write_png(s, 6, 8, 1, [3, 4, 0, 1, 2]), pw.expected_bgr(s, 6, 8)),
             ("webp palette 37x53", ww.write_webp(37, 53, coded, transforms, rs=rs), ww.convert(37, 53, coded, transforms)),
             ("bmp8 37x53", rw.write_bmp(idx, 8, palette=pal), rw.lookup(idx, pal)),
             ("tiff rgb8", tw.write_tiff(samples, 8, tw.RGB, compression=tw.LZW, predictor=2, rows_per_strip=8), tw.convert(samples, 8, tw.RGB)),
             ("webp rgba", *golden("rgba_130x33_m6"))]
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
    """ocr_webp_time (decode_tool --time <iters> <file>) and ocr_webp_time_batch (... <batch>): OCR_OK and finite positive times"""
    src = tmp_path / "t.webp"
    src.write_bytes(golden("rgb_65x66_m4")[0])
    for extra, batch in (([], 1), (["3"], 3)):
        r = subprocess.run([tool, "--time", "2", str(src)] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-1000:]
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        assert rec["batch"] == batch and rec["iters"] == 2 and rec["size"] == [66, 65] and rec["bytes_out"] == 66 * 65 * 3 * batch
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


def card_webps(card):
    """the test card (BGR) as lossless WebPs whose pixels ARE the card's, and as a PNG: {name: bytes}"""
    import png_writer as pw
    rs = np.random.RandomState(12)
    h, w = card.shape[:2]
    files = {"green cross predictor": ww.encode(card, rs, lz=dict(codes=[1, 2, 3, 121, 122], prob=0.2), cache_bits=4)[0],
             "predictor bits 2 in vp8x": ww.encode(card, rs, predictor_bits=2, cross_bits=3, container="vp8x")[0]}
    files["png"] = pw.write_png(card[:, :, ::-1].astype(np.int64).reshape(h, w, 3), 2, 8, 0, [0] * h)
    return files


@pytest.mark.gpu
def test_service_answers_webps_like_the_same_pixels_as_png(built, card, tmp_path, service):
    """lossless WebP `recognize` requests (image_path and base64): "success":true and the reply the same pixels get as a PNG -
    with OCR_DEVICE_WEBP=1 and without, so the two routes give equal replies; a lossy file and an animated one are answered
    with the error that says so"""
    c = Client(service)
    files = card_webps(card)
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
    lossy = ww.riff([ww.chunk(b"VP8 ", bytes(30))])
    animated = ww.riff([ww.vp8x(4, 4, 0x02), ww.chunk(b"ANIM", bytes(6)), ww.chunk(b"ANMF", bytes(24))])
    for name, data in (("lossy", lossy), ("animated", animated)):
        bad = tmp_path / (name + ".webp")
        bad.write_bytes(data)
        for request in ({"image_path": str(bad)}, {"image_data": base64.b64encode(data).decode()}):
            reply = c.call(dict(request, command="recognize"))
            assert reply["success"] is False and "lossy or animated WebP is not decoded" in reply["error"], (name, reply)
