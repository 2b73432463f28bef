"""JPEG 2000 requests, device half (csrc/kernels_j2k.hip through ocr_j2k_decode / ocr_pipe_stage_batch) and through the
service.  The yardstick is the host pixel stage, j2k::pixels of host/j2k_decode.h (run by host/j2k_check --pixels over the same
descriptors), which tests/test_j2k_decode.py pins against OpenJPEG.  Neither OpenJPEG nor Pillow's support for it is needed
here: the files are those of tests/golden/jp2."""
import base64
import glob
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
import j2k_frames as jf  # noqa: E402
from test_ipc_service import Client, _start  # noqa: E402
from test_raw_decode import TOOL, decode_files  # noqa: E402

ROOT = jf.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "jp2")


@pytest.fixture(scope="module")
def tool(built):
    subprocess.check_call(["make", "-s", "-C", jf.HOST])
    return TOOL


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("j2kpixels")
    return d, jf.build_check(d)


def check_frames(pkg, checker, frames, names):
    d, exe = checker
    for fr, want, name in zip(frames, jf.host_pixels(exe, d, frames), names):
        got = jf.to_binding(pkg, fr).decode()
        assert got.shape == want.shape and np.array_equal(got, want), (name, fr["width"], fr["height"])


@pytest.mark.gpu
@pytest.mark.parametrize("transform", [0, 1])
@pytest.mark.parametrize("levels", [0, 1, 2, 3, 4, 5])
def test_device_equals_host_pixels(built, pkg, checker, transform, levels):
    """ocr_j2k_decode == j2k::pixels byte for byte over random descriptors of every width x height of the grid at this level
    count and transform, the component transform, both parities of the origin in x and y, the precision (8, 12, 16 and 5) and
    the component count going round; one frame is tiled 40 x 24 from an odd tile origin, so its edge tiles are ragged"""
    rs = np.random.RandomState(10 * levels + transform)
    frames, names, k = [], [], 0
    seen = set()
    for w in jf.WIDTHS:
        for h in jf.HEIGHTS:
            mct, px, py = k % 2, (k // 2) % 2, (k // 4 + k) % 2
            prec = (8, 12, 16, 5)[(k // 3) % 4]
            frames.append(jf.random_frame(rs, w, h, levels, transform, mct, x0=px + 2 * (k % 3), y0=py, prec=prec, ncomp=(3, 1)[(k // 5) % 2], dense=k % 4 != 3))
            names.append((w, h, mct, px, py, prec))
            seen.add((mct, px, py))
            k += 1
    assert len(seen) == 8
    frames.append(jf.random_frame(rs, 129, 65, levels, transform, 1, x0=3, y0=5, tiling=(40, 24, 1, 2)))
    names.append("tiled")
    check_frames(pkg, checker, frames, names)


@pytest.mark.gpu
def test_a_tall_and_a_wide_frame(built, pkg, checker):
    """a column and a row longer than a workgroup's window (56 rows, 248 samples of a row), from odd origins, both transforms"""
    rs = np.random.RandomState(5)
    frames = [jf.random_frame(rs, w, h, 3, t, t, x0=1, y0=1) for t in (0, 1) for (w, h) in ((9, 700), (1100, 7))]
    check_frames(pkg, checker, frames, ["tall 5/3", "wide 5/3", "tall 9/7", "wide 9/7"])


def golden_files():
    return sorted(glob.glob(os.path.join(GOLDEN, "*.jp2")) + glob.glob(os.path.join(GOLDEN, "*.j2k")))


@pytest.mark.gpu
def test_golden_files_of_openjpegs_encoder(built, pkg, checker):
    """tests/golden/jp2: j2k::parse (j2k_check --frame) -> ocr_j2k_decode equals the stored pixels of OpenJPEG's decoder"""
    d, exe = checker
    files = golden_files()
    assert len(files) >= 20
    for path in files:
        dump = d / "golden.bin"
        subprocess.check_call([exe, "--frame", path, str(dump)])
        fr = jf.read_frames(dump)[0]
        assert fr["device_ok"] == 1, path
        got, want = jf.to_binding(pkg, fr).decode(), np.load(os.path.splitext(path)[0] + ".npy")
        assert got.shape == want.shape and np.array_equal(got, want), os.path.basename(path)


def descriptor_rules(pkg):
    """every rule of j2k::fault_of / device_fault: (what is broken, part of the message)"""
    rs = np.random.RandomState(3)

    def sound():
        return jf.random_frame(rs, 20, 17, 2, 1, 1, x0=1, y0=0, tiling=(16, 16, 0, 0))
    out = []

    def rule(change, text):
        fr = sound()
        change(fr)
        out.append((fr, text))

    def setk(key, value):
        return lambda fr: fr.__setitem__(key, value)

    def tc(i, key, value):
        def f(fr):
            fr["tcs"][i][key] = value
        return f
    rule(setk("width", 0), "positive")
    rule(setk("x0", -1), "origin")
    rule(setk("ncomp", 2), "1 or 3")
    rule(setk("prec", 17), "precision")
    rule(setk("transform", 2), "0 or 1")
    rule(setk("chan", [0, 3, 1]), "channel map")
    rule(lambda fr: fr.__setitem__("tcs", fr["tcs"][:-1]), "ncomp a tile")
    rule(tc(0, "x1", 30), "share|outside|raster")
    rule(tc(1, "y1", 3), "share")
    rule(tc(3, "x0", 17), "raster|outside")
    rule(tc(2, "levels", 33), "levels")
    rule(tc(2, "levels", 9), "device stage")
    rule(tc(1, "levels", 1), "one level count")
    rule(tc(4, "step_off", 1 << 20), "step sizes")
    rule(tc(5, "coeff_off", 1 << 40), "coefficients")
    rule(lambda fr: fr.__setitem__("tcs", fr["tcs"][:6]), "cover")
    return out


@pytest.mark.gpu
def test_descriptor_rules_are_refused_before_any_device_call(built, pkg, checker):
    """every descriptor rule -> OCR_ERR_ARG with its message and the 0xA5-filled output untouched; a sound descriptor decodes"""
    import re
    for fr, text in descriptor_rules(pkg):
        with pytest.raises(pkg.OcrError) as e:
            jf.to_binding(pkg, fr).decode(fill=0xA5)
        assert e.value.code == -1 and re.search(text, str(e.value)), (text, str(e.value))
        assert (e.value.out == 0xA5).all()
    rs = np.random.RandomState(7)
    check_frames(pkg, checker, [jf.random_frame(rs, 20, 17, 2, 1, 1, x0=1, tiling=(16, 16, 0, 0))], ["sound"])


def golden(name):
    stem = os.path.join(GOLDEN, name)
    path = stem + (".jp2" if os.path.exists(stem + ".jp2") else ".j2k")
    return open(path, "rb").read(), np.load(stem + ".npy")


@pytest.mark.gpu
def test_one_stage_call_with_jpeg2000_frames_beside_the_other_formats(tool, tmp_path):
    """One ocr_pipe_stage_batch call (decode_tool --stage) with JPEG 2000 frames of different shapes, transforms and level counts
    beside a JPEG, a PNG and both kinds of WebP: every ocr_pipe_slot_image equals the single device decode and the host decode
    of the same file, and the stored pixels"""
    import io
    import png_writer as pw
    from PIL import Image
    rs = np.random.RandomState(43)
    rgb = rs.randint(0, 256, (53, 37, 3)).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="JPEG", quality=90, subsampling=2)
    s = pw.random_samples(rs, 53, 37, 6, 8)
    lossless = os.path.join(ROOT, "tests", "golden", "webp", "rgb_65x66_m4")
    lossy = os.path.join(ROOT, "tests", "golden", "webp_lossy", "text_65x66_q90_m6")
    names = [os.path.splitext(os.path.basename(p))[0] for p in golden_files()]
    pick = [n for n in names if not n.startswith("card")][::3]
    cases = [("jp2 " + n, *golden(n)) for n in pick[:3]]
    cases += [("4:2:0 37x53", buf.getvalue(), None), ("RGBA 8 interlaced 37x53", pw.write_png(s, 6, 8, 1, [3, 4, 0, 1, 2]), pw.expected_bgr(s, 6, 8)),
              ("lossless webp", open(lossless + ".webp", "rb").read(), np.load(lossless + ".npy")),
              ("lossy webp", open(lossy + ".webp", "rb").read(), np.load(lossy + ".npy"))]
    cases += [("jp2 " + n, *golden(n)) for n in pick[3:]]
    assert sum(name.startswith("jp2") for name, _, _ in cases) >= 6
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
    """ocr_j2k_time (decode_tool --time <iters> <file>) and ocr_j2k_time_batch (... <batch>): OCR_OK and finite positive times"""
    src = tmp_path / "t.jp2"
    data, want = golden("card_53")
    src.write_bytes(data)
    for extra, batch in (([], 1), (["3"], 3)):
        r = subprocess.run([tool, "--time", "2", str(src)] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-1000:]
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        assert rec["j2k"] is True and rec["batch"] == batch and rec["iters"] == 2 and rec["size"] == list(want.shape[:2])
        for key in ("upload_ms", "pixel_stage_ms", "host_pixels_ms", "host_tier1_ms_per_image"):
            assert math.isfinite(rec[key]) and rec[key] > 0, rec


def _same_reply(got, want):
    assert got["success"] is True and want["success"] is True, (got.get("error"), want.get("error"))
    assert got["width"] == want["width"] and got["height"] == want["height"]
    assert len(got["words"]) == len(want["words"])
    for g, w in zip(got["words"], want["words"]):
        assert g["box"] == w["box"] and g["text"] == w["text"] and g["confidence"] == w["confidence"]


@pytest.fixture(scope="module", params=["device", "host"])
def service(request, built):
    """the service with the JPEG 2000 pixel stage on the device (OCR_DEVICE_J2K=1) and on the host (unset, the default)"""
    d = tempfile.mkdtemp(prefix="ocr", dir="/tmp")
    before = os.environ.get("OCR_DEVICE_J2K")
    if request.param == "device":
        os.environ["OCR_DEVICE_J2K"] = "1"
    else:
        os.environ.pop("OCR_DEVICE_J2K", None)
    try:
        proc, sock = _start(d, 1)
    finally:
        if before is None:
            os.environ.pop("OCR_DEVICE_J2K", None)
        else:
            os.environ["OCR_DEVICE_J2K"] = before
    try:
        yield sock
        Client(sock).call({"command": "shutdown"})
        assert proc.wait(timeout=30) == 0
    finally:
        if proc.poll() is None:
            proc.kill()
        shutil.rmtree(d, ignore_errors=True)


@pytest.mark.gpu
def test_service_answers_jpeg2000_like_its_pixels_as_png(built, tmp_path, service):
    """the card as a JP2 (5/3) and as a bare codestream (9/7), as `recognize` requests by path and by base64: "success": true and
    the reply the stored decoded pixels get when they are sent as a PNG - with OCR_DEVICE_J2K=1 and without"""
    import png_writer as pw
    c = Client(service)
    for name in ("card_53", "card_97_bare"):
        data, pixels = golden(name)
        h, w = pixels.shape[:2]
        files = {"j2k": data, "png": pw.write_png(pixels[:, :, ::-1].astype(np.int64).reshape(h, w, 3), 2, 8, 0, [0] * h)}
        paths = {}
        for kind, blob in files.items():
            p = tmp_path / (name + "." + kind)
            p.write_bytes(blob)
            paths[kind] = str(p)
        want = c.call({"command": "recognize", "image_path": paths["png"]})
        assert want["success"] is True and (want["width"], want["height"]) == (w, h)
        _same_reply(c.call({"command": "recognize", "image_path": paths["j2k"]}), want)
        _same_reply(c.call({"command": "recognize", "image_data": base64.b64encode(data).decode()}), want)


@pytest.mark.gpu
def test_a_refused_file_is_answered_with_its_reason(built, service):
    """a codestream whose COD sets a code-block style bit: the reply carries the decoder's reason"""
    data = bytearray(golden("card_97_bare")[0])
    at = data.index(b"\xff\x52")
    data[at + 12] |= 1  # selective arithmetic coding bypass
    reply = Client(service).call({"command": "recognize", "image_data": base64.b64encode(bytes(data)).decode()})
    assert reply["success"] is False and "code-block styles" in reply["error"], reply
