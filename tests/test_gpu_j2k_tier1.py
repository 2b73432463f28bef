"""JPEG 2000 requests, tier-1 on the device (csrc/kernels_j2k_t1.hip through ocr_j2k_tier1 / ocr_j2k_decode_coded /
ocr_pipe_stage_batch) and through the service with OCR_DEVICE_J2K=2.  The yardstick is the host's j2k::tier1 (host/j2k_check
--tier1 over the same descriptors), which tests/test_j2k_blocks.py holds to j2k::parse and tests/test_j2k_decode.py to OpenJPEG.
Every comparison is exact equality of integers or bytes."""
import base64
import json
import math
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import j2k_blocks as jb  # noqa: E402
import j2k_frames as jf  # noqa: E402
from test_gpu_j2k import _same_reply, golden, golden_files  # noqa: E402
from test_ipc_service import Client, _start  # noqa: E402
from test_raw_decode import TOOL, read_ppm  # noqa: E402

ROOT = jf.ROOT


@pytest.fixture(scope="module")
def tool(built):
    subprocess.check_call(["make", "-s", "-C", jf.HOST])
    return TOOL


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("j2ktier1")
    return d, jf.build_check(d)


@pytest.mark.gpu
def test_random_blocks_equal_the_host_tier1(built, pkg, checker):
    """ocr_j2k_tier1 == j2k::tier1 over 416 blocks in one batch: every size of jb.SIZES with every segment kind of jb.SEGMENTS
    and every orientation, numbps (1, 2, 9, 30) and passes (1, 2, 3, 4, 3 * numbps - 2, at most what numbps allows) going round
    so that each pair of them meets each size; three tile-components, blocks at non-zero offsets in planes wider than any
    block.  The planes are compared whole, so every sample outside the blocks must read zero."""
    d, exe = checker
    cd, cases = jb.random_blocks(np.random.RandomState(17))
    assert len(cases) == len(jb.SIZES) * len(jb.SEGMENTS) * 4
    seen = {(c["w"], c["h"], c["numbps"], c["passes"]) for c in cases}
    for (w, h) in jb.SIZES:
        for nb in jb.NUMBPS:
            for pa in jb.PASSES:
                assert (w, h, nb, min(pa, 3 * nb - 2) if pa else 3 * nb - 2) in seen
    assert {(c["seg"], c["orient"]) for c in cases} == {(s, o) for s in jb.SEGMENTS for o in range(4)}
    want = jb.host_tier1(exe, d, [cd])[0]["coeffs"]
    got = jb.to_binding(pkg, cd).tier1(fill=0x5a5a5a5a)
    assert got.shape == want.shape
    plane = cd["width"] * cd["height"]
    inside = np.zeros(len(want), bool)
    for c, k in zip(cases, cd["cblks"]):
        at = int(k["tc"]) * plane + int(k["at"])
        rows = at + np.arange(c["h"])[:, None] * cd["width"] + np.arange(c["w"])[None, :]
        inside[rows.reshape(-1)] = True
        assert np.array_equal(got[rows], want[rows]), c
    assert not got[~inside].any() and not want[~inside].any()
    assert np.array_equal(got, want)
    # (the blocks are not all zero: random bytes decode to something in all but the shortest segments)
    assert np.count_nonzero(want) > inside.sum() // 4


def coded_of(exe, d, path):
    dump = os.path.join(str(d), "g.coded")
    subprocess.check_call([exe, "--coded", path, dump])
    return jb.read_coded(dump)[0]


@pytest.mark.gpu
def test_golden_files_through_the_coded_route(built, pkg, checker):
    """tests/golden/jp2: j2k::parse_coded (j2k_check --coded) -> ocr_j2k_decode_coded equals the stored pixels of OpenJPEG's
    decoder and ocr_j2k_decode of the coefficient route; ocr_j2k_tier1 equals the coefficients of j2k::parse"""
    d, exe = checker
    files = golden_files()
    assert len(files) >= 20
    for path in files:
        cd = coded_of(exe, d, path)
        dump = d / "golden.bin"
        subprocess.check_call([exe, "--frame", path, str(dump)])
        fr = jf.read_frames(dump)[0]
        assert cd["device_ok"] == 1, path
        coded = jb.to_binding(pkg, cd)
        got, want = coded.decode(), np.load(os.path.splitext(path)[0] + ".npy")
        assert got.shape == want.shape and np.array_equal(got, want), os.path.basename(path)
        assert np.array_equal(got, jf.to_binding(pkg, fr).decode()), os.path.basename(path)
        assert np.array_equal(coded.tier1(), fr["coeffs"]), os.path.basename(path)


@pytest.mark.gpu
def test_one_stage_call_with_coded_frames_beside_the_other_formats(tool, tmp_path):
    """One ocr_pipe_stage_batch call (decode_tool --stage) with coded JPEG 2000 frames of different shapes beside
    coefficient-form JPEG 2000 frames, a JPEG, a PNG and both kinds of WebP: every ocr_pipe_slot_image equals the single device
    decode of the coded route (OCR_DEVICE_J2K=2, --device), the host decode, and the stored pixels"""
    import io
    import png_writer as pw
    from PIL import Image
    rs = np.random.RandomState(44)
    rgb = rs.randint(0, 256, (53, 37, 3)).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="JPEG", quality=90, subsampling=2)
    s = pw.random_samples(rs, 53, 37, 6, 8)
    lossless = os.path.join(ROOT, "tests", "golden", "webp", "rgb_65x66_m4")
    lossy = os.path.join(ROOT, "tests", "golden", "webp_lossy", "text_65x66_q90_m6")
    names = [os.path.splitext(os.path.basename(p))[0] for p in golden_files()]
    pick = [n for n in names if not n.startswith("card")][::3]
    # (name, file bytes, stored pixels, coded form?)
    cases = [("jp2 " + n, *golden(n), k % 2 == 0) for k, n in enumerate(pick[:4])]
    cases += [("4:2:0 37x53", buf.getvalue(), None, False), ("RGBA 8 interlaced 37x53", pw.write_png(s, 6, 8, 1, [3, 4, 0, 1, 2]), pw.expected_bgr(s, 6, 8), False),
              ("lossless webp", open(lossless + ".webp", "rb").read(), np.load(lossless + ".npy"), False),
              ("lossy webp", open(lossy + ".webp", "rb").read(), np.load(lossy + ".npy"), False)]
    cases += [("jp2 " + n, *golden(n), k % 2 == 1) for k, n in enumerate(pick[4:])]
    ncoded = sum(c[3] for c in cases)
    assert ncoded >= 3 and sum(c[0].startswith("jp2") and not c[3] for c in cases) >= 3
    assert len({c[2].shape for c in cases if c[3]}) >= 2

    def run(flags, coded_prefix, env=None):
        args = []
        for i, (_, data, _, coded) in enumerate(cases):
            src = tmp_path / ("r%04d.bin" % i)
            src.write_bytes(data)
            args += [("coded:" if coded and coded_prefix else "") + str(src), str(tmp_path / ("r%04d.ppm" % i))]
        r = subprocess.run([TOOL, *flags] + args, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        return [read_ppm(tmp_path / ("r%04d.ppm" % i)) for i in range(len(cases))]
    host = run([], False, {"OCR_DEVICE_J2K": "0"})
    single = run(["--device"], False, {"OCR_DEVICE_J2K": "2"})
    staged = run(["--stage", os.path.join(ROOT, "models")], True)
    for (name, _, want, _), a, b, c in zip(cases, staged, single, host):
        assert a.shape == b.shape and np.array_equal(a, b), name
        assert np.array_equal(a, c), name
        if want is not None:
            assert np.array_equal(a, want), name


def coded_rules():
    """every rule a coded descriptor can break: (change, part of the message) - those of j2k::coded_fault, one of the frame's
    (j2k::fault_of) and those of the entry point itself"""
    def blk(i, key, value):
        def f(cd):
            cd["cblks"][i][key] = value
        return f

    def size(i, w, h):
        def f(cd):
            cd["cblks"][i]["w"], cd["cblks"][i]["h"] = w, h
        return f
    return [(blk(0, "w", 0), "1 .. 1024"), (blk(1, "h", 0), "1 .. 1024"), (blk(2, "w", 1025), "1 .. 1024"), (blk(2, "h", 1025), "1 .. 1024"), (size(3, 128, 64), "4096 samples"),
            (blk(4, "orient", 4), "orientation"), (blk(5, "numbps", 0), "bit planes"), (blk(5, "numbps", 31), "bit planes"), (blk(6, "passes", 0), "passes"),
            (blk(6, "passes", 14), "passes"), (blk(7, "tc", 6), "tile-component lies beyond"), (blk(1, "h", 7), "rectangle leaves"), (blk(1, "w", 4), "rectangle leaves"),
            (blk(8, "at", 1 << 20), "rectangle leaves"), (blk(9, "byte_off", 1 << 40), "bytes lie beyond"), (blk(17, "byte_len", 41), "bytes lie beyond"),
            (lambda cd: cd.__setitem__("bytes", cd["bytes"][:-1]), "bytes lie beyond"), (lambda cd: cd.__setitem__("prec", 17), "precision"),
            (lambda cd: cd.__setitem__("ncoeffs", cd["ncoeffs"] - 1), "coefficients lie beyond")]


@pytest.mark.gpu
def test_coded_descriptor_rules_are_refused_before_any_device_call(built, pkg, checker):
    """every rule -> OCR_ERR_ARG with its message from ocr_j2k_decode_coded and from ocr_j2k_tier1, the 0xA5-filled output
    untouched; the sound descriptor decodes to the host's pixels"""
    d, exe = checker
    sound = jb.small_coded(np.random.RandomState(2))
    for change, text in coded_rules():
        cd = dict(sound, cblks=sound["cblks"].copy(), bytes=sound["bytes"].copy())
        change(cd)
        for call in ("decode", "tier1"):
            with pytest.raises(pkg.OcrError) as e:
                getattr(jb.to_binding(pkg, cd), call)(fill=0xA5 if call == "decode" else -1515870811)
            assert e.value.code == -1 and re.search(re.escape(text), str(e.value)), (text, call, str(e.value))
            assert (e.value.out == (0xA5 if call == "decode" else -1515870811)).all()
    fr = jb.host_tier1(exe, d, [sound])[0]
    want = jf.host_pixels(exe, d, [fr])[0]
    got = jb.to_binding(pkg, sound).decode()
    assert got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(jb.to_binding(pkg, sound).tier1(), fr["coeffs"])


@pytest.mark.gpu
def test_coded_timing_entry_points_run(built, pkg, checker, tool, tmp_path):
    """ocr_j2k_time_coded and ocr_j2k_time_coded_batch, through the binding and through decode_tool --time: OCR_OK and finite
    positive times; the record keeps its keys and gains the coded route's"""
    d, exe = checker
    path = [p for p in golden_files() if os.path.basename(p).startswith("card_53")][0]
    coded = jb.to_binding(pkg, coded_of(exe, d, path))
    for ms in (coded.time(2), pkg.time_j2k_coded([coded, coded, coded], 2)):
        assert len(ms) == 3 and all(math.isfinite(t) and t > 0 for t in ms), ms
    for extra, batch in (([], 1), (["3"], 3)):
        r = subprocess.run([tool, "--time", "2", path] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-1000:]
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        assert rec["j2k"] is True and rec["batch"] == batch and rec["iters"] == 2
        for key in ("upload_ms", "pixel_stage_ms", "host_pixels_ms", "host_tier1_ms_per_image", "coded_upload_ms", "tier1_stage_ms", "coded_pixel_stage_ms",
                    "host_tier2_ms_per_image"):
            assert math.isfinite(rec[key]) and rec[key] > 0, (key, rec)
        assert 0 < rec["coded_descriptor_bytes"] < rec["descriptor_bytes"]


@pytest.fixture(scope="module")
def service(built):
    """the service with tier-1 and the pixel stage on the device (OCR_DEVICE_J2K=2)"""
    d = tempfile.mkdtemp(prefix="ocr", dir="/tmp")
    before = os.environ.get("OCR_DEVICE_J2K")
    os.environ["OCR_DEVICE_J2K"] = "2"
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
def test_service_answers_jpeg2000_through_the_coded_route(built, tmp_path, service):
    """card_53 (JP2, 5/3) and card_97_bare (codestream, 9/7) as `recognize` requests by path and by base64 under
    OCR_DEVICE_J2K=2: "success": true and the reply the stored decoded pixels get when they are sent as a PNG"""
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
