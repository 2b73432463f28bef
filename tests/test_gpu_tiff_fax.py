"""CCITT fax TIFF requests, device half: csrc/kernels_tiff_fax.hip through ocr_tiff_unfax / ocr_tiff_decode_fax /
ocr_pipe_stage_batch (OCR_FRAME_TIFF_FAX) and through the service with OCR_DEVICE_TIFF=1 .. 4.  The yardstick
is the host's tiff::unfax_all (run by host/tiff_check --unfax over the same fax frames), which tests/test_tiff_fax.py ties to
tiff::parse, to the bitmaps that were encoded and to libtiff.  Equality is exact, and the output is pre-filled with 0x5A, so a
byte the kernel does not write shows."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fax_writer as fx  # noqa: E402
from test_tiff_decode import build_check  # noqa: E402
from test_tiff_fax import LAYOUTS, bitmap_of  # noqa: E402
from test_tiff_fax import test_fax_rules_are_refused_before_any_device_call as _fax_rules  # noqa: E402


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """host/tiff_check.cpp, a plain host program: tiff::unfax_all and tiff::parse + tiff::pixels"""
    d = tmp_path_factory.mktemp("faxexpand")
    return build_check(d), d


def check_expansion(pkg, checker, codeds, tag):
    exe, d = checker
    for c, ref in zip(codeds, fx.host_unfax(exe, codeds, d, tag)):
        got = fx.to_pkg(pkg, c).unfax(fill=0x5A)
        assert got.shape == ref.shape and np.array_equal(got, ref), (c.get("name"), len(ref), int((got != ref).sum()), np.nonzero(got != ref)[0][:4])


@pytest.mark.gpu
def test_hand_built_and_branch_streams(built, pkg, checker):
    """one chunk each, in every coding: the branch bitmaps of the host's tests (all white, all black, alternating pixels, black
    from column 0, stripes shifting by -4 .. +4 a row, pass modes, runs of 63 .. 5200 around every make-up boundary); a chain of
    repeated make-ups built by hand; rows of 1, 3, 4, 5, 16 and 17 bytes in an odd number, so that the word stores meet every
    alignment; a short last strip (zero rows behind the stream's); a chunk whose coded bytes fill the LDS window several times
    (alternating pixels, 600 x 20); and a full list - width + 1 changing elements at 2048 pixels"""
    W, B = fx.WHITE, fx.BLACK
    cases = []
    for cname, comp, ckw in fx.CODINGS:
        enc = {a: b for a, b in ckw.items() if a != "t4"}
        for bname, bm in fx.branch_bitmaps():
            cases.append(fx.coded(bm, comp, t4=ckw.get("t4", 0), name="%s %s" % (cname, bname), **enc))
        for w in (8, 20, 32, 39, 128, 130):
            bm = bitmap_of(np.random.RandomState(w), w % 3, 3, w)
            cases.append(fx.coded(bm, comp, t4=ckw.get("t4", 0), name="%s row bytes of %d wide" % (cname, w), **enc))
        bm = bitmap_of(np.random.RandomState(5), 2, 3, 37)
        c = fx.coded(bm, comp, t4=ckw.get("t4", 0), name="%s short last strip" % cname, **enc)
        c["tile"] = (37, 8)   # a strip of 8 rows of which the image has 3
        c["h"] = 3
        cases.append(c)
        cases.append(fx.coded(np.tile(np.arange(600) % 2, (20, 1)), comp, t4=ckw.get("t4", 0), name="%s 600 x 20 alternating" % cname, **enc))
        cases.append(fx.coded(np.tile((np.arange(2048) + 1) % 2, (2, 1)), comp, t4=ckw.get("t4", 0), name="%s full list at 2048" % cname, **enc))
    chain = [("word", W, 2560), ("word", W, 2560), ("run", W, 80), ("run", B, 3)]
    cases.append(fx.one_chunk(chain, 5203, 1, fx.MH, name="mh: 2560 + 2560 + 80 by hand"))
    cases.append(fx.one_chunk([("eol",)] + chain + [("eol",)] + chain, 5203, 2, fx.G3, name="g3: the chain twice"))
    cases.append(fx.one_chunk([("horiz",)] + chain + [("v", 0), ("v", 0)], 5203, 2, fx.G4, name="g4: the chain in horizontal mode, then V0 V0"))
    cases.append(fx.one_chunk([("word", W, 64), ("word", W, 64), ("run", W, 2), ("run", B, 0), ("run", W, 3)], 133, 1, fx.MH, name="mh: 64 + 64 + 2, a zero black run"))
    assert max(len(c["data"]) for c in cases) > 4 * 1024
    check_expansion(pkg, checker, cases, "hand")


@pytest.mark.gpu
def test_geometry_matrix(built, pkg, checker):
    """every coding x {strips of 1, 2, 16 rows, one strip, 16 x 16 and 32 x 16 tiles} x both photometrics at the small sizes;
    what lies in an edge tile beyond the image is noise"""
    rs = np.random.RandomState(31)
    cases, n = [], 0
    for cname, comp, ckw in fx.CODINGS:
        enc = {a: b for a, b in ckw.items() if a != "t4"}
        for layout in LAYOUTS:
            for photometric in (0, 1):
                w, h = (1, 7, 9, 33, 65, 257)[n % 6], (1, 2, 5, 17)[(n // 2) % 4]
                cases.append(fx.coded(bitmap_of(rs, n % 3, h, w), comp, photometric=photometric, t4=ckw.get("t4", 0), rs=rs,
                                      name="%s %dx%d %s" % (cname, w, h, layout), **enc, **layout))
                n += 1
    check_expansion(pkg, checker, cases, "geo")


@pytest.mark.gpu
def test_decode_fax_equals_parse_and_pixels(built, pkg, checker):
    """ocr_tiff_decode_fax of the frame == tiff::parse + tiff::pixels of the file (tiff_check --decode) == the bitmap under the
    file's photometric"""
    exe, d = checker
    rs = np.random.RandomState(32)
    n = 0
    for cname, comp, ckw in fx.CODINGS:
        enc = {a: b for a, b in ckw.items() if a != "t4"}
        for layout in LAYOUTS[1::2]:
            photometric = n % 2
            w, h = (9, 33, 65, 257)[n % 4], (2, 5, 17)[n % 3]
            bm = bitmap_of(rs, n % 3, h, w)
            n += 1
            p = os.path.join(str(d), "d.tif")
            open(p, "wb").write(fx.write_fax(bm, comp, photometric=photometric, **ckw, **layout))
            assert subprocess.run([exe, "--decode", p, p + ".bgr"], capture_output=True).returncode == 0
            host = np.fromfile(p + ".bgr", np.uint8).reshape(h, w, 3)
            got = fx.to_pkg(pkg, fx.coded(bm, comp, photometric=photometric, t4=ckw.get("t4", 0), **enc, **layout)).decode(fill=0x5A)
            assert np.array_equal(host, fx.wanted(bm, photometric)) and np.array_equal(got, host), (cname, w, h, layout)


@pytest.mark.gpu
def test_a_chunk_wider_than_the_cap_takes_the_host_route(built, pkg, checker):
    """8200 pixels across: ocr_tiff_unfax refuses the frame before any launch; tiff::unfax_all expands it and ocr_tiff_decode
    takes the expanded frame to the pixels tiff::pixels gives"""
    exe, d = checker
    bm = bitmap_of(np.random.RandomState(33), 2, 3, 8200)
    c = fx.coded(bm, fx.G4)
    with pytest.raises(pkg.OcrError, match="wider than the device") as e:
        fx.to_pkg(pkg, c).unfax(fill=0x5A)
    assert e.value.code == -1 and (e.value.out == 0x5A).all()
    chunks = fx.host_unfax(exe, [c], d, "wide")[0]
    assert chunks.tobytes() == fx.expanded(bm)
    assert np.array_equal(pkg.TiffFrame(8200, 3, 0, 1, 1, chunks).decode(), fx.wanted(bm, 0))


@pytest.mark.gpu
def test_refusals_on_the_gpu_machine(built, pkg):
    """every refusal class returns OCR_ERR_ARG with the output untouched where a device is present too: no damaged stream is
    ever launched"""
    _fax_rules(built, pkg)


# ---- the frame kind, the tool and the service -------------------------------------------------------------------------------
import base64  # noqa: E402
import json  # noqa: E402
import math  # noqa: E402
import shutil  # noqa: E402
import tempfile  # noqa: E402

import tiff_writer as tw  # noqa: E402
from test_ipc_service import Client, _start  # noqa: E402
from test_raw_decode import TOOL, read_ppm  # noqa: E402
from test_tiff_decode import HOST  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tool(built):
    subprocess.check_call(["make", "-s", "-C", HOST])
    return TOOL


@pytest.mark.gpu
def test_one_stage_call_with_fax_tiffs_a_png_an_lzw_and_a_deflate_tiff(tool, tmp_path):
    """One ocr_pipe_stage_batch call (decode_tool --stage) with fax frames of every coding ("coded:<file>": OCR_FRAME_TIFF_FAX),
    a PNG, an LZW TIFF (OCR_FRAME_TIFF_CODED) and a Deflate TIFF (OCR_FRAME_TIFF_DEFLATE) between them: every
    ocr_pipe_slot_image equals the OCR_DEVICE_TIFF=0 decode and the bitmap; --stage and --device under OCR_DEVICE_TIFF=4 give
    the same, and stage the fax files as kind 10"""
    import png_writer as pw
    rs = np.random.RandomState(41)
    rgb = rs.randint(0, 256, (21, 37, 3))
    s = pw.random_samples(rs, 53, 37, 6, 8)
    cases = []
    for n, (cname, comp, ckw) in enumerate(fx.CODINGS):
        w, h = (200, 37, 65, 257, 33, 130)[n], (70, 53, 17, 9, 40, 5)[n]
        bm = bitmap_of(rs, n % 3, h, w)
        layout = LAYOUTS[n % len(LAYOUTS)]
        cases.append(("fax " + cname, fx.write_fax(bm, comp, photometric=n % 2, fill_order=1 + n % 2, **ckw, **layout), fx.wanted(bm, n % 2), True))
    cases.insert(2, ("png", pw.write_png(s, 6, 8, 1, [3, 4, 0, 1, 2]), pw.expected_bgr(s, 6, 8), False))
    cases.insert(4, ("lzw", tw.write_tiff(rgb, 8, tw.RGB, compression=tw.LZW, predictor=2, rows_per_strip=8), rgb[:, :, ::-1].astype(np.uint8), True))
    cases.insert(6, ("deflate", tw.write_tiff(rgb, 8, tw.RGB, compression=tw.ADOBE_DEFLATE, tile=(16, 16)), rgb[:, :, ::-1].astype(np.uint8), True))

    def run(flags, coded_prefix, env):
        args = []
        for i, (_, data, _, coded) in enumerate(cases):
            src = tmp_path / ("r%04d.bin" % i)
            src.write_bytes(data)
            args += [("coded:" if coded and coded_prefix else "") + str(src), str(tmp_path / ("r%04d.ppm" % i))]
        r = subprocess.run([tool, *flags] + args, capture_output=True, text=True, env=dict(os.environ, **env))
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        return [read_ppm(tmp_path / ("r%04d.ppm" % i)) for i in range(len(cases))], r.stdout

    models = os.path.join(ROOT, "models")
    host, _ = run([], False, {"OCR_DEVICE_TIFF": "0"})
    coded, out = run(["--stage", models], True, {"OCR_DEVICE_TIFF": "0"})
    kinds = json.loads(out.strip().splitlines()[0])["kinds"]
    assert kinds == [10, 10, 1, 10, 8, 10, 9, 10, 10], kinds
    switched, out = run(["--stage", models], False, {"OCR_DEVICE_TIFF": "4"})
    assert json.loads(out.strip().splitlines()[0])["kinds"] == kinds
    single, _ = run(["--device"], False, {"OCR_DEVICE_TIFF": "4"})
    for (name, _, want, _), a, b, c, d in zip(cases, coded, host, switched, single):
        assert a.shape == b.shape and np.array_equal(a, b) and np.array_equal(a, want), name
        assert np.array_equal(a, c) and np.array_equal(a, d), name


@pytest.mark.gpu
def test_a_frame_that_is_not_device_ok_takes_the_host_route(tool, tmp_path):
    """2^20 + 1 strips: more chunks than the device stage takes.  Under OCR_DEVICE_TIFF=4 the file is finished on the host (no
    descriptor would pass: the CPU rules test shows the ABI's refusal) and gives the pixels it gives with the switch off"""
    n = (1 << 20) + 1
    src = tmp_path / "many.tif"
    src.write_bytes(fx.many_strips(n))
    got = []
    for mode in ("4", "0"):
        r = subprocess.run([tool, "--device", str(src), str(tmp_path / ("m%s.ppm" % mode))], capture_output=True, text=True, env=dict(os.environ, OCR_DEVICE_TIFF=mode))
        assert r.returncode == 0, r.stderr[-1000:]
        got.append(read_ppm(tmp_path / ("m%s.ppm" % mode)))
    assert got[0].shape == (n, 1, 3) and (got[0] == 255).all() and np.array_equal(got[0], got[1])


@pytest.mark.gpu
def test_timing_entry_points_run(built, pkg, tool, tmp_path):
    """ocr_tiff_time_fax and ocr_tiff_time_fax_batch, through the binding and through decode_tool --time: three finite positive
    figures, and the host's scan and expansion figures beside them"""
    bm = bitmap_of(np.random.RandomState(52), 2, 70, 200)
    t = fx.to_pkg(pkg, fx.coded(bm, fx.G4, rows_per_strip=16))
    for ms in (pkg.time_tiff_fax([t], 2, single=True), pkg.time_tiff_fax([t, t, t], 2)):
        assert len(ms) == 3 and all(math.isfinite(v) and v > 0 for v in ms), ms
    src = tmp_path / "t.tif"
    src.write_bytes(fx.write_fax(bm, fx.G4, rows_per_strip=16))
    for extra, batch in (([], 1), (["3"], 3)):
        r = subprocess.run([tool, "--time", "2", str(src)] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-1000:]
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        assert rec["batch"] == batch and rec["compression"] == 4 and rec["chunks"] == 5 and rec["coded_bytes"] > 0
        for key in ("coded_upload_ms", "unfax_stage_ms", "coded_pixel_stage_ms", "host_scan_ms_per_image", "host_unfax_ms_per_image"):
            assert math.isfinite(rec[key]) and rec[key] > 0, rec


def _service(mode):
    d = tempfile.mkdtemp(prefix="ocr", dir="/tmp")
    before = os.environ.get("OCR_DEVICE_TIFF")
    if mode is None:
        os.environ.pop("OCR_DEVICE_TIFF", None)
    else:
        os.environ["OCR_DEVICE_TIFF"] = mode
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


@pytest.fixture(scope="module", params=["4", "1", "2", "3"])
def service(request, built):
    """the service under OCR_DEVICE_TIFF=4 (fax chunks handed over coded) and under =1, =2, =3 (expanded on the host thread)"""
    yield from _service(request.param)


@pytest.fixture(scope="module")
def host_service(built):
    """the service with the switch unset: every TIFF is finished on its host thread"""
    yield from _service(None)


def _same_reply(got, want):
    assert got["success"] is True and want["success"] is True, (got.get("error"), want.get("error"))
    assert got["width"] == want["width"] and got["height"] == want["height"]
    assert len(got["words"]) == len(want["words"])
    for g, w in zip(got["words"], want["words"]):
        assert g["box"] == w["box"] and g["text"] == w["text"] and g["confidence"] == w["confidence"]


@pytest.mark.gpu
def test_service_answers_fax_tiffs_like_the_same_pixels_as_png(built, card, tmp_path, service, host_service):
    """the card, made bilevel, as Group 4 strips, Group 3 two-dimensional tiles, Modified Huffman in one strip and the
    word-aligned form with FillOrder 2, by image_path and base64: every reply equals the reply the file gets with the switch
    unset, and that is the reply the same pixels get as a PNG.  A damaged fax file gets, field for field, the refusal it gets
    with the switch unset, and the refusal names the rule"""
    import png_writer as pw
    bm = (card.astype(np.int64).sum(2) < 384).astype(np.int64)
    h, w = bm.shape
    files = {"g4 strips": fx.write_fax(bm, fx.G4, rows_per_strip=16), "g3-2d tiles": fx.write_fax(bm, fx.G3, t4=1, k=4, tile=(64, 32), photometric=1),
             "mh one strip": fx.write_fax(bm, fx.MH, big_endian=True), "mhw fill order 2": fx.write_fax(bm, fx.MHW, fill_order=2, rows_per_strip=50)}
    c, ref = Client(service), Client(host_service)
    png = {0: tmp_path / "w.png", 1: tmp_path / "b.png"}
    for ph, p in png.items():
        p.write_bytes(pw.write_png(fx.wanted(bm, ph)[:, :, ::-1].astype(np.int64), 2, 8, 0, [0] * h))
    want = {ph: ref.call({"command": "recognize", "image_path": str(p)}) for ph, p in png.items()}
    assert want[0]["success"] is True and (want[0]["width"], want[0]["height"]) == (w, h) and len(want[0]["words"]) > 0
    for name, data in files.items():
        p = tmp_path / (name.replace(" ", "_") + ".tif")
        p.write_bytes(data)
        for request in ({"command": "recognize", "image_path": str(p)}, {"command": "recognize", "image_data": base64.b64encode(data).decode()}):
            unset = ref.call(request)
            _same_reply(unset, want[1 if name == "g3-2d tiles" else 0])
            _same_reply(c.call(request), unset)
    data = fx.write_fax(np.zeros((2, 16), int), fx.MH, streams=[fx.pack([("run", fx.WHITE, 20), ("run", fx.BLACK, 4), ("zeros", 16)])])
    bad = tmp_path / "bad.tif"
    bad.write_bytes(data)
    for request in ({"command": "recognize", "image_path": str(bad)}, {"command": "recognize", "image_data": base64.b64encode(data).decode()}):
        got, unset = c.call(request), ref.call(request)
        assert unset["success"] is False and "Failed to" in unset["error"] and "passes the row's width" in unset["error"]
        assert got == unset, (got, unset)
