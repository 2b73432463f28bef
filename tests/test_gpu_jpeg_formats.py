"""JPEG requests beyond grey / YCbCr 4:4:4, 4:2:2, 4:2:0 on the device (csrc/kernels_jpeg.hip, the general kinds, through
ocr_jpeg_decode_frame / ocr_pipe_stage_frames) and through the service.  Same case table and same expectation as the
host half, tests/test_jpeg_formats.py: Pillow's decode of the same bytes, bit for bit."""
import base64
import os
import shutil
import subprocess
import sys
import tempfile
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_writer as jw  # noqa: E402
from test_ipc_service import Client, _png_bytes, _start  # noqa: E402
from test_jpeg_formats import FAMILIES, GROUPS, case_table, check_group, decode_group, exif, expected_rgb, pillow_bytes, planes  # noqa: E402
from test_jpeg_orientation import HOST, with_segments  # noqa: E402

TILE = 64  # kJpegTile of csrc/kernels_jpeg.h


@pytest.fixture(scope="module")
def table():
    t = case_table()
    # the transposing orientations around the edge of the LDS tile, one 4:4:0 and one CMYK file
    tiles = []
    for rows, cols in ((TILE + 1, TILE), (TILE, TILE + 1)):
        cmyk = pillow_bytes(np.stack(planes(rows, cols, 4), -1), "CMYK", quality=90)
        for tag in (5, 6, 7, 8):
            tiles.append(("4:4:0 %dx%d tag %d" % (rows, cols, tag),
                          jw.write_jpeg(planes(rows, cols, 3), FAMILIES["1x2,1x1,1x1"], jfif=True, segments=[exif(tag)]), tag))
            tiles.append(("CMYK %dx%d tag %d" % (rows, cols, tag), with_segments(cmyk, exif(tag)), tag))
    t["tiles"] = tiles
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS + ["tiles"])
def test_device_decode_equals_pillow(built, table, tmp_path, group):
    """decode_tool --device on every file of the group (one process per group): the pixel half on the GPU == Pillow's
    decode (4 components: OpenCV's CMYK -> BGR on libjpeg's samples), turned as the EXIF tag says."""
    subprocess.check_call(["make", "-s", "-C", HOST])
    check_group(table[group], tmp_path, "--device")


@pytest.mark.gpu
def test_old_and_new_entry_points_agree(built, tmp_path):
    """4:4:4 / 4:2:2 / 4:2:0 / grey files, upright and turned, widths down to one chroma sample: ocr_jpeg_decode (--device)
    and ocr_jpeg_decode_frame (--frame) give the same bytes, Pillow's.  The new descriptor does not change what the old
    kinds compute."""
    from PIL import Image
    subprocess.check_call(["make", "-s", "-C", HOST])
    rs = np.random.RandomState(31)
    cases = []
    for rows, cols in ((53, 37), (TILE + 1, TILE), (9, 2), (9, 4), (9, 6)):
        arr = rs.randint(0, 256, (rows, cols, 3)).astype(np.uint8)
        for name, a, kw in (("444", arr, dict(subsampling=0)), ("422", arr, dict(subsampling=1)), ("420", arr, dict(subsampling=2)),
                            ("grey", np.array(Image.fromarray(arr).convert("L")), {})):
            plain = pillow_bytes(a, quality=88, **kw)
            for tag in (1, 3, 6):
                cases.append(("%s %dx%d tag %d" % (name, rows, cols, tag), with_segments(plain, exif(tag)), tag))
    old = decode_group(cases, tmp_path, "--device")
    new = decode_group(cases, tmp_path, "--frame")
    for (name, a), (_, b), (_, data, tag) in zip(old, new, cases):
        assert a.shape == b.shape and np.array_equal(a, b), name
        assert np.array_equal(a, expected_rgb(data, tag)), name


@pytest.mark.gpu
def test_one_stage_call_with_a_mixed_batch(built, tmp_path):
    """One ocr_pipe_stage_frames call (decode_tool --stage) with 4:2:0, 4:4:0, CMYK, grey and turned files of several
    sizes, two of them of one oriented size and not adjacent: the classic and the general kernels write one slot, the
    descriptors go to their two arrays, the layout reorders the images by size.  Every staged image, read back with
    ocr_pipe_slot_image, equals the per-file device decode and the expectation, byte for byte."""
    from PIL import Image
    subprocess.check_call(["make", "-s", "-C", HOST])
    rs = np.random.RandomState(41)
    rgb = rs.randint(0, 256, (53, 37, 3)).astype(np.uint8)
    f440, f411 = FAMILIES["1x2,1x1,1x1"], FAMILIES["4x1,1x1,1x1"]
    cases = [("4:2:0 53x37", pillow_bytes(rgb, quality=90, subsampling=2), 1),
             ("4:4:0 65x64", jw.write_jpeg(planes(TILE + 1, TILE, 3), f440, jfif=True), 1),
             ("CMYK 53x37", pillow_bytes(np.stack(planes(53, 37, 4), -1), "CMYK", quality=90), 1),
             ("grey 17x5", pillow_bytes(np.array(Image.fromarray(rgb[:17, :5]).convert("L")), quality=90), 1),
             ("4:1:1 37x53 tag 6", jw.write_jpeg(planes(37, 53, 3), f411, jfif=True, segments=[exif(6)]), 6),   # oriented 53x37
             ("4:4:4 64x65 tag 8", with_segments(pillow_bytes(rs.randint(0, 256, (TILE, TILE + 1, 3)).astype(np.uint8), quality=90, subsampling=0), exif(8)), 8),
             ("YCCK 9x4", jw.write_jpeg(planes(9, 4, 4), [(2, 2), (1, 1), (1, 1), (2, 2)], adobe=2), 1),
             ("4:2:0 9x4 (chroma 2 wide)", pillow_bytes(rgb[:9, :4], quality=90, subsampling=2), 1)]
    each = decode_group(cases, tmp_path, "--device")
    staged = decode_group(cases, tmp_path, "--stage", os.path.join(os.path.dirname(os.path.dirname(HOST)), "models"))
    for (name, a), (_, b), (_, data, tag) in zip(staged, each, cases):
        assert a.shape == b.shape and np.array_equal(a, b), name
        assert np.array_equal(a, expected_rgb(data, tag)), name


@pytest.fixture(scope="module")
def service(built):
    d = tempfile.mkdtemp(prefix="ocr", dir="/tmp")
    proc, sock = _start(d, 1)
    try:
        yield sock
        Client(sock).call({"command": "shutdown"})
        assert proc.wait(timeout=30) == 0
    finally:
        if proc.poll() is None:
            proc.kill()
        shutil.rmtree(d, ignore_errors=True)


def _same_reply(got, want):
    assert got["success"] is True and want["success"] is True, (got.get("error"), want.get("error"))
    assert got["width"] == want["width"] and got["height"] == want["height"]
    assert len(got["words"]) == len(want["words"])
    for g, w in zip(got["words"], want["words"]):
        assert g["box"] == w["box"] and g["text"] == w["text"] and g["confidence"] == w["confidence"]


def card_files(card):
    """the card as a CMYK file (Pillow), a 4:4:0 file and a 4:1:1 file with tag 6 (the writer), and two files of the old kinds"""
    from PIL import Image
    rgb = Image.fromarray(card[:, :, ::-1].copy())
    ycc = [np.ascontiguousarray(p) for p in np.array(rgb.convert("YCbCr")).transpose(2, 0, 1)]
    return {"cmyk": pillow_bytes(np.array(rgb.convert("CMYK")), "CMYK", quality=92),
            "440": jw.write_jpeg(ycc, FAMILIES["1x2,1x1,1x1"], quality=92, jfif=True),
            "411 tag 6": jw.write_jpeg(ycc, FAMILIES["4x1,1x1,1x1"], quality=92, jfif=True, segments=[exif(6)]),
            "420": pillow_bytes(np.array(rgb), quality=90, subsampling=2),
            "grey tag 6": with_segments(pillow_bytes(np.array(rgb.convert("L")), quality=90), exif(6))}


@pytest.mark.gpu
def test_service_answers_cmyk_and_440_requests(built, card, tmp_path, service):
    """A CMYK request and a 4:4:0 request, each as image_path and as base64: the reply equals the reply to a PNG request
    that carries exactly the expected pixels (width, height, words' text / confidence / box)."""
    c = Client(service)
    files = card_files(card)
    found_words = False
    for name in ("cmyk", "440"):
        jb = files[name]
        want_rgb = expected_rgb(jb)
        png = _png_bytes(np.ascontiguousarray(want_rgb[:, :, ::-1]))
        jpath, ppath = tmp_path / (name + ".jpg"), tmp_path / (name + ".png")
        jpath.write_bytes(jb)
        ppath.write_bytes(png)
        want = c.call({"command": "recognize", "image_path": str(ppath)})
        assert want["success"] is True and (want["width"], want["height"]) == (card.shape[1], card.shape[0])
        found_words = found_words or len(want["words"]) > 0
        _same_reply(c.call({"command": "recognize", "image_path": str(jpath)}), want)
        _same_reply(c.call({"command": "recognize", "image_data": base64.b64encode(jb).decode()}), want)
    assert found_words


@pytest.mark.gpu
def test_concurrent_requests_mix_old_and_new_kinds(built, card, tmp_path, service):
    """Eight concurrent JPEG requests that mix 4:2:0 and grey with CMYK, 4:4:0 and a turned 4:1:1 file (one batch on the
    device: OCRWorker::processBatch -> ocr_pipe_stage_frames): every reply equals the reply the same file gets alone,
    and that one equals the reply to the PNG of the expected pixels."""
    files = card_files(card)
    paths = []
    for name, data in files.items():
        p = tmp_path / (name.replace(" ", "_") + ".jpg")
        p.write_bytes(data)
        paths.append(str(p))
    c0 = Client(service)
    alone = [c0.call({"command": "recognize", "image_path": p}) for p in paths]
    assert all(a["success"] for a in alone) and len(alone[0]["words"]) > 0
    for (name, data), a in zip(files.items(), alone):
        tag = 6 if name.endswith("tag 6") else 1
        png = tmp_path / "want.png"
        png.write_bytes(_png_bytes(np.ascontiguousarray(expected_rgb(data, tag)[:, :, ::-1])))
        _same_reply(a, c0.call({"command": "recognize", "image_path": str(png)}))
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
