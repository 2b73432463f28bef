"""EXIF orientation of JPEG requests on the device (csrc/kernels_jpeg.hip: per pixel for tags 1..4, by LDS tiles for the
transposing tags 5..8) and through the service.  The pixels are pinned to Pillow's ImageOps.exif_transpose bit for bit, the
service's replies to those of PNG requests that carry exactly the oriented pixels.  The host half and the helpers are in
tests/test_jpeg_orientation.py."""
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
from test_ipc_service import Client, _png_bytes, _start  # noqa: E402
from test_jpeg_orientation import HOST, TOOL, hand_exif_jpeg, jpeg_bytes, pillow_exif_jpeg, pillow_oriented  # noqa: E402

TILE = 64  # kJpegTile of csrc/kernels_jpeg.h: the side of the square of stored pixels one workgroup transposes
# rows x cols: one pixel; fewer rows than a tile and three tiles of columns; smaller than a tile in both; one row / one
# column more than a tile; several tiles with partial ones at the right and bottom edges
SIZES = [(1, 1), (3, 130), (53, 37), (TILE + 1, TILE), (TILE, TILE + 1), (333, 517)]
SAMPLINGS = {"444": dict(subsampling=0), "422": dict(subsampling=1), "420": dict(subsampling=2), "grey": None}


def test_tile_side_is_the_kernels():
    hdr = open(os.path.join(os.path.dirname(HOST), "csrc", "kernels_jpeg.h")).read()
    assert "constexpr int kJpegTile = %d;" % TILE in hdr


@pytest.mark.gpu
@pytest.mark.parametrize("sampling", list(SAMPLINGS))
def test_device_decode_applies_exif_orientation(built, tmp_path, sampling):
    """decode_tool --device, tags 1..8 at sizes around the tile edges: equal to exif_transpose of Pillow's decode, bit for
    bit.  One process decodes all files of a sampling."""
    from PIL import Image
    subprocess.check_call(["make", "-s", "-C", HOST])
    rs = np.random.RandomState(21)
    args, wants = [], []
    for rows, cols in SIZES:
        arr = rs.randint(0, 256, (rows, cols, 3)).astype(np.uint8)
        if rows * cols > 4096:  # (a smooth part too: noise alone saturates many pixels)
            arr[: rows // 2] = (np.add.outer(np.arange(rows // 2) * 3, np.arange(cols) * 2)[:, :, None] // (1, 2, 3)) % 256
        kw = SAMPLINGS[sampling]
        if kw is None:
            arr, kw = np.array(Image.fromarray(arr).convert("L")), {}
        plain = jpeg_bytes(arr, quality=88, **kw)
        for tag in range(1, 9):
            data = hand_exif_jpeg(plain, "II", tag) if tag % 2 else pillow_exif_jpeg(arr, tag, quality=88, **kw)
            src, dst = tmp_path / ("%dx%d_%d.jpg" % (rows, cols, tag)), tmp_path / ("%dx%d_%d.ppm" % (rows, cols, tag))
            src.write_bytes(data)
            args += [str(src), str(dst)]
            wants.append(((rows, cols, tag), dst, pillow_oriented(data)))
    r = subprocess.run([TOOL, "--device"] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for case, dst, want in wants:
        got = np.array(Image.open(dst))
        assert got.shape == want.shape, (case, got.shape, want.shape)
        assert np.array_equal(got, want), case


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
    assert got["success"] is True and want["success"] is True
    assert got["width"] == want["width"] and got["height"] == want["height"]
    assert len(got["words"]) == len(want["words"])
    for g, w in zip(got["words"], want["words"]):
        assert g["box"] == w["box"] and g["text"] == w["text"] and g["confidence"] == w["confidence"]


@pytest.mark.gpu
def test_service_answers_in_the_upright_frame(built, card, tmp_path, service):
    """The card JPEG with Orientation 6 and 3, as base64 and as a path, against PNG requests that carry exactly the
    pixels exif_transpose gives: width, height and words (text, confidence, boxes) are identical; with tag 6 width and
    height are swapped relative to the stored size."""
    c = Client(service)
    rgb = card[:, :, ::-1].copy()
    found_words = False
    for tag in (6, 3):
        jb = pillow_exif_jpeg(rgb, tag, quality=92)
        upright = pillow_oriented(jb)
        png = _png_bytes(np.ascontiguousarray(upright[:, :, ::-1]))
        jpath, ppath = tmp_path / ("card%d.jpg" % tag), tmp_path / ("card%d.png" % tag)
        jpath.write_bytes(jb)
        ppath.write_bytes(png)
        want = c.call({"command": "recognize", "image_path": str(ppath)})
        assert want["success"] is True
        if tag == 6:
            assert (want["width"], want["height"]) == (card.shape[0], card.shape[1])
        else:
            assert (want["width"], want["height"]) == (card.shape[1], card.shape[0])
        found_words = found_words or len(want["words"]) > 0
        _same_reply(c.call({"command": "recognize", "image_data": base64.b64encode(png).decode()}), want)
        _same_reply(c.call({"command": "recognize", "image_path": str(jpath)}), want)
        _same_reply(c.call({"command": "recognize", "image_data": base64.b64encode(jb).decode()}), want)
    assert found_words


@pytest.mark.gpu
def test_concurrent_jpegs_of_several_orientations(built, card, tmp_path, service):
    """A burst of JPEG-only requests (decoded on the device as one batch: OCRWorker::processBatch -> ocr_pipe_stage_frames)
    that mixes tags 1, 6 and 8; the card as stored and its transpose stored with tag 6 have the same oriented size and
    share a size group.  Every reply equals the reply the same file gets alone."""
    rgb = card[:, :, ::-1].copy()
    sideways = np.ascontiguousarray(rgb[:, ::-1].transpose(1, 0, 2))  # what a camera held upright stores: tag 6 undoes it
    files = {"tag1": pillow_exif_jpeg(rgb, 1, quality=90, subsampling=2),
             "tag6 sideways": pillow_exif_jpeg(sideways, 6, quality=90, subsampling=2),
             "tag8": pillow_exif_jpeg(rgb, 8, quality=90, subsampling=0),
             "tag6": pillow_exif_jpeg(rgb, 6, quality=90, subsampling=1)}
    paths = []
    for name, data in files.items():
        p = tmp_path / (name.replace(" ", "_") + ".jpg")
        p.write_bytes(data)
        paths.append(str(p))
    c0 = Client(service)
    alone = [c0.call({"command": "recognize", "image_path": p}) for p in paths]
    assert all(a["success"] for a in alone) and len(alone[0]["words"]) > 0
    assert (alone[0]["width"], alone[0]["height"]) == (alone[1]["width"], alone[1]["height"]) == (card.shape[1], card.shape[0])
    assert (alone[2]["width"], alone[2]["height"]) == (alone[3]["width"], alone[3]["height"]) == (card.shape[0], card.shape[1])
    nthreads, rounds = 8, 2
    out = [[None] * rounds for _ in range(nthreads)]

    go = threading.Barrier(nthreads)

    def work(t):
        c = Client(service)
        go.wait(timeout=60)  # connected clients send together: the worker finds the others queued behind the first request
        for r in range(rounds):
            k = (t + r) % len(paths)
            out[t][r] = (k, c.call({"command": "recognize", "image_path": paths[k]}))

    th = [threading.Thread(target=work, args=(t,)) for t in range(nthreads)]
    [t.start() for t in th]
    [t.join() for t in th]
    batches = {}  # the replies of one batched run carry that run's wall time (OCRWorker::processBatch), all 17 digits of it
    for t in range(nthreads):
        for r in range(rounds):
            k, got = out[t][r]
            _same_reply(got, alone[k])
            batches.setdefault(got["processing_time_ms"], set()).add(k)
    # the burst was not served one request at a time: one device-decoded batch held an as-stored image next to a
    # transposed one (both pixel kernels in one launch pair), and one held the two files of the same oriented size
    assert any(0 in ks and (ks & {1, 2, 3}) for ks in batches.values()), sorted(map(sorted, batches.values()))
    assert any({0, 1} <= ks for ks in batches.values()), sorted(map(sorted, batches.values()))
