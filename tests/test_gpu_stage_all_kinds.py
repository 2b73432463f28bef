"""All ten ocr_frame_kinds in ONE ocr_pipe_stage_batch call (decode_tool --stage): the path that csrc/frame_kinds.h drives -
size, bucket and decode per kind, in kFrameLaunchOrder.  The yardstick is the host route of the same files (decode_tool with
every OCR_DEVICE_* at 0); equality is byte for byte."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_writer as pw  # noqa: E402
import raw_writer as rw  # noqa: E402
import tiff_writer as tw  # noqa: E402
import vp8_writer as vw  # noqa: E402
import webp_writer as ww  # noqa: E402
from test_jpeg_orientation import pillow_exif_jpeg  # noqa: E402
from test_raw_decode import HOST, TOOL, read_ppm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JPEG, PNG, RAW, TIFF, WEBP, VP8, J2K, J2K_CODED, TIFF_CODED, TIFF_DEFLATE = range(10)  # ocr_frame_kind
HOST_ROUTE = {"OCR_DEVICE_" + f: "0" for f in ("JPEG", "PNG", "RAW", "TIFF", "WEBP", "J2K")}
# every file on its device route: a plain TIFF as expanded chunks (=2 and =3 would send an uncompressed file the coded way),
# a plain JPEG 2000 as coefficients; the coded kinds are asked for per file, "coded:<file>"
DEVICE_ROUTE = {"OCR_DEVICE_JPEG": "1", "OCR_DEVICE_PNG": "1", "OCR_DEVICE_RAW": "1", "OCR_DEVICE_TIFF": "1", "OCR_DEVICE_WEBP": "1", "OCR_DEVICE_J2K": "1"}


@pytest.fixture(scope="module")
def tool(built):
    subprocess.check_call(["make", "-s", "-C", HOST])
    return TOOL


def ten_files():
    """[(name, file bytes, "coded:" form?, kind, (rows, cols))]: 40 x 24, 24 x 40 and 17 x 33, ordered so that no two neighbours
    share a size - the slot's layout (by size) then moves most images away from their place in the batch.  The JPEG is stored
    24 x 40 and turned by its EXIF tag, so it lies in the 40 x 24 group."""
    rs = np.random.RandomState(90)
    tall, wide = (40, 24), (24, 40)

    def rgb(shape):
        return rs.randint(0, 256, shape + (3,)).astype(np.uint8)

    def webp(shape):
        coded, transforms = ww.random_case(rs, shape[1], shape[0], (ww.PREDICTOR, ww.ADD_GREEN))
        return ww.write_webp(shape[1], shape[0], coded, transforms, rs=rs)

    jp2 = open(os.path.join(ROOT, "tests", "golden", "jp2", "rgb_33x17_nomct.jp2"), "rb").read()
    idx, pal = rs.randint(0, 256, tall), rs.randint(0, 256, (256, 3))
    return [("jpeg, orientation 6", pillow_exif_jpeg(rgb(wide), 6, quality=90, subsampling=2), False, JPEG, tall),
            ("png", pw.write_png(pw.random_samples(rs, 24, 40, 2, 8), 2, 8), False, PNG, wide),
            ("jp2", jp2, False, J2K, (17, 33)),
            ("bmp", rw.write_bmp(idx, 8, palette=pal), False, RAW, tall),
            ("tiff uncompressed", tw.write_tiff(rgb(wide), 8, tw.RGB, rows_per_strip=7), False, TIFF, wide),
            ("tiff lzw", tw.write_tiff(rgb(tall), 8, tw.RGB, compression=tw.LZW, predictor=2, rows_per_strip=9), True, TIFF_CODED, tall),
            ("jp2 coded", jp2, True, J2K_CODED, (17, 33)),
            ("tiff deflate", tw.write_tiff(rgb(wide), 8, tw.RGB, compression=tw.ADOBE_DEFLATE, tile=(16, 16)), True, TIFF_DEFLATE, wide),
            ("webp lossless", webp(tall), False, WEBP, tall),
            ("webp lossy", vw.write_webp(vw.random_description(rs, 40, 24, "mix", "deltas", "dense")), False, VP8, wide)]


@pytest.mark.gpu
def test_one_stage_call_with_every_frame_kind(tool, tmp_path):
    """ten files, one of each kind, as one batch; then the same files in reverse as a second batch through the same slot of the
    same pipeline (every scratch is used again): each ocr_pipe_slot_image equals the host decode of its file"""
    files = ten_files()
    assert sorted(f[3] for f in files) == list(range(10))
    assert all(a[4] != b[4] for a, b in zip(files, files[1:])) and len({f[4] for f in files}) == 3
    src = []
    for i, (_, data, _, _, _) in enumerate(files):
        src.append(tmp_path / ("f%02d.bin" % i))
        src[-1].write_bytes(data)

    def run(flags, order, tag, env, coded_prefix):
        """decode_tool over files[k] for k in order; batch b of `order` (a list of lists) behind a "--".  Returns stdout, images"""
        args, outs = [], []
        for b, batch in enumerate(order):
            args += ["--"] if b else []
            for k in batch:
                outs.append(tmp_path / ("%s%d_%02d.ppm" % (tag, b, k)))
                args += [("coded:" if coded_prefix and files[k][2] else "") + str(src[k]), str(outs[-1])]
        r = subprocess.run([tool, *flags] + args, capture_output=True, text=True, env=dict(os.environ, **env))
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        return r.stdout, [read_ppm(p) for p in outs]

    forward, backward = list(range(10)), list(range(9, -1, -1))
    _, host = run([], [forward], "host", HOST_ROUTE, False)
    for (name, _, _, _, shape), want in zip(files, host):
        assert want.shape == shape + (3,), (name, want.shape)
    out, staged = run(["--stage", os.path.join(ROOT, "models")], [forward, backward], "dev", DEVICE_ROUTE, True)
    kinds = [json.loads(line)["kinds"] for line in out.splitlines() if line.startswith('{"kinds"')]
    assert kinds == [[files[k][3] for k in forward], [files[k][3] for k in backward]], kinds
    for b, batch in enumerate([forward, backward]):
        for k, got in zip(batch, staged[10 * b:10 * b + 10]):
            assert got.shape == host[k].shape and np.array_equal(got, host[k]), (files[k][0], "batch", b)
