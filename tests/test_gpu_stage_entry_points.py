"""The pipeline's staging entry points for coded images (csrc/pipe.hip): ocr_pipe_stage_jpeg, ocr_pipe_stage_jpeg_frames and
ocr_pipe_stage_coded are ocr_pipe_stage_frames under other argument lists - one staging body, ocr_pipe::stage_coded - and the
three formats' scratches share one pinned staging buffer type (csrc/image_stage.h) that is reused from call to call."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_writer as jw  # noqa: E402
import png_writer as pw  # noqa: E402
import raw_writer as rw  # noqa: E402
from test_jpeg_formats import exif, planes  # noqa: E402
from test_raw_decode import HOST, TOOL, decode_files, read_ppm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(ROOT, "models")
F420 = [(2, 2), (1, 1), (1, 1)]


@pytest.fixture(scope="module")
def tool(built):
    subprocess.check_call(["make", "-s", "-C", HOST])
    return TOOL


@pytest.mark.gpu
def test_four_entry_points_stage_the_same_bytes(tool, tmp_path):
    """One batch - a grey 8 x 8 file (one exact block), a 4:2:0 file of 17 x 23 (partial blocks, chroma sizes rounded up) and a
    4:2:0 file of 40 x 72 with EXIF orientation 6 (turned: it changes its size group) - through ocr_pipe_stage_jpeg,
    ocr_pipe_stage_jpeg_frames, ocr_pipe_stage_coded (pngs null) and ocr_pipe_stage_frames (pngs and raws null), decode_tool
    --stage-ways: every ocr_pipe_slot_image of every way equals the host decoder's pixels.  After each way the tool stages the
    batch again with an unsound second frame and exits non-zero unless that is refused with OCR_ERR_ARG; the images are read
    back after the refused call, so a refused batch left the slot as it was."""
    cases = [("grey 8x8", jw.write_jpeg(planes(8, 8, 1), [(1, 1)]), None),
             ("4:2:0 17x23", jw.write_jpeg(planes(17, 23, 3), F420, jfif=True), None),
             ("4:2:0 40x72 tag 6", jw.write_jpeg(planes(40, 72, 3), F420, jfif=True, segments=[exif(6)]), None)]
    host = decode_files(cases, tmp_path)  # jpeg::Decoder::pixels
    assert [h.shape for h in host] == [(8, 8, 3), (17, 23, 3), (72, 40, 3)]
    decode_files(cases, tmp_path, "--stage-ways", MODELS)
    for way in ("jpeg", "jpeg_frames", "coded", "frames"):
        for i, ((name, _, _), want) in enumerate(zip(cases, host)):
            got = read_ppm(tmp_path / ("r%04d.ppm.%s" % (i, way)))
            assert got.shape == want.shape and np.array_equal(got, want), (way, name)


@pytest.mark.gpu
def test_scratch_reuse_across_growth(tool, tmp_path):
    """Three consecutive ocr_pipe_stage_frames calls on one pipeline and one slot (decode_tool --stage with "--" between the
    batches), each with JPEG, PNG and BMP content: one 8 x 8 image per format, then two larger ones per format (64 x 64 and
    more), then the first batch again.  The pinned staging of each format is allocated, waited for and regrown, then found
    large enough; after each call every slot image equals the host decode of the same file."""
    rs = np.random.RandomState(61)

    def batch(sizes):
        out = []
        for rows, cols in sizes:
            rgb = rs.randint(0, 256, (rows, cols, 3)).astype(np.uint8)
            s = pw.random_samples(rs, rows, cols, 2, 8)
            out += [("jpeg %dx%d" % (rows, cols), jw.write_jpeg(planes(rows, cols, 3), F420, jfif=True), None),
                    ("png %dx%d" % (rows, cols), pw.write_png(s, 2, 8, 0, [0, 1, 2, 3, 4]), pw.expected_bgr(s, 2, 8)),
                    ("bmp %dx%d" % (rows, cols), rw.write_bmp(rgb, 24), rgb)]
        return out

    small, large = batch([(8, 8)]), batch([(64, 80), (75, 64)])
    batches = [small, large, small]
    cases = [c for b in batches for c in b]
    host = decode_files(cases, tmp_path)
    args, k = [], 0
    for j, b in enumerate(batches):
        args += ["--"] if j else []
        for _ in b:
            args += [str(tmp_path / ("r%04d.bin" % k)), str(tmp_path / ("s%04d.ppm" % k))]
            k += 1
    r = subprocess.run([tool, "--stage", MODELS] + args, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    for k, ((name, _, want), h) in enumerate(zip(cases, host)):
        got = read_ppm(tmp_path / ("s%04d.ppm" % k))
        assert got.shape == h.shape and np.array_equal(got, h), (k, name)
        if want is not None:
            assert np.array_equal(got, want), (k, name)
