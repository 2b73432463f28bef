"""The JPEG pixel stage on the device (csrc/kernels_jpeg.hip: jpeg_idct_kernel, the classic and the general output kernels,
upright and tiled) alone, per descriptor: ocr_jpeg_decode_frame / ocr_jpeg_decode / ocr_pipe_stage_jpeg_frames on descriptors
of the tests' own making == tools/jpeg_ref.py byte for byte.  The reference is libjpeg-turbo's arithmetic restated in exact
integers; tests/test_jpeg_ref.py pins it to Pillow and to the host pixel stage, and shows on the CPU that every mutation of its
list changes the result on a frame of tests/jpeg_frames.CASES - the same frames the device decodes here."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_frames as jf  # noqa: E402
from jpeg_frames import ref  # noqa: E402

GROUPS = ["branch", "grid", "tiles", "layout"]
_wanted = {}


def wanted(case):
    """(frame, reference image) of a case, computed once for the module"""
    if case["name"] not in _wanted:
        fr = jf.frame_of(case)
        _wanted[case["name"]] = (fr, ref.decode(fr))
    return _wanted[case["name"]]


def same(got, want):
    return got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS)
def test_device_equals_reference(built, pkg, group):
    """every case of the group through ocr_jpeg_decode_frame, and through ocr_jpeg_decode where ocr_jpeg_img can hold the frame:
    the same bytes from both, the reference's.  branch: one case per rule of chroma_at / sample_at (dw 1, 2, 3, dh 1, 2, last
    column even and odd, first and last row, h1v2, every box factor), as dense and as extreme coefficients; grid: every size of
    SIZES as rows and as cols with every sampling, colours, orientations 1..8 and coefficient forms going round; tiles: the
    transposing orientations around the edges of the 64 x 64 LDS tile, classic and general kernels; layout: planes of 1, 31, 32,
    33 and 65 blocks one block wide"""
    cases = [c for c in jf.CASES if c["group"] == group]
    assert len(cases) >= 10
    both = 0
    for case in cases:
        fr, want = wanted(case)
        frame = jf.to_binding(pkg, fr)
        got = frame.decode()
        assert same(got, want), (case["name"], "ocr_jpeg_decode_frame")
        classic = frame.decode_classic()
        holds = case["color"] == "grey" or (case["color"] == "ycbcr" and case["sampling"] in ("1x1", "2x1", "2x2"))
        assert (classic is not None) == holds, case["name"]
        if holds:
            assert same(classic, got), (case["name"], "ocr_jpeg_decode")
            both += 1
    assert both >= (2 if group == "layout" else 8)


@pytest.mark.gpu
def test_one_idct_launch_over_many_planes(built, pkg):
    """one ocr_pipe_stage_jpeg_frames call with 14 descriptors: the ten layout frames (planes of 1, 31, 32, 33 and 65 blocks, grey
    and three components) between a 4:2:0, a CMYK, a turned 4:4:0 and a subsampled-luma frame - more than 20 planes in one
    jpeg_idct_kernel launch, plane boundaries inside workgroups, a block total that is no multiple of 32.  Every plane has a DC of
    its own in all its blocks, so a block taken from a neighbouring plane shows.  Every ocr_pipe_slot_image == the single
    decode of the same descriptor == the reference"""
    layout = [c for c in jf.CASES if c["group"] == "layout"]
    rs = np.random.RandomState(77)
    extra = [jf.random_frame(rs, 23, 37, "2x2", "ycbcr", 1, "dense"), jf.random_frame(rs, 17, 9, "four components", "cmyk", 1, "dense"),
             jf.random_frame(rs, 20, 33, "1x2", "ycbcr", 6, "dense"), jf.random_frame(rs, 9, 21, "subsampled luma", "ycbcr", 3, "dense")]
    frames = [jf.frame_of(c) for c in layout]
    frames = [extra[0]] + frames[:5] + [extra[1]] + frames[5:] + extra[2:]
    plane, firsts, blocks = 0, [], 0
    for fr in frames:
        for c in fr["comps"]:
            c["coef"].reshape(-1, 64)[:, 0] = (plane * 7) % 61 - 30   # distinct for up to 61 planes; under quant[0] = 16 the plane means are 2 apart at the least
            firsts.append(blocks)
            blocks += c["bw"] * c["bh"]
            plane += 1
    assert len(frames) >= 9 and plane > 20 and blocks % 32 != 0 and sum(f % 32 != 0 for f in firsts) >= 15
    want = [ref.decode(fr) for fr in frames]
    bound = [jf.to_binding(pkg, fr) for fr in frames]
    single = [b.decode() for b in bound]
    pipe = pkg.Pipe()
    try:
        pipe.stage_jpeg_frames(0, bound)
        staged = [pipe.slot_image(0, i, *b.out_shape()) for i, b in enumerate(bound)]
    finally:
        pipe.close()
    for i, (a, b, w) in enumerate(zip(staged, single, want)):
        assert same(b, w), ("single", i)
        assert same(a, w), ("staged", i)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ycbcr a", "ycbcr b", "cmyk", "ycck"])
def test_colour_tables_exhaustively(built, pkg, kind):
    """2048 x 2048 images of flat 8 x 8 blocks (a DC of v - 128 under a table entry of 8), one block per pair of table indices:
    all 65536 (Cb, Cr) pairs of ycc_to_bgr with Y running over 0..255 (the two YCbCr images together hold the eight corners of
    (Y, Cb, Cr)), all (c, k) pairs of cmyk_channel, and the (Cb, Cr) pairs again under YCCK.  device == reference, byte for byte;
    the reference's colour arithmetic itself is checked over its whole domain in tests/test_jpeg_ref.py"""
    fr = jf.colour_table_frame(kind)
    planes = [c["coef"].reshape(256, 256, 64)[:, :, 0].astype(np.int64) + 128 for c in fr["comps"]]
    if kind == "cmyk":
        assert len({(int(c), int(k)) for c, k in zip(planes[0].ravel(), planes[3].ravel())}) == 65536
    else:
        assert len({(int(b), int(r)) for b, r in zip(planes[1].ravel(), planes[2].ravel())}) == 65536
        corners = {(int(planes[0][r, b]), b, r) for b in (0, 255) for r in (0, 255)}
        assert corners == ({(0, 0, 0), (255, 255, 0), (255, 0, 255), (0, 255, 255)} if kind != "ycbcr b" else {(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 255)})
        assert all(set(row.tolist()) == set(range(256)) for row in planes[0])
    want = ref.decode(fr)
    got = jf.to_binding(pkg, fr).decode()
    assert same(got, want), kind
    if kind.startswith("ycbcr"):   # the same pixels from the decimal constants in float64
        r, g, b = ref.ycc_to_rgb_float(*planes[:3])
        assert np.array_equal(got[::8, ::8], np.stack([b, g, r], -1))


@pytest.mark.gpu
def test_every_output_byte_is_written_and_the_capacity_is_honoured(built, pkg):
    """an oriented odd-sized image into buffers pre-filled with 0xA5 and with 0x5A: both come back as the reference, so no byte of
    rows * cols * 3 keeps its fill; a capacity one byte short is refused (OCR_ERR_CAPACITY) with the buffer untouched"""
    rs = np.random.RandomState(9)
    for sampling, color, orient in (("2x2", "ycbcr", 6), ("1x2", "ycbcr", 7), ("1x1", "grey", 3), ("four components", "ycck", 8)):
        fr = jf.random_frame(rs, 67, 35, sampling, color, orient, "dense")
        want = ref.decode(fr)
        frame = jf.to_binding(pkg, fr)
        for fill in (0xA5, 0x5A):
            assert same(frame.decode(fill=fill), want), (sampling, orient, fill)
        with pytest.raises(pkg.OcrError) as e:
            frame.decode(fill=0xA5, cap=67 * 35 * 3 - 1)
        assert e.value.code == -4 and "too small" in str(e.value) and (e.value.out == 0xA5).all()
        assert same(frame.decode(fill=0xA5, cap=67 * 35 * 3), want)


def descriptor_rules(pkg):
    """every rule include/ocr_hip.h states for ocr_jpeg_frame: (a frame that breaks it, part of the message)"""
    rs = np.random.RandomState(3)
    out = []

    def rule(change, text, sampling="2x1", color="ycbcr"):
        frame = jf.to_binding(pkg, jf.random_frame(rs, 17, 20, sampling, color, 1, "dense"))
        change(frame.c)
        out.append((frame, text))

    def comp(i, key, value):
        return lambda c: setattr(c.comp[i], key, value)

    def both(*changes):
        return lambda c: [f(c) for f in changes]
    rule(lambda c: setattr(c, "color", 0), "colour space")
    rule(lambda c: setattr(c, "color", 3), "colour space")
    rule(lambda c: setattr(c, "color", 1), "colour space", "four components", "cmyk")
    rule(lambda c: setattr(c, "color", 2), "colour space", "1x1", "grey")
    rule(lambda c: setattr(c, "color", 5), "colour space")
    rule(lambda c: setattr(c, "ncomp", 2), "1, 3 or 4")
    rule(lambda c: setattr(c, "ncomp", 5), "1, 3 or 4")
    rule(comp(0, "h", 0), "outside 1..4")
    rule(comp(0, "h", 5), "outside 1..4")
    rule(comp(1, "v", 5), "outside 1..4")
    rule(comp(2, "v", 0), "outside 1..4")
    rule(comp(0, "h", 2), "single component", "1x1", "grey")
    rule(both(comp(0, "h", 3), comp(1, "h", 2)), "fractional")
    rule(both(comp(0, "v", 3), comp(1, "v", 2), comp(2, "v", 3)), "fractional")
    rule(comp(0, "bw", 2), "do not cover")          # 16 < dw = 20
    rule(comp(1, "bh", 2), "do not cover")          # 16 < dh = 17
    rule(comp(1, "dw", 11), "dw / dh")
    rule(comp(0, "dh", 16), "dw / dh")
    rule(comp(2, "bw", 0), "without coefficients")
    rule(comp(2, "coef", None), "without coefficients")
    rule(comp(0, "coef", None), "without coefficients", "1x1", "grey")
    rule(lambda c: setattr(c, "reserved", 1), "reserved")
    rule(lambda c: setattr(c, "orientation", 9), "orientation")
    rule(lambda c: setattr(c, "orientation", -1), "orientation")
    rule(lambda c: setattr(c, "rows", 0), "size")
    rule(lambda c: setattr(c, "cols", -3), "size")
    return out


@pytest.mark.gpu
def test_descriptor_rules_are_refused_before_any_device_call(built, pkg):
    """every descriptor rule -> OCR_ERR_ARG with its message and the 0xA5-filled output untouched, through ocr_jpeg_decode_frame
    and as the second frame of an ocr_pipe_stage_jpeg_frames call; the sound descriptor the rules start from decodes"""
    rules = descriptor_rules(pkg)
    for frame, text in rules:
        with pytest.raises(pkg.OcrError) as e:
            frame.decode(fill=0xA5)
        assert e.value.code == -1 and re.search(text, str(e.value)), (text, str(e.value))
        assert (e.value.out == 0xA5).all(), text
    fr = jf.random_frame(np.random.RandomState(4), 17, 20, "2x1", "ycbcr", 1, "dense")
    sound = jf.to_binding(pkg, fr)
    assert same(sound.decode(fill=0xA5), ref.decode(fr))
    pipe = pkg.Pipe()
    try:
        for frame, text in rules[::5]:
            with pytest.raises(pkg.OcrError) as e:
                pipe.stage_jpeg_frames(0, [sound, frame])
            assert re.search(text, str(e.value)), (text, str(e.value))
    finally:
        pipe.close()


@pytest.mark.gpu
def test_the_device_has_none_of_the_mutations(built, pkg):
    """for each entry of MUTATIONS (none is listed as equivalent), on the frame tests/test_jpeg_ref.py names for it: the device's
    bytes are the reference's and differ from the mutated reference's - the suite would fail if a kernel had that error"""
    assert set(jf.WITNESS) == set(ref.MUTATIONS) - set(ref.EQUIVALENT)
    for mut, name in jf.WITNESS.items():
        fr, want = wanted(jf.case_named(name))
        got = jf.to_binding(pkg, fr).decode()
        assert same(got, want), name
        assert not same(got, ref.decode(fr, mut)), (mut, name)
