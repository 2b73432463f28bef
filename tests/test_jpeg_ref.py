"""The reference of the JPEG pixel stage (tools/jpeg_ref.py: libjpeg-turbo's jidctint.c, jdsample.c and jdcolor.c and OpenCV's
CMYK -> BGR restated in exact integers) pinned from both sides on the CPU: against Pillow (libjpeg-turbo) over files, so that
it is tied to that library and not to the code under test, and against the host pixel stage of host/jpeg_decode.h over the
descriptors of tests/jpeg_frames.CASES.  The mutation list of the reference shows which subtle errors those cases can see.
The device half is tests/test_gpu_jpeg_ops.py, over the same cases."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_frames as jf  # noqa: E402
from jpeg_frames import ref  # noqa: E402
from test_jpeg_formats import case_table, expected_rgb, pillow_bytes  # noqa: E402
from test_jpeg_orientation import oriented_cases, pillow_oriented  # noqa: E402


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("jpegpixels")
    return d, jf.build_check(d)


@pytest.fixture(scope="module")
def frames():
    return [jf.frame_of(c) for c in jf.CASES]


@pytest.fixture(scope="module")
def wanted(frames):
    return [ref.decode(fr) for fr in frames]


def frames_of_files(checker, files):
    """jpeg_check --frame over file bytes: the descriptors Decoder::decode_coefficients makes of them"""
    d, exe = checker
    args = []
    for i, data in enumerate(files):
        (d / ("f%04d.jpg" % i)).write_bytes(data)
        args += [str(d / ("f%04d.jpg" % i)), str(d / ("f%04d.bin" % i))]
    subprocess.check_call([exe, "--frame"] + args)
    return [jf.read_frames(d / ("f%04d.bin" % i))[0] for i in range(len(files))]


def test_reference_equals_pillow_on_files(card, checker):
    """every file of test_jpeg_formats.case_table(), the orientation files of test_jpeg_orientation (tags 1..8, a progressive
    one among them) and Pillow files at quality 5, 25, 50 and 100 (large and unit tables; 4:4:4, 4:2:2, 4:2:0, progressive, grey):
    jpeg_check --frame -> jpeg_ref.decode == Pillow's decode of the same bytes, byte for byte"""
    from PIL import Image
    cases = [(name, data, expected_rgb(data, tag)) for group in case_table().values() for name, data, tag in group]
    cases += [(name, data, pillow_oriented(data)) for name, data in oriented_cases(card)]
    rs = np.random.RandomState(17)
    arr = rs.randint(0, 256, (37, 53, 3)).astype(np.uint8)
    smooth = np.clip(np.add.outer(np.arange(37) * 5, np.arange(53) * 3)[:, :, None] + rs.randint(-9, 9, (37, 53, 3)), 0, 255).astype(np.uint8)
    tables = set()
    for q in (5, 25, 50, 100):
        for img in (arr, smooth):
            for kw in (dict(subsampling=0), dict(subsampling=1), dict(subsampling=2), dict(subsampling=2, progressive=True)):
                data = pillow_bytes(img, quality=q, **kw)
                cases.append(("quality %d %r" % (q, kw), data, expected_rgb(data)))
            data = pillow_bytes(np.array(Image.fromarray(img).convert("L")), quality=q)
            cases.append(("quality %d grey" % q, data, expected_rgb(data)))
    got = frames_of_files(checker, [data for _, data, _ in cases])
    for (name, _, want), fr in zip(cases, got):
        assert ref.in_domain(fr), name
        tables.add(int(max(c["quant"].max() for c in fr["comps"])))
        tables.add(int(min(c["quant"].min() for c in fr["comps"])))
        bgr = ref.decode(fr)
        assert bgr.shape == want.shape and np.array_equal(bgr[:, :, ::-1], want), name
    assert 1 in tables and 255 in tables   # quality 100 and quality 5 brought the unit table and the saturated one
    assert len(cases) > 300


def test_a_dc_of_v_minus_128_under_a_table_entry_of_8_is_flat_at_v():
    """the identity the colour-table cases of the device test stand on"""
    v = np.arange(256)
    blocks = np.zeros((256, 64), np.int64)
    blocks[:, 0] = v - 128
    quant = np.ones(64, np.int64)
    quant[0] = 8
    assert np.array_equal(ref.idct_blocks(blocks, quant), np.broadcast_to(v[:, None, None], (256, 8, 8)))
    fr = jf.colour_table_frame("ycbcr a")
    assert fr["comps"][1]["coef"].reshape(256, 256, 64)[3, 200, 0] == 200 - 128 and fr["comps"][2]["coef"].reshape(256, 256, 64)[3, 200, 0] == 3 - 128


def test_colour_arithmetic_over_its_whole_domain():
    """ycc_to_rgb (integer tables) == the float64 evaluation of jdcolor.c's decimal constants, rounded as that file rounds, for
    every (Y, Cb, Cr) - exactly, no tolerance; the eight corners by hand; cmyk_channel over every (c, k) against its definition"""
    cb, cr = np.meshgrid(np.arange(256), np.arange(256))
    for y in range(256):
        a, b = ref.ycc_to_rgb(np.full_like(cb, y), cb, cr), ref.ycc_to_rgb_float(np.full_like(cb, y), cb, cr)
        assert all(np.array_equal(p, q) for p, q in zip(a, b)), y
    corner = {(0, 0, 0): (0, 135, 0), (255, 0, 0): (76, 255, 28), (0, 255, 0): (0, 48, 225), (0, 0, 255): (178, 0, 0),
              (255, 255, 255): (255, 121, 255), (0, 255, 255): (178, 0, 225), (255, 0, 255): (255, 208, 28), (255, 255, 0): (76, 255, 255)}
    for (y, b, r), want in corner.items():
        assert tuple(int(v) for v in ref.ycc_to_rgb(np.int64(y), np.int64(b), np.int64(r))) == want, (y, b, r)
    c, k = np.meshgrid(np.arange(256), np.arange(256))
    got = ref.cmyk_channel(c, k)
    assert got.min() == 0 and got.max() == 255 and np.array_equal(got, k - np.floor((255 - c) * k / 256.0).astype(np.int64))
    assert int(ref.cmyk_channel(np.int64(255), np.int64(255))) == 255 and int(ref.cmyk_channel(np.int64(0), np.int64(255))) == 1


def test_host_pixel_stage_equals_reference(checker, frames, wanted):
    """Decoder::pixels (jpeg_check --pixels) == jpeg_ref.decode on every frame of CASES, byte for byte"""
    d, exe = checker
    for case, got, want in zip(jf.CASES, jf.host_pixels(exe, d, frames), wanted):
        assert got.shape == want.shape and np.array_equal(got, want), case["name"]
    assert len(frames) >= 250 and {c["coef"] for c in jf.CASES} == set(jf.FORMS) and {c["orient"] for c in jf.CASES} == set(range(1, 9))
    assert {c["color"] for c in jf.CASES} == set(jf.COLORS) and {c["sampling"] for c in jf.CASES} == set(jf.SAMPLINGS)
    grid = [c for c in jf.CASES if c["group"] == "grid"]
    for name in jf.SAMPLINGS:   # every size as rows and as cols with every sampling
        assert {c["rows"] for c in grid if c["sampling"] == name} == {c["cols"] for c in grid if c["sampling"] == name} == set(jf.SIZES)


def test_frame_files_round_trip(tmp_path, frames):
    jf.write_frames(tmp_path / "f.bin", frames[:40])
    for a, b in zip(frames, jf.read_frames(tmp_path / "f.bin")):
        assert {k: a[k] for k in ("rows", "cols", "color", "orientation")} == {k: b[k] for k in ("rows", "cols", "color", "orientation")}
        for p, q in zip(a["comps"], b["comps"]):
            assert all(p[k] == q[k] for k in jf.COMP) and np.array_equal(p["quant"], q["quant"]) and np.array_equal(p["coef"], q["coef"])


def test_every_mutation_shows_on_its_case(frames, wanted):
    """each entry of MUTATIONS that is not listed as equivalent changes the reference's output on the frame WITNESS names for
    it: the case table can see each of those errors before any device is involved"""
    assert set(jf.WITNESS) == set(ref.MUTATIONS) - set(ref.EQUIVALENT)
    index = {c["name"]: i for i, c in enumerate(jf.CASES)}
    for mut, name in jf.WITNESS.items():
        fr, want = frames[index[name]], wanted[index[name]]
        got = ref.decode(fr, mut)
        assert got.shape != want.shape or not np.array_equal(got, want), "mutation %s does not show on frame %r" % (mut, name)
    for mut in ref.EQUIVALENT:
        for fr, want in zip(frames, wanted):
            assert np.array_equal(ref.decode(fr, mut), want), mut


def test_frames_stay_inside_the_domain_and_extreme_ones_reach_both_clamps(frames):
    """random_frame's bound holds for every case (it asserts it itself; here again, and that the bound is what the docstring
    derives); a 16-bit table is outside; the `extreme` form drives the IDCT beyond both ends of 0..255, and both clamps answer"""
    assert ref.GAIN == 61214 and ref.DEQUANT_BOUND == ((1 << 31) - 2) * 2048 // 61214 and 32768 * 255 <= ref.DEQUANT_BOUND < 32768 * 65535
    assert all(ref.in_domain(fr) for fr in frames)
    wide = jf.random_frame(np.random.RandomState(1), 8, 8, "1x1", "grey", 1, "zero")
    wide["comps"][0]["quant"][:] = 65535
    wide["comps"][0]["coef"][:] = 32767
    assert not ref.in_domain(wide)
    seen = 0
    for case, fr in zip(jf.CASES, frames):
        if case["coef"] != "extreme":
            continue
        for c, raw, plane in zip(fr["comps"], ref.planes(fr, raw=True), ref.planes(fr)):
            if c["quant"][0] == 255 and c["bw"] * c["bh"] >= 4:
                assert raw.min() + 128 < -1000 and raw.max() + 128 > 1255, case["name"]
                assert plane.min() == 0 and plane.max() == 255 and plane[raw + 128 < 0].max() == 0 and plane[raw + 128 > 255].min() == 255
                seen += 1
    assert seen >= 20


def test_every_branch_of_the_upsampling_rules_is_met(frames):
    """the pixels per branch (jpeg_ref.branch_counts, from the geometry): positive for every branch a case says it is there for,
    and CASES together leave no branch out"""
    total = dict.fromkeys(ref.BRANCHES, 0)
    for case, fr in zip(jf.CASES, frames):
        n = ref.branch_counts(fr)
        for b in case["branches"]:
            assert n[b] > 0, (case["name"], b)
        for b, k in n.items():
            total[b] += k
    assert all(k > 0 for k in total.values()), [b for b, k in total.items() if k == 0]
    claimed = {b for c in jf.CASES for b in c["branches"]}
    assert claimed == set(ref.BRANCHES), set(ref.BRANCHES) - claimed
    dws = {(c["dw"], c["dh"]) for case, fr in zip(jf.CASES, frames) if case["group"] == "branch" for c in fr["comps"][1:]}
    assert {dw for dw, _ in dws} >= {1, 2, 3} and {dh for _, dh in dws} >= {1, 2}


def test_check_program_under_sanitizers(tmp_path, frames, wanted):
    """jpeg_check built with AddressSanitizer + UBSan (no recovery), stand-alone: --pixels over the dumped CASES ends clean with
    the reference's bytes, --frame over files of several kinds gives the descriptors the plain build gives, and a descriptor
    that breaks a rule is refused with exit status 1, not decoded"""
    exe = jf.build_check(tmp_path, "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    src, out = tmp_path / "frames.bin", tmp_path / "pixels.bin"
    jf.write_frames(src, frames)
    r = subprocess.run([exe, "--pixels", str(src), str(out)], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
    assert np.array_equal(np.fromfile(out, np.uint8), np.concatenate([w.reshape(-1) for w in wanted]))
    files = [data for group in ("four components", "orientation", "1x4,1x1,1x1") for _, data, _ in case_table()[group]]
    plain = jf.build_check(tmp_path)
    for i, data in enumerate(files):
        (tmp_path / "f.jpg").write_bytes(data)
        for e, name in ((exe, "san.bin"), (plain, "plain.bin")):
            r = subprocess.run([e, "--frame", str(tmp_path / "f.jpg"), str(tmp_path / name)], capture_output=True, text=True, env=env)
            assert r.returncode == 0 and r.stderr == "", (i, r.stderr[-3000:])
        assert (tmp_path / "san.bin").read_bytes() == (tmp_path / "plain.bin").read_bytes()
    broken = jf.frame_of(jf.CASES[0])
    broken["comps"][1]["bw"] += 1   # more blocks than coefficients
    jf.write_frames(src, [broken])
    r = subprocess.run([exe, "--pixels", str(src), str(out)], capture_output=True, text=True, env=env)
    assert r.returncode == 1 and r.stderr.startswith("refused:"), (r.returncode, r.stderr[-3000:])
