"""Deflate TIFF requests, device half: csrc/kernels_inflate.hip through ocr_tiff_inflate / ocr_tiff_decode_deflate /
ocr_pipe_stage_batch (OCR_FRAME_TIFF_DEFLATE) and through the service with OCR_DEVICE_TIFF=3.  The yardstick is the host:
tiff::detail::inflate, which is zlib, run by host/tiff_check --inflate over the same streams - its verdict per chunk, its count
and its bytes; for sound streams Python's zlib as well.  Equality is exact, and so is accept / refuse.  One stream travels as
one chunk (tests/deflate_streams.frame_of), many chunks as one frame and one launch."""
import base64
import json
import math
import os
import shutil
import struct
import subprocess
import sys
import tempfile
import threading
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_streams as ds  # noqa: E402
import tiff_coded as tc  # noqa: E402
import tiff_writer as tw  # noqa: E402
from test_gpu_tiff_coded import _jpeg, _same_reply  # noqa: E402
from test_ipc_service import Client, _start  # noqa: E402
from test_raw_decode import TOOL, read_ppm  # noqa: E402
from test_tiff_decode import HOST, build_check  # noqa: E402
from test_tiff_deflate import test_deflate_rules_are_refused_before_any_device_call as _deflate_rules  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BY_NAME = {f[0]: f for f in tw.FORMS}


@pytest.fixture(scope="module")
def tool(built):
    subprocess.check_call(["make", "-s", "-C", HOST])
    return TOOL


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """host/tiff_check.cpp, a plain host program: zlib's verdicts, tiff::inflate_all and tiff::pixels"""
    d = tmp_path_factory.mktemp("tiffinflate")
    return build_check(d), d


def check_streams(pkg, checker, cases, tag, compression=tw.ADOBE_DEFLATE):
    """one frame, one launch: per chunk the device's count == the host's, the bytes == the host's up to `need` (zeros behind what
    came out, on both sides) and zeros from there to the nominal size; sound streams == zlib.decompress"""
    exe, d = checker
    host = ds.verdicts(exe, cases, d, tag)
    frame = ds.frame_of(cases, compression)
    out, produced = tc.to_pkg(pkg, frame).inflate(fill=0x5A)
    out = out.reshape(len(cases), frame["tile"][1])
    for i, ((name, need, stream), (good, count, data)) in enumerate(zip(cases, host)):
        assert int(produced[i]) == count and (int(produced[i]) == need) == good, (name, "device", int(produced[i]), "host", count, "need", need)
        ref = np.frombuffer(data, np.uint8)
        assert np.array_equal(out[i, :need], ref), (name, np.nonzero(out[i, :need] != ref)[0][:4])
        assert not out[i, need:].any(), (name, "bytes behind need")
        if good:
            try:
                assert zlib.decompressobj().decompress(stream)[:need] == data, name
            except zlib.error:
                pass  # (a fault behind `need` is not the host's business)
    return host


@pytest.mark.gpu
def test_hand_built_streams(built, pkg, checker):
    """stored blocks (LEN 0, 1, 65535, three in a row, behind a Huffman block off a byte boundary, NLEN mismatch); fixed blocks
    (literals of 1 .. 300 bytes, matches of 3 .. 258 with 258 both as 285 and as 284 + 31, distances 1 .. 65 against lengths
    around 64, 128 and 258, distance == o and o + 1, 32768 in 33000 bytes, codes 286 / 287 and 30 / 31); dynamic blocks (HCLEN 4
    and 19, 16 / 17 / 18 at their extremes and across the two sets, 16 first, a run past the end, 15-bit codes in both sets, one
    distance code, none, over-subscribed, incomplete, no end-of-block code, HLIT 287, HDIST 31); whole streams (three block
    types, bytes behind the end, no final block, each header fault, a wrong and a cut Adler-32, CINFO 0 with distance 300);
    `need` against the stream (surplus, the last match cut at 280 .. 299 for period 1 and 2, one byte short, the input cut at
    each of its last 12 bytes)"""
    cases = ds.hand_built()
    host = check_streams(pkg, checker, cases, "hand")
    verdict = {c[0]: h[0] for c, h in zip(cases, host)}
    # what the issue states outright about the host
    assert verdict["a wrong Adler-32"] and verdict["a cut trailer"] and verdict["CINFO 0 with a distance of 300"] and verdict["distance == o"]
    assert not verdict["distance == o + 1"] and not verdict["header fault: FDICT"] and not verdict["one byte short"]


@pytest.mark.gpu
def test_streams_longer_than_the_lds_window(built, pkg, checker):
    """random bytes of 3000 and 9000 at level 9, and 40 000 bytes of text, zeros, period 3 and random at levels 0 / 1 / 6 / 9 with
    the default strategy, Z_FIXED, Z_RLE, Z_HUFFMAN_ONLY and Z_FILTERED: the coded bytes exceed the window several times over;
    as Compression 32946"""
    cases = ds.refill_streams()
    assert max(len(s) for _, _, s in cases) > 8 * 2048
    host = check_streams(pkg, checker, cases, "refill", tw.DEFLATE)
    assert all(h[0] for h in host)


def geometry_cases(rs):
    out = []
    for comp in (tw.ADOBE_DEFLATE, tw.DEFLATE):
        for w in (1, 3, 17, 257):
            out.append(("rgb8", 5, w, dict(compression=comp, rows_per_strip=2)))
        out.append(("rgb8", 9, 33, dict(compression=comp, rows_per_strip=8)))   # a last strip of 1 row
        out.append(("rgb8", 17, 33, dict(compression=comp, tile=(16, 16))))
        out.append(("rgba8", 17, 33, dict(compression=comp, planar=2, rows_per_strip=4)))
        out.append(("rgb16", 17, 33, dict(compression=comp, planar=2, tile=(16, 16), big_endian=True)))
        out.append(("rgb16", 9, 33, dict(compression=comp, predictor=2, big_endian=True, rows_per_strip=8)))
        out.append(("black1", 9, 33, dict(compression=comp, rows_per_strip=8)))
        out.append(("pal4", 17, 33, dict(compression=comp, tile=(16, 16))))
    out.append(("rgba16", 17, 33, dict(compression=tw.ADOBE_DEFLATE, predictor=2, big_endian=True, planar=2, tile=(32, 16))))
    out.append(("rgb8", 9, 257, dict(compression=tw.ADOBE_DEFLATE, predictor=2, rows_per_strip=8)))
    res = []
    for name, h, w, kw in out:
        form = BY_NAME[name]
        samples, cm = tw.random_case(rs, form, h, w)
        if name == "rgb8":
            samples = np.repeat(samples[:, :(w + 3) // 4], 4, 1)[:, :w]
        comp = kw.pop("compression")
        c, expanded = tc.make_coded(samples, form, comp, colormap=cm, rs=rs, **kw)
        c["name"] = "%s %dx%d %d %s" % (name, w, h, comp, kw)
        res.append((c, expanded, tw.convert(samples, form[2], form[1], kw.get("planar", 1), form[4], cm)))
    return res


def unflat(raw):
    """a coded frame of the flat form of tiff_check --coded / --route-deflate"""
    v = struct.unpack_from("<11i", raw, 0)
    palette = np.frombuffer(raw, np.uint8, 1024, 44).reshape(256, 4)
    comp, n = struct.unpack_from("<iQ", raw, 1068)
    chunks = [struct.unpack_from("<QII", raw, 1080 + 16 * k) for k in range(n)]
    pos = 1080 + 16 * n
    (size,) = struct.unpack_from("<Q", raw, pos)
    return dict(w=v[0], h=v[1], photometric=v[2], bits=v[3], samples=v[4], planar=v[5], predictor=v[6], big_endian=v[7], premultiply=v[8], tile=(v[9], v[10]),
                palette=palette, compression=comp, chunks=chunks, data=raw[pos + 8:pos + 8 + size])


@pytest.mark.gpu
def test_geometry(built, pkg, checker, tmp_path):
    """widths 1, 3, 17 and 257, a last strip of 1 row, 16 x 16 tiles on 33 x 17, planar 2, 16 bits big-endian with the predictor,
    1-bit grey and a 4-bit palette, under both Deflate tags, and one FillOrder 2 file through tiff::parse_deflate:
    ocr_tiff_inflate == tiff::inflate_all == the chunks the writer stored, every chunk's count what its rows need, and
    ocr_tiff_decode_deflate == tiff::pixels == the numpy rules"""
    exe, d = checker
    rs = np.random.RandomState(43)
    cases = geometry_cases(rs)
    samples = np.repeat(rs.randint(0, 256, (9, 9, 3)), 4, 1)[:, :33]
    turned = tmp_path / "fill2.tif"
    turned.write_bytes(tw.write_tiff(samples, 8, tw.RGB, compression=tw.ADOBE_DEFLATE, fill_order=2, predictor=2, rows_per_strip=4))
    subprocess.check_call([exe, "--route-deflate", str(turned), str(tmp_path / "fill2.coded")], stdout=subprocess.DEVNULL)
    c = unflat(open(tmp_path / "fill2.coded", "rb").read())
    c["name"] = "FillOrder 2"
    cases.append((c, tw.frame_data(samples, 8, predictor=2, rows_per_strip=4)[0], tw.convert(samples, 8, tw.RGB, 1, None, None)))
    with open(d / "geo.coded", "wb") as f:
        for c, _, _ in cases:
            f.write(tc.flat(c))
    r = subprocess.run([exe, "--inflate-all", str(d / "geo.coded"), str(d / "geo.chunks")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-1000:]
    host, pos = np.fromfile(d / "geo.chunks", np.uint8), 0
    src, out = d / "frames.bin", d / "pixels.bin"
    with open(src, "wb") as f:
        for c, expanded, _ in cases:
            got, produced = tc.to_pkg(pkg, c).inflate(fill=0x5A)
            ref = host[pos:pos + tc.nominal(c)]
            pos += tc.nominal(c)
            assert np.array_equal(got, ref), (c["name"], int((got != ref).sum()))
            assert np.array_equal(got, np.frombuffer(expanded, np.uint8)), c["name"]
            row = len(expanded) // len(c["chunks"]) // c["tile"][1]
            assert [int(p) for p in produced] == [k[2] * row for k in c["chunks"]], c["name"]
            f.write(tc.head(c) + struct.pack("<Q", len(expanded)) + expanded)
    assert pos == len(host)
    subprocess.check_call([exe, "--pixels", str(src), str(out)])
    flat, pos = np.fromfile(out, np.uint8), 0
    for c, _, model in cases:
        ref = flat[pos:pos + model.size].reshape(model.shape)
        pos += model.size
        assert np.array_equal(ref, model), ("tiff::pixels differs from the numpy rules", c["name"])
        got = tc.to_pkg(pkg, c).decode_deflate()
        assert np.array_equal(got, ref), (c["name"], int((got != ref).sum()))
    assert pos == len(flat)


@pytest.mark.gpu
def test_64_chunks_of_different_lengths_in_one_frame(built, pkg, checker):
    """64 strips whose streams run from a few bytes to a whole row: one workgroup each, in one launch"""
    rs = np.random.RandomState(44)
    w = 700
    rows = np.zeros((64, w, 1), np.int64)
    for y in range(64):
        k = 1 + y * 11
        rows[y, :k, 0] = rs.randint(0, 256, k)
        rows[y, k:, 0] = y
    c, expanded = tc.make_coded(rows, BY_NAME["black8"], tw.ADOBE_DEFLATE, rows_per_strip=1)
    assert len(c["chunks"]) == 64 and len({k[1] for k in c["chunks"]}) > 40
    got, produced = tc.to_pkg(pkg, c).inflate(fill=0x5A)
    assert np.array_equal(got, np.frombuffer(expanded, np.uint8)) and (produced == w).all()
    assert np.array_equal(tc.to_pkg(pkg, c).decode_deflate()[:, :, 0], rows[:, :, 0])


@pytest.mark.gpu
def test_mutated_streams_are_refused_as_the_host_refuses_them(built, pkg, checker):
    """240 seeded mutations - bit flips, truncations, random bytes - of streams of 55 .. 311 bytes, a sound chunk on either side
    of each, one frame and one launch: the device's accept set is the host's, accepted bytes are the host's, every sound
    neighbour comes out untouched.  A refusal check, not a stress run: at least a tenth refused and a tenth accepted, on the
    host's verdicts alone"""
    corpus = ds.fuzz_corpus()
    exe, d = checker
    alone = ds.verdicts(exe, corpus, d, "fuzz_alone")
    good = sum(v[0] for v in alone)
    assert len(corpus) == 240 and good * 10 >= len(corpus) and (len(corpus) - good) * 10 >= len(corpus), good
    text = (ds.TEXT * 3)[:200]
    sound = ("sound", len(text), ds.deflate(text))
    cases = [sound]
    for c in corpus:
        cases += [c, sound]
    host = check_streams(pkg, checker, cases, "fuzz")
    assert [h[0] for h in host[1::2]] == [v[0] for v in alone]
    assert all(h[0] and h[2] == text for h in host[0::2])


@pytest.mark.gpu
def test_one_stage_call_with_deflate_tiffs_lzw_tiffs_a_jpeg_and_a_png(tool, tmp_path):
    """One ocr_pipe_stage_batch call (decode_tool --stage) with Deflate frames ("coded:<file>": OCR_FRAME_TIFF_DEFLATE), LZW coded
    frames, a JPEG and a PNG: every ocr_pipe_slot_image equals the OCR_DEVICE_TIFF=0 decode; --stage and --device under
    OCR_DEVICE_TIFF=3 give the same; the same batch with one faulty Deflate chunk is refused, naming frame and chunk"""
    import png_writer as pw
    rs = np.random.RandomState(45)
    rgb = rs.randint(0, 256, (53, 37, 3)).astype(np.uint8)
    s = pw.random_samples(rs, 53, 37, 6, 8)

    def tiff(name, h, w, **kw):
        form = BY_NAME[name]
        samples, cm = tw.random_case(rs, form, h, w)
        return ("tiff " + name, tw.write_tiff(samples, form[2], form[1], extra=form[4], colormap=cm, rs=rs, **kw), tw.convert(samples, form[2], form[1], kw.get("planar", 1), form[4], cm), True)

    tiffs = [tiff("rgb8", 53, 37, compression=tw.ADOBE_DEFLATE, predictor=2, rows_per_strip=8), tiff("pal8", 53, 37, compression=tw.DEFLATE, tile=(16, 16)),
             tiff("rgb8", 53, 37, compression=tw.LZW, predictor=2, rows_per_strip=8), tiff("rgba16", 53, 37, compression=tw.ADOBE_DEFLATE, predictor=2, big_endian=True, planar=2, tile=(32, 16)),
             tiff("white1", 70, 200, compression=tw.ADOBE_DEFLATE, rows_per_strip=16), tiff("pal4", 17, 33, compression=tw.LZW),
             tiff("rgb8", 9, 257, compression=tw.ADOBE_DEFLATE, fill_order=2, rows_per_strip=8)]
    others = [("4:2:0 37x53", _jpeg(rgb, quality=90, subsampling=2), None, False),
              ("RGBA 8 interlaced 37x53", pw.write_png(s, 6, 8, 1, [3, 4, 0, 1, 2]), pw.expected_bgr(s, 6, 8), False)]
    cases = tiffs[:3] + others[:1] + tiffs[3:5] + others[1:] + tiffs[5:]

    def run(flags, coded_prefix, env=None, files=cases, ok=True):
        args = []
        for i, (_, data, _, coded) in enumerate(files):
            src = tmp_path / ("r%04d.bin" % i)
            src.write_bytes(data)
            args += [("coded:" if coded and coded_prefix else "") + str(src), str(tmp_path / ("r%04d.ppm" % i))]
        r = subprocess.run([TOOL, *flags] + args, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
        if not ok:
            return r
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        return [read_ppm(tmp_path / ("r%04d.ppm" % i)) for i in range(len(files))]

    models = os.path.join(ROOT, "models")
    host = run([], False, {"OCR_DEVICE_TIFF": "0"})
    coded = run(["--stage", models], True)
    switched = run(["--stage", models], False, {"OCR_DEVICE_TIFF": "3"})
    single = run(["--device"], False, {"OCR_DEVICE_TIFF": "3"})
    for (name, _, want, _), a, b, c, d in zip(cases, coded, host, switched, single):
        assert a.shape == b.shape and np.array_equal(a, b), name
        assert np.array_equal(a, c) and np.array_equal(a, d), name
        if want is not None:
            assert np.array_equal(a, want), name
    # frame 5 of the batch (white1: 70 rows in strips of 16) with its third strip's stream one byte short
    samples, _ = tw.random_case(rs, BY_NAME["white1"], 70, 200)
    good = tc.make_coded(samples, BY_NAME["white1"], tw.ADOBE_DEFLATE, rows_per_strip=16)[0]
    streams = [good["data"][o:o + n] for o, n, _ in good["chunks"]]
    streams[2] = zlib.compress(zlib.decompress(streams[2])[:-1])
    bad = list(cases)
    bad[5] = ("faulty", tw.write_tiff(samples, 1, tw.MINISWHITE, compression=tw.ADOBE_DEFLATE, rows_per_strip=16, streams=streams), None, True)
    r = run(["--stage", models], True, files=bad, ok=False)
    assert r.returncode == 1 and "deflate: a chunk's stream does not hold the bytes its rows need (frame 5, chunk 2)" in r.stderr, r.stderr[-1000:]


@pytest.mark.gpu
def test_deflate_rules_reach_no_launch(built, pkg):
    """every structural rule -> OCR_ERR_ARG with its message and the output buffer untouched (the CPU test, on the machine that
    could launch); a sound frame decodes; a stream one byte short is the stream refusal of ocr_tiff_decode_deflate, while
    ocr_tiff_inflate reports it in `produced`"""
    _deflate_rules(built, pkg)
    samples = np.random.RandomState(7).randint(0, 256, (5, 4, 3))
    c, _ = tc.make_coded(samples, BY_NAME["rgb8"], tw.ADOBE_DEFLATE, rows_per_strip=3)
    assert np.array_equal(tc.to_pkg(pkg, c).decode_deflate(), samples[:, :, ::-1])
    (o0, l0, r0), (o1, l1, r1) = c["chunks"]
    short = zlib.compress(zlib.decompress(c["data"][o1:o1 + l1])[:-1])
    c2 = dict(c, chunks=[(o0, l0, r0), (l0, len(short), r1)], data=c["data"][:l0] + short)
    with pytest.raises(pkg.OcrError, match=r"deflate: a chunk's stream does not hold the bytes its rows need \(frame 0, chunk 1\)") as e:
        tc.to_pkg(pkg, c2).decode_deflate()
    assert e.value.code == -1
    _, produced = tc.to_pkg(pkg, c2).inflate()
    assert [int(p) for p in produced] == [36, 23]


@pytest.mark.gpu
def test_timing_entry_points_run(built, pkg, tool, tmp_path):
    """ocr_tiff_time_deflate and ocr_tiff_time_deflate_batch, through the binding and through decode_tool --time: three finite
    positive figures, and the host's zlib figure beside them"""
    rs = np.random.RandomState(51)
    samples = np.repeat(rs.randint(0, 256, (70, 50, 3)), 4, 1)
    c, _ = tc.make_coded(samples, BY_NAME["rgb8"], tw.ADOBE_DEFLATE, predictor=1, rows_per_strip=16)
    t = tc.to_pkg(pkg, c)
    for ms in (pkg.time_tiff_deflate([t], 2, single=True), pkg.time_tiff_deflate([t, t, t], 2)):
        assert len(ms) == 3 and all(math.isfinite(v) and v > 0 for v in ms), ms
    src = tmp_path / "t.tif"
    src.write_bytes(tw.write_tiff(samples, 8, tw.RGB, compression=tw.ADOBE_DEFLATE, predictor=2, rows_per_strip=16))
    for extra, batch in (([], 1), (["3"], 3)):
        r = subprocess.run([tool, "--time", "2", str(src)] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-1000:]
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        assert rec["batch"] == batch and rec["compression"] == 8 and rec["chunks"] == 5 and rec["coded_bytes"] > 0
        for key in ("coded_upload_ms", "inflate_stage_ms", "coded_pixel_stage_ms", "host_inflate_ms_per_image"):
            assert math.isfinite(rec[key]) and rec[key] > 0, rec


def _service(mode):
    d = tempfile.mkdtemp(prefix="ocr", dir="/tmp")
    before = os.environ.get("OCR_DEVICE_TIFF")
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


@pytest.fixture(scope="module")
def service(built):
    """the service with the Deflate chunks, the other expansions and the pixel stage on the device (OCR_DEVICE_TIFF=3)"""
    yield from _service("3")


@pytest.fixture(scope="module")
def host_service(built):
    """the service that finishes every TIFF on its host thread (OCR_DEVICE_TIFF=0)"""
    yield from _service("0")


@pytest.mark.gpu
def test_service_answers_deflate_tiffs_like_the_same_pixels_as_png(built, card, tmp_path, service, host_service):
    """TIFF `recognize` requests under OCR_DEVICE_TIFF=3 - Deflate strips with the predictor, Deflate tiles big-endian, a 32946
    file - by image_path and base64: "success":true and the reply the same pixels get as a PNG.  A Deflate file with a stream
    one byte short: the reply, field for field, that a service under OCR_DEVICE_TIFF=0 gives for it"""
    import png_writer as pw
    c = Client(service)
    rgb = card[:, :, ::-1].astype(np.int64)
    h, w = rgb.shape[:2]
    files = {"strips deflate predictor": tw.write_tiff(rgb, 8, tw.RGB, compression=tw.ADOBE_DEFLATE, predictor=2, rows_per_strip=16),
             "tiles deflate big-endian": tw.write_tiff(rgb, 8, tw.RGB, big_endian=True, compression=tw.ADOBE_DEFLATE, predictor=2, tile=(64, 32)),
             "strips 32946": tw.write_tiff(rgb, 8, tw.RGB, compression=tw.DEFLATE, rows_per_strip=50),
             "png": pw.write_png(rgb.reshape(h, w, 3), 2, 8, 0, [0] * h)}
    paths = {}
    for name, data in files.items():
        p = tmp_path / (name.replace(" ", "_") + ".bin")
        p.write_bytes(data)
        paths[name] = str(p)
    want = c.call({"command": "recognize", "image_path": paths["png"]})
    assert want["success"] is True and (want["width"], want["height"]) == (w, h) and len(want["words"]) > 0
    for name, data in files.items():
        if name == "png":
            continue
        _same_reply(c.call({"command": "recognize", "image_path": paths[name]}), want)
        if len(data) * 4 // 3 < 1000000:
            _same_reply(c.call({"command": "recognize", "image_data": base64.b64encode(data).decode()}), want)
    small = rgb[:8, :8]
    bad = tmp_path / "short.tif"
    data = tw.write_tiff(small, 8, tw.RGB, compression=tw.ADOBE_DEFLATE, streams=[zlib.compress(small.astype(np.uint8).tobytes()[:-1])])
    bad.write_bytes(data)
    for request in ({"command": "recognize", "image_path": str(bad)}, {"command": "recognize", "image_data": base64.b64encode(data).decode()}):
        got, ref = c.call(request), Client(host_service).call(request)
        assert ref["success"] is False and "Failed to" in ref["error"]
        assert got == ref, (got, ref)


@pytest.mark.gpu
def test_a_faulty_deflate_tiff_fails_alone_in_a_batch_with_host_pixels(built, card, tmp_path, service, host_service):
    """Eight concurrent requests under OCR_DEVICE_TIFF=3 (one batch: OCRWorker::processBatch), twice: a Deflate TIFF with a
    stream one byte short, a BMP - host pixels, so the batch takes the host path and every image is materialised there - a
    sound Deflate TIFF and a PNG.  The faulty file gets the reply a service under OCR_DEVICE_TIFF=0 gives it; every other
    request gets the reply its file gets alone"""
    import png_writer as pw
    import raw_writer as rw
    rgb = card[:, :, ::-1].astype(np.int64)
    h, w = rgb.shape[:2]
    files = {"short.tif": tw.write_tiff(rgb, 8, tw.RGB, compression=tw.ADOBE_DEFLATE, streams=[zlib.compress(rgb.astype(np.uint8).tobytes()[:-1])]),
             "card.bmp": rw.write_bmp(card, 24),
             "sound.tif": tw.write_tiff(rgb, 8, tw.RGB, compression=tw.ADOBE_DEFLATE, predictor=2, rows_per_strip=16),
             "card.png": pw.write_png(rgb.reshape(h, w, 3), 2, 8, 0, [0] * h)}
    paths = []
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
        paths.append(str(tmp_path / name))
    c0 = Client(service)
    alone = [c0.call({"command": "recognize", "image_path": p}) for p in paths]
    ref = Client(host_service).call({"command": "recognize", "image_path": paths[0]})
    assert ref["success"] is False and "Failed to" in ref["error"] and alone[0] == ref
    assert all(a["success"] for a in alone[1:]) and len(alone[1]["words"]) > 0
    nthreads = 8
    for _ in range(2):
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
            if k == 0:
                assert got == ref, (got, ref)
            else:
                _same_reply(got, alone[k])
