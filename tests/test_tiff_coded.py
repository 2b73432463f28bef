"""TIFF requests before the expansion, host half (host/tiff_decode.h): tiff::parse_coded + tiff::expand give the bytes
tiff::parse gives (which tests/test_tiff_decode.py pins against libtiff); the extent scans lzw_extent / packbits_extent say what
the expanders unlzw / unpack_bits say; every rule of coded_fault is refused with its message before the runtime is touched.
The decoder runs in host/tiff_check.cpp, a plain host program built with -fsanitize=address,undefined - nothing of it is
loaded into Python.  The device half is tests/test_gpu_tiff_coded.py."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiff_coded as tc  # noqa: E402
import tiff_writer as tw  # noqa: E402
from test_tiff_decode import build_check  # noqa: E402


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """host/tiff_check.cpp with AddressSanitizer and UBSan: a stand-alone host program"""
    return build_check(tmp_path_factory.mktemp("tiffcoded"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return r


def test_parse_coded_and_expand_give_the_bytes_of_parse(checker, tmp_path):
    """every form x {none, PackBits, LZW} x {strips, tiles}: Frame::data of parse_coded + expand == Frame::data of parse, byte
    for byte, and both are the chunks the writer stored (a short last strip zero-filled); FillOrder 2 and a Deflate file (the
    other route) beside them"""
    rs = np.random.RandomState(11)
    files, want, k = [], [], 0
    for form in tw.FORMS:
        name, photometric, bits, spp, extra = form
        for comp in (tw.NONE, tw.PACKBITS, tw.LZW):
            for layout in ("strips", "tiles"):
                k += 1
                h, w = (5, 17, 33)[k % 3], (3, 31, 65)[(k // 3) % 3]
                samples, colormap = tw.random_case(rs, form, h, w)
                kw = dict(big_endian=bool(k & 1), compression=comp)
                if comp == tw.LZW and bits >= 8 and k % 3:
                    kw["predictor"] = 2
                if layout == "strips":
                    kw["rows_per_strip"] = (None, 1, 2, 4)[k % 4]
                else:
                    kw["tile"] = ((16, 16), (32, 16))[k % 2]
                if k % 7 == 0:
                    kw["fill_order"] = 2
                if bits >= 8 and (photometric == tw.RGB or (photometric <= 1 and spp >= 2)) and k % 2:
                    kw["planar"] = 2
                files.append(tw.write_tiff(samples, bits, photometric, extra=extra, colormap=colormap, **kw))
                geo = {a: b for a, b in kw.items() if a in ("planar", "predictor", "tile", "rows_per_strip", "big_endian")}
                want.append(tw.frame_data(samples, bits, **geo)[0])
    assert len(files) == len(tw.FORMS) * 6
    args_chunks, args_coded = [], []
    for i, data in enumerate(files):
        p = str(tmp_path / ("f%03d.tif" % i))
        open(p, "wb").write(data)
        args_chunks += [p, p + ".chunks"]
        args_coded += [p, p + ".coded"]
    assert run(checker, "--chunks", *args_chunks).returncode == 0
    assert run(checker, "--coded", *args_coded).returncode == 0
    with open(tmp_path / "all.coded", "wb") as f:
        for i in range(len(files)):
            f.write(open(args_coded[2 * i + 1], "rb").read())
    assert run(checker, "--expand", str(tmp_path / "all.coded"), str(tmp_path / "all.chunks")).returncode == 0
    got = open(tmp_path / "all.chunks", "rb").read()
    pos = 0
    for i, w in enumerate(want):
        parsed = open(args_chunks[2 * i + 1], "rb").read()
        assert parsed == w, ("parse differs from the stored chunks", i)
        assert got[pos:pos + len(w)] == w, ("parse_coded + expand differs from parse", i)
        pos += len(w)
    assert pos == len(got)
    # the routes: Deflate goes through parse, a refused file is refused
    samples = rs.randint(0, 256, (4, 4, 3))
    names = {"lzw.tif": tw.write_tiff(samples, 8, tw.RGB, compression=tw.LZW), "deflate.tif": tw.write_tiff(samples, 8, tw.RGB, compression=tw.ADOBE_DEFLATE),
             "ccitt.tif": tw.write_tiff(np.zeros((4, 4, 1), int), 1, tw.MINISWHITE, drop=(259,), more_tags=[(259, tw.SHORT, [4])]),
             "short.tif": tw.write_tiff(samples, 8, tw.RGB, compression=tw.LZW, streams=[tw.lzw_encode(bytes(47))])}
    for n, data in names.items():
        open(tmp_path / n, "wb").write(data)
    r = run(checker, "--why", *[str(tmp_path / n) for n in names])
    assert r.returncode == 0
    assert [line.rsplit(": ", 1)[1] for line in r.stdout.strip().splitlines()] == ["ok", "other route", "refused", "refused"]
    assert run(checker, "--coded", str(tmp_path / "deflate.tif"), str(tmp_path / "d.coded")).returncode == 3
    assert run(checker, "--coded", str(tmp_path / "short.tif"), str(tmp_path / "s.coded")).returncode == 1
    assert run(checker, "--chunks", str(tmp_path / "short.tif"), str(tmp_path / "s.chunks")).returncode == 1


def test_extent_scans_agree_with_the_expanders(checker, tmp_path):
    """2400 streams - LZW and PackBits, cut, bit-flipped and byte-spliced, and pure random bytes - with `need` at, below and above
    what the sound stream holds: lzw_extent / packbits_extent answer what unlzw / unpack_bits answer, in the sanitizer build (a
    read past a stream or a write past `need` is its to see).  Both answers occur; a tenth of the cases at least are accepted."""
    cases = tc.corpus()
    assert len(cases) >= 2000
    with open(tmp_path / "streams.bin", "wb") as f:
        for comp, need, stream in cases:
            f.write(struct.pack("<III", comp, need, len(stream)) + stream)
    assert run(checker, "--extents", str(tmp_path / "streams.bin"), str(tmp_path / "verdicts.bin")).returncode == 0
    v = np.fromfile(tmp_path / "verdicts.bin", np.uint8).reshape(-1, 2)
    assert len(v) == len(cases)
    differ = np.nonzero(v[:, 0] != v[:, 1])[0]
    assert len(differ) == 0, [(int(i), cases[i][0], cases[i][1], len(cases[i][2])) for i in differ[:5]]
    for comp in (tw.LZW, tw.PACKBITS):
        mine = v[[c[0] == comp for c in cases], 1]
        print("compression %d: %d streams, %d accepted" % (comp, len(mine), int(mine.sum())))
        assert mine.sum() * 10 >= len(mine) and (mine == 0).sum() * 10 >= len(mine), (comp, int(mine.sum()), len(mine))


def test_expand_over_mutated_frames_under_the_sanitizers(checker, tmp_path):
    """tiff::expand over coded frames whose streams are the mutated corpus, and over frames with broken records: accepted or
    refused, never a sanitizer report"""
    rs = np.random.RandomState(6)
    cases = tc.corpus(seed=8, count=800)
    with open(tmp_path / "all.coded", "wb") as f:
        for comp, need, stream in cases:
            c = tc.grey_strip(stream, need, comp)
            if rs.randint(8) == 0:
                c["chunks"] = [(int(rs.randint(0, 2 * len(stream) + 1)), int(rs.randint(0, 2 * len(stream) + 1)), int(rs.randint(0, 3)))]
            f.write(tc.flat(c))
    r = run(checker, "--expand", str(tmp_path / "all.coded"), str(tmp_path / "all.chunks"))
    assert r.returncode in (0, 1), (r.returncode, r.stderr[-2000:])
    answers = r.stdout.split()
    assert len(answers) == len(cases) and answers.count("ok") > 50 and answers.count("refused") > 50, (len(answers), answers.count("ok"))


def coded(pkg, **kw):
    """a sound 4 x 5 RGB frame in two LZW strips, fields changed by name"""
    samples = np.random.RandomState(3).randint(0, 256, (5, 4, 3))
    c, _ = tc.make_coded(samples, tw.FORMS[16], kw.pop("compression", tw.LZW), rows_per_strip=3)
    for name in ("chunks", "data"):
        if name in kw:
            c[name] = kw.pop(name)
    t = tc.to_pkg(pkg, c)
    for name, value in kw.items():
        if name == "frame_data":
            t.c.frame.data, t.c.frame.data_len = t.data.ctypes.data, 60
        elif name in ("compression", "chunks_len", "bytes_len", "bytes"):
            setattr(t.c, name, value)
        else:
            setattr(t.c.frame, name, value)
    return t, c


def test_coded_rules_are_refused_before_any_device_call(built, pkg):
    """every rule of ocr_tiff_coded drives ocr_tiff_expand and ocr_tiff_decode_coded to OCR_ERR_ARG with a message that names
    it - on a machine with or without a GPU: the check comes before the runtime is touched, so nothing was launched and the
    output buffer is as it was"""
    def refused_as(t, what):
        for call in (t.expand, t.decode):
            with pytest.raises(pkg.OcrError, match=what) as e:
                call(fill=0xA5)
            assert e.value.code == -1  # OCR_ERR_ARG
            assert (e.value.out == 0xA5).all()

    _, sound = coded(pkg)
    (o0, l0, r0), (o1, l1, r1) = sound["chunks"]
    assert (r0, r1) == (3, 2)
    refused_as(coded(pkg, bits_per_sample=3)[0], "bits per sample")                       # fault()
    refused_as(coded(pkg, width=0)[0], "positive")
    refused_as(coded(pkg, frame_data=True)[0], "carries no expanded chunks")
    refused_as(coded(pkg, compression=8)[0], "compression must be 1")
    refused_as(coded(pkg, compression=7)[0], "compression must be 1")
    refused_as(coded(pkg, chunks_len=1)[0], "as many chunk records")
    refused_as(coded(pkg, chunks=sound["chunks"] + [(0, 1, 1)])[0], "as many chunk records")
    refused_as(coded(pkg, chunks=[(o0, l0, 0), (o1, l1, r1)])[0], "rows must be 1 .. tile_height")
    refused_as(coded(pkg, chunks=[(o0, l0, 4), (o1, l1, r1)])[0], "rows must be 1 .. tile_height")
    refused_as(coded(pkg, chunks=[(o0, l0, r0), (o1, l1 + 1, r1)])[0], "outside the pool")
    refused_as(coded(pkg, chunks=[(o0, l0, r0), (len(sound["data"]) + 1, 0, r1)])[0], "outside the pool")
    refused_as(coded(pkg, chunks=[((1 << 64) - 1, 2, r0), (o1, l1, r1)])[0], "outside the pool")
    refused_as(coded(pkg, bytes_len=len(sound["data"]) - 1)[0], "outside the pool")
    refused_as(coded(pkg, bytes=None)[0], "byte pool is missing")
    refused_as(coded(pkg, chunks=[(o0, l0 - 3, r0), (o1, l1, r1)])[0], "does not hold the bytes")    # an LZW stream that ends early
    refused_as(coded(pkg, chunks=[(o0, l0, r0), (o1, l1, 3)])[0], "does not hold the bytes")         # EOI before the rows' bytes
    t, c = coded(pkg, compression=tw.PACKBITS)
    (o0, l0, r0), (o1, l1, r1) = c["chunks"]
    refused_as(coded(pkg, compression=tw.PACKBITS, chunks=[(o0, l0 - 1, r0), (o1, l1, r1)])[0], "does not hold the bytes")
    t, c = coded(pkg, compression=tw.NONE)
    (o0, l0, r0), (o1, l1, r1) = c["chunks"]
    refused_as(coded(pkg, compression=tw.NONE, chunks=[(o0, l0 - 1, r0), (o1, l1, r1)])[0], "does not hold the bytes")
    # an LZW stream of the old LSB-first variant, a first code above 255, a code beyond the table
    for stream in (b"\x00\x01" + bytes(40), tc.pack_codes([256, 300, 257]), tc.pack_codes([256, 65, 259, 257])):
        refused_as(tc.to_pkg(pkg, tc.grey_strip(stream, 2)), "does not hold the bytes")
    # a table that is never cleared: 3838 codes fill it, the next one is refused
    full = tc.pack_codes([256] + [65] * 3840 + [257])
    refused_as(tc.to_pkg(pkg, tc.grey_strip(full, 3840)), "does not hold the bytes")
    # more chunks than the device stage takes: tiff::expand is the route for such a frame
    n = (1 << 20) + 1
    records = np.ones(n, pkg.TIFF_CHUNK)
    records["byte_off"] = np.arange(n)
    big = dict(tc.grey_strip(bytes(n), 1, tw.NONE), h=n, chunks=records)
    refused_as(tc.to_pkg(pkg, big), "beyond the device bounds")


def test_the_library_exports_the_coded_route(built, pkg):
    L = pkg.lib()
    for name in ("ocr_tiff_expand", "ocr_tiff_decode_coded", "ocr_tiff_time_coded", "ocr_tiff_time_coded_batch"):
        assert hasattr(L, name) and name in pkg.EXPORTS
    assert pkg.FRAME_TIFF_CODED == 8
