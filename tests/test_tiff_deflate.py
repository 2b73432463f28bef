"""Deflate TIFF requests, host half (host/tiff_decode.h): tiff::parse_deflate + tiff::inflate_all give the bytes tiff::parse gives;
every structural rule of the Deflate entry points is refused with its message before the runtime is touched; and the walk of
the device's inflate kernel (csrc/inflate_core.h), compiled as plain C++ for one lane in host/inflate_check.cpp with
-fsanitize=address,undefined, gives zlib's verdict and zlib's bytes (tiff_check --inflate) on the hand-built streams, the
refill streams and the mutated corpus.  Nothing sanitized is loaded into Python.  The device half is
tests/test_gpu_tiff_deflate.py."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_streams as ds  # noqa: E402
import tiff_coded as tc  # noqa: E402
import tiff_writer as tw  # noqa: E402
from test_tiff_decode import HOST, build_check  # noqa: E402

SAN = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """host/tiff_check.cpp with AddressSanitizer and UBSan: a stand-alone host program"""
    return build_check(tmp_path_factory.mktemp("tiffdeflate"), *SAN)


@pytest.fixture(scope="module")
def inflate_check(tmp_path_factory):
    """host/inflate_check.cpp with AddressSanitizer and UBSan: the kernel's walk for one lane, a stand-alone host program"""
    exe = os.path.join(str(tmp_path_factory.mktemp("inflatecheck")), "inflate_check_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", *SAN, "-o", exe, os.path.join(HOST, "inflate_check.cpp")])
    return exe


def run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return r


def test_parse_deflate_and_inflate_all_give_the_bytes_of_parse(checker, tmp_path):
    """every form x {8, 32946} x {strips, tiles}, with planar 2, the predictor at 8 and 16 bits, both byte orders and FillOrder 2
    among them: Frame::data of parse_deflate + inflate_all == Frame::data of parse == the chunks the writer stored; an LZW file
    is not parse_deflate's, and a Deflate file with a short stream passes parse_deflate (no stream is looked at) and is refused
    by inflate_all as by parse"""
    rs = np.random.RandomState(41)
    files, want, k = [], [], 0
    for form in tw.FORMS:
        name, photometric, bits, spp, extra = form
        for comp in (tw.ADOBE_DEFLATE, tw.DEFLATE):
            for layout in ("strips", "tiles"):
                k += 1
                h, w = (5, 17, 33)[k % 3], (3, 31, 65)[(k // 3) % 3]
                samples, colormap = tw.random_case(rs, form, h, w)
                kw = dict(big_endian=bool(k & 1), compression=comp)
                if bits >= 8 and k % 3:
                    kw["predictor"] = 2
                if layout == "strips":
                    kw["rows_per_strip"] = (None, 1, 2, 4)[k % 4]
                else:
                    kw["tile"] = ((16, 16), (32, 16))[k % 2]
                if k % 5 == 0:
                    kw["fill_order"] = 2
                if bits >= 8 and (photometric == tw.RGB or (photometric <= 1 and spp >= 2)) and k % 2:
                    kw["planar"] = 2
                files.append(tw.write_tiff(samples, bits, photometric, extra=extra, colormap=colormap, **kw))
                geo = {a: b for a, b in kw.items() if a in ("planar", "predictor", "tile", "rows_per_strip", "big_endian")}
                want.append(tw.frame_data(samples, bits, **geo)[0])
    assert len(files) == len(tw.FORMS) * 4
    args_chunks, args_coded = [], []
    for i, data in enumerate(files):
        p = str(tmp_path / ("f%03d.tif" % i))
        open(p, "wb").write(data)
        args_chunks += [p, p + ".chunks"]
        args_coded += [p, p + ".coded"]
    assert run(checker, "--chunks", *args_chunks).returncode == 0
    assert run(checker, "--route-deflate", *args_coded).returncode == 0
    with open(tmp_path / "all.coded", "wb") as f:
        for i in range(len(files)):
            f.write(open(args_coded[2 * i + 1], "rb").read())
    r = run(checker, "--inflate-all", str(tmp_path / "all.coded"), str(tmp_path / "all.chunks"))
    assert r.returncode == 0 and r.stdout.split() == ["ok"] * len(files)
    got = open(tmp_path / "all.chunks", "rb").read()
    pos = 0
    for i, w in enumerate(want):
        assert open(args_chunks[2 * i + 1], "rb").read() == w, ("parse differs from the stored chunks", i)
        assert got[pos:pos + len(w)] == w, ("parse_deflate + inflate_all differs from parse", i)
        pos += len(w)
    assert pos == len(got)
    samples = rs.randint(0, 256, (4, 4, 3))
    short = zlib.compress(bytes(47))
    names = {"lzw.tif": tw.write_tiff(samples, 8, tw.RGB, compression=tw.LZW), "short.tif": tw.write_tiff(samples, 8, tw.RGB, compression=tw.ADOBE_DEFLATE, streams=[short])}
    for n, data in names.items():
        open(tmp_path / n, "wb").write(data)
    assert run(checker, "--route-deflate", str(tmp_path / "lzw.tif"), str(tmp_path / "l.coded")).returncode == 1
    assert run(checker, "--route-deflate", str(tmp_path / "short.tif"), str(tmp_path / "s.coded")).returncode == 0
    r = run(checker, "--inflate-all", str(tmp_path / "s.coded"), str(tmp_path / "s.chunks"))
    assert r.returncode == 1 and r.stdout.split() == ["refused"]
    assert run(checker, "--chunks", str(tmp_path / "short.tif"), str(tmp_path / "s2.chunks")).returncode == 1
    # the old surface: a Deflate file is still the other route of parse_coded
    r = run(checker, "--why", str(tmp_path / "short.tif"))
    assert r.stdout.strip().endswith("other route")


def deflated(pkg, **kw):
    """a sound 4 x 5 RGB frame in two Deflate strips, fields changed by name"""
    samples = np.random.RandomState(3).randint(0, 256, (5, 4, 3))
    c, _ = tc.make_coded(samples, tw.FORMS[16], kw.pop("compression", tw.ADOBE_DEFLATE), rows_per_strip=3)
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


def test_deflate_rules_are_refused_before_any_device_call(built, pkg):
    """every structural rule drives ocr_tiff_inflate and ocr_tiff_decode_deflate to OCR_ERR_ARG with a message that names it - on
    a machine with or without a GPU: the check comes before the runtime is touched, so nothing was launched and the output
    buffer is as it was.  Compression 5 handed to a Deflate entry point is one of them; no rule looks at a stream"""
    def refused_as(t, what):
        for call in (t.inflate, t.decode_deflate):
            with pytest.raises(pkg.OcrError, match=what) as e:
                call(fill=0xA5)
            assert e.value.code == -1  # OCR_ERR_ARG
            assert (e.value.out == 0xA5).all()

    _, sound = deflated(pkg)
    (o0, l0, r0), (o1, l1, r1) = sound["chunks"]
    assert (r0, r1) == (3, 2)
    refused_as(deflated(pkg, bits_per_sample=3)[0], "bits per sample")
    refused_as(deflated(pkg, width=0)[0], "positive")
    refused_as(deflated(pkg, frame_data=True)[0], "carries no expanded chunks")
    for comp in (5, 1, 32773, 7):
        refused_as(deflated(pkg, compression=comp)[0], "compression must be 8 or 32946")
    refused_as(deflated(pkg, chunks_len=1)[0], "as many chunk records")
    refused_as(deflated(pkg, chunks=sound["chunks"] + [(0, 1, 1)])[0], "as many chunk records")
    refused_as(deflated(pkg, chunks=[(o0, l0, 0), (o1, l1, r1)])[0], "rows must be 1 .. tile_height")
    refused_as(deflated(pkg, chunks=[(o0, l0, 4), (o1, l1, r1)])[0], "rows must be 1 .. tile_height")
    refused_as(deflated(pkg, chunks=[(o0, l0, r0), (o1, l1 + 1, r1)])[0], "outside the pool")
    refused_as(deflated(pkg, chunks=[(o0, l0, r0), (len(sound["data"]) + 1, 0, r1)])[0], "outside the pool")
    refused_as(deflated(pkg, chunks=[((1 << 64) - 1, 2, r0), (o1, l1, r1)])[0], "outside the pool")
    refused_as(deflated(pkg, bytes_len=len(sound["data"]) - 1)[0], "outside the pool")
    refused_as(deflated(pkg, bytes=None)[0], "byte pool is missing")
    n = (1 << 20) + 1
    records = np.ones(n, pkg.TIFF_CHUNK)
    records["byte_off"] = np.arange(n)
    big = dict(tc.grey_strip(bytes(n), 1, tw.ADOBE_DEFLATE), h=n, chunks=records)
    refused_as(tc.to_pkg(pkg, big), "beyond the device bounds")
    # the old entry points keep their rule and their words for the same frame
    t = deflated(pkg)[0]
    for call in (t.expand, t.decode):
        with pytest.raises(pkg.OcrError, match=r"compression must be 1 \(none\), 5 \(LZW\) or 32773 \(PackBits\)"):
            call()


def test_the_library_exports_the_deflate_route(built, pkg):
    L = pkg.lib()
    for name in ("ocr_tiff_inflate", "ocr_tiff_decode_deflate", "ocr_tiff_time_deflate", "ocr_tiff_time_deflate_batch",
                 "ocr_tiff_expand", "ocr_tiff_decode_coded", "ocr_tiff_time_coded", "ocr_tiff_time_coded_batch"):
        assert hasattr(L, name) and name in pkg.EXPORTS
    assert pkg.FRAME_TIFF_CODED == 8 and pkg.FRAME_TIFF_DEFLATE == 9


def test_the_kernels_walk_under_the_sanitizers_gives_the_hosts_verdicts(checker, inflate_check, tmp_path):
    """inflate_check (csrc/inflate_core.h for one lane, ASan + UBSan) against tiff_check --inflate (zlib, the host's rule) over the
    hand-built list, the refill streams and the mutated corpus: the same verdict, the same count and the same bytes per stream.
    Sound streams are held to Python's zlib as well.  The corpus refuses and accepts at least a tenth each, on the host's
    verdicts alone."""
    for tag, cases in (("hand", ds.hand_built()), ("refill", ds.refill_streams()), ("fuzz", ds.fuzz_corpus())):
        host = ds.verdicts(checker, cases, tmp_path, tag + "_host")
        mine = ds.verdicts(inflate_check, cases, tmp_path, tag + "_walk")
        for (name, need, stream), h, m in zip(cases, host, mine):
            assert h[0] == m[0] and h[1] == m[1], (name, "host", h[:2], "walk", m[:2])
            assert h[2] == m[2], (name, "bytes differ")
            if h[0]:
                try:
                    whole = zlib.decompressobj().decompress(stream)
                except zlib.error:
                    continue  # (zlib reads on behind `need`: a fault or a wrong checksum there is not the host's business)
                assert whole[:need] == h[2], name
        good = sum(h[0] for h in host)
        print(tag, len(cases), "streams,", good, "accepted")
        if tag == "fuzz":
            assert len(cases) == 240 and good * 10 >= len(cases) and (len(cases) - good) * 10 >= len(cases), good
        else:
            assert 0 < good <= len(cases)
