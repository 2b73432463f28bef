"""JPEG 2000 requests, host half: host/j2k_decode.h (through host/j2k_check, built with -fsanitize=address,undefined) against
OpenJPEG 2.5 as Pillow bundles it - the library OpenCV decodes JPEG 2000 with.  What is compared is cv::imdecode(IMREAD_COLOR)'s
view of OpenJPEG's samples: BGR, alpha dropped, 16 bits reduced by >> 8.

OpenJPEG's ENCODER refuses some files (more resolutions than the smaller side supports, offsets without a tile size) and
aborts the process on an irreversible line of one sample at an odd coordinate; the plan leaves those out (encodable())."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import j2k_frames as jf  # noqa: E402

Image = pytest.importorskip("PIL.Image")
from PIL import features  # noqa: E402

pytestmark = pytest.mark.skipif(not features.check_codec("jpg_2000"), reason="Pillow without OpenJPEG")

SIZES = [1, 2, 3, 4, 5, 16, 17, 31, 32, 33, 63, 64, 65, 129]
MODES = ["L", "RGB", "RGBA", "I;16"]
OPTIONS = [("reversible", {}), ("irreversible", dict(irreversible=True))] + \
          [("progression " + p, dict(progression=p, quality_layers=[10, 2], quality_mode="rates")) for p in ("LRCP", "RLCP", "RPCL", "PCRL", "CPRL")] + \
          [("resolutions %d" % n, dict(num_resolutions=n)) for n in range(1, 7)] + \
          [("code blocks %dx%d" % cb, dict(codeblock_size=cb)) for cb in ((4, 4), (32, 32), (64, 64), (1024, 4))] + \
          [("precincts", dict(precinct_size=(32, 32), codeblock_size=(16, 16))), ("layers 1", dict(quality_layers=[4], quality_mode="rates")),
           ("layers 3", dict(quality_layers=[30, 8, 1], quality_mode="rates", irreversible=True)), ("mct off", dict(mct=0)), ("mct off 9/7", dict(mct=0, irreversible=True)), ("mct on", dict(mct=1)), ("mct on 9/7", dict(mct=1, irreversible=True)),
           ("mct on layers", dict(mct=1, irreversible=True, quality_layers=[20, 3], quality_mode="rates")),
           ("tiles 32x32", dict(tile_size=(32, 32))), ("tiles 17x13", dict(tile_size=(17, 13))), ("bare", dict(no_jp2=True)), ("plt", dict(plt=True)),
           ("tiles 32x32 9/7", dict(tile_size=(32, 32), irreversible=True))]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return jf.build_check(tmp_path_factory.mktemp("j2kcheck"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def encodable(w, h, kw, ox, oy):
    """what OpenJPEG's encoder takes without refusing or aborting"""
    tw, th = kw.get("tile_size", (1 << 20, 1 << 20))
    tox, toy = kw.get("tile_offset", (0, 0))
    n = kw.get("num_resolutions", 6)
    xs = sorted({ox, ox + w} | {x for x in range(tox, ox + w, tw) if x > ox})
    ys = sorted({oy, oy + h} | {y for y in range(toy, oy + h, th) if y > oy})
    for lo, hi in list(zip(xs, xs[1:])) + list(zip(ys, ys[1:])):
        if "num_resolutions" in kw and hi - lo < 1 << (n - 1):
            return False
        if kw.get("irreversible"):
            for lev in range(0, n - 1):  # the lines that are transformed
                a, b = -(-lo >> lev), -(-hi >> lev)
                if b - a == 1 and (a & 1):
                    return False
    return True


def samples(rs, mode, w, h):
    smooth = np.add.outer(np.arange(h) * 3, np.arange(w) * 5)[:, :, None] + np.array([0, 80, 160])
    a = (smooth + rs.randint(-20, 21, (h, w, 3))) % 256
    if mode == "L":
        return a[:, :, 0].astype(np.uint8)
    if mode == "I;16":
        return (a[:, :, 0] * 257 + rs.randint(0, 257, (h, w))).astype(np.uint16)
    if mode == "RGBA":
        return np.dstack([a, rs.randint(0, 256, (h, w, 1))]).astype(np.uint8)
    return a.astype(np.uint8)


def encode(arr, **kw):
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG2000", **kw)
    return buf.getvalue()


def openjpeg_bgr(data):
    im = Image.open(io.BytesIO(data))
    im.load()
    a = np.asarray(im)
    if a.dtype != np.uint8:
        a = (a.astype(np.uint16) >> 8).astype(np.uint8)
    if a.ndim == 2:
        a = np.repeat(a[:, :, None], 3, 2)
    return a[:, :, :3][:, :, ::-1]


def plan():
    """every option value with every parity class of the image origin (which is the first tile-component's), sizes and modes
    going round; then the sizes crossed, and a few non-square ones"""
    rs = np.random.RandomState(11)
    out, k = [], 0
    for name, kw in OPTIONS:
        for ox, oy in ((0, 0), (1, 0), (0, 1), (1, 1)):
            for attempt in range(len(SIZES) * 2):
                w, h = SIZES[(k + attempt) % len(SIZES)], SIZES[(3 * k + 5 + 3 * attempt) % len(SIZES)]
                if name.startswith("code blocks 1024"):
                    w, h = 257, 3 + attempt
                opts = dict(kw)
                if ox or oy or "tile_size" in kw:
                    opts.update(offset=(ox + 2 * (k % 2), oy), tile_offset=(ox, 0) if "tile_size" in kw else (0, 0))
                    opts.setdefault("tile_size", (256, 256))
                    if opts.get("irreversible"):  # an odd origin stays odd down the levels: stop before a line of one sample
                        opts.setdefault("num_resolutions", 3)
                x0, y0 = opts.get("offset", (0, 0))
                if max(w, h) >= 4 and encodable(w, h, opts, x0, y0):
                    break
            else:
                raise AssertionError(name)
            out.append((name, (x0 & 1, y0 & 1), MODES[k % 4], w, h, opts))
            k += 1
    for i, w in enumerate(SIZES):
        for j, h in enumerate(SIZES):
            if (i + 2 * j) % 3 == 0:
                irr = bool((i + j) % 2)
                opts = dict(irreversible=True) if irr else {}
                if encodable(w, h, opts, 0, 0):
                    out.append(("size", (0, 0), MODES[(i + j) % 4], w, h, opts))
    for w, h in ((257, 3), (3, 257), (300, 2)):
        out.append(("size", (0, 0), "RGB", w, h, {}))
    return rs, out


@pytest.fixture(scope="module")
def decoded(exe, tmp_path_factory):
    """the whole plan encoded by OpenJPEG, decoded by j2k_check (one process) and by OpenJPEG, with the descriptor dumps"""
    d = tmp_path_factory.mktemp("j2kplan")
    rs, cases = plan()
    args, dumps, want = [], [], []
    for i, (name, parity, mode, w, h, opts) in enumerate(cases):
        data = encode(samples(rs, mode, w, h), **opts)
        src = d / ("c%04d.jp2" % i)
        src.write_bytes(data)
        args += [str(src), str(d / ("c%04d.bin" % i))]
        dumps += [str(src), str(d / ("c%04d.frame" % i))]
        want.append(openjpeg_bgr(data))
    r = subprocess.run([exe, "--decode"] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    subprocess.check_call([exe, "--frame"] + dumps)
    got = [np.fromfile(args[2 * i + 1], np.uint8).reshape(want[i].shape) for i in range(len(cases))]
    frames = [jf.read_frames(dumps[2 * i + 1])[0] for i in range(len(cases))]
    return cases, got, want, frames


def test_the_plan_covers_every_option_in_every_parity_class(decoded):
    """from the descriptor dumps: each option value met each parity class of a tile-component origin; all five progressions,
    1 .. 3 layers, 0 .. 5 levels, both transforms, JP2 and bare, tiled files, explicit precincts, every code-block size"""
    cases, _, _, frames = decoded
    seen = {}
    for (name, parity, *_), fr in zip(cases, frames):
        assert (fr["x0"] & 1, fr["y0"] & 1) == parity
        seen.setdefault(name, set()).update((int(t["x0"]) & 1, int(t["y0"]) & 1) for t in fr["tcs"])
    for name, _ in OPTIONS:
        assert len(seen[name]) == 4, (name, seen[name])
    assert {fr["progression"] for fr in frames} == {0, 1, 2, 3, 4}
    assert {fr["layers"] for fr in frames} >= {1, 2, 3}
    assert {int(fr["tcs"][0]["levels"]) for fr in frames} >= {0, 1, 2, 3, 4, 5}
    assert {fr["transform"] for fr in frames} == {0, 1} and {fr["jp2"] for fr in frames} == {0, 1} and {fr["mct"] for fr in frames} == {0, 1}
    assert {(fr["cbw"], fr["cbh"]) for fr in frames} >= {(4, 4), (32, 32), (64, 64), (1024, 4), (16, 16)}
    assert any(fr["precincts"] for fr in frames) and any(fr["tiles_x"] * fr["tiles_y"] > 4 for fr in frames)
    assert {fr["prec"] for fr in frames} == {8, 16} and {fr["file_comps"] for fr in frames} == {1, 3, 4}


def test_reversible_files_equal_openjpeg_byte_for_byte(decoded):
    cases, got, want, frames = decoded
    n = 0
    for case, g, w, fr in zip(cases, got, want, frames):
        if fr["transform"] == 0:
            assert np.array_equal(g, w), case
            n += 1
    assert n >= 80


def test_irreversible_files_equal_openjpeg_byte_for_byte(decoded):
    """the 9/7 path in OpenJPEG's operation order leaves no residue on this grid: measured share of differing samples 0, so
    the cap (twice the measured share) is 0 as well - byte for byte"""
    cases, got, want, frames = decoded
    n = differ = total = 0
    for case, g, w, fr in zip(cases, got, want, frames):
        if fr["transform"] == 1:
            d = np.abs(g.astype(int) - w.astype(int))
            assert d.max() <= 1, case
            differ += int((d > 0).sum())
            total += d.size
            n += 1
    print("irreversible files %d, samples %d, differing %d" % (n, total, differ))
    assert n >= 30 and differ == 0


# ------------------------------------------------------------------------------------------------------------------ refusals
def _marker(data, m):
    return data.index(bytes([0xff, m]))


def _insert_main(data, segment):
    at = _marker(data, 0x90)  # in front of the first SOT
    return data[:at] + segment + data[at:]


def refusals():
    rs = np.random.RandomState(4)
    rgb = samples(rs, "RGB", 17, 16)
    bare = bytearray(encode(rgb, no_jp2=True))
    jp2 = bytearray(encode(rgb))
    cod, siz = _marker(bare, 0x52), _marker(bare, 0x51)
    out = []

    def patched(src, at, value, text, op="set"):
        b = bytearray(src)
        b[at] = value if op == "set" else b[at] | value
        out.append((text, bytes(b)))
    for bit, _ in enumerate(("bypass", "reset", "terminate all", "vertically causal", "predictable termination", "segmentation symbols")):
        patched(bare, cod + 12, 1 << bit, "code-block styles", "or")
    patched(bare, cod + 12, 0x40, "HT code blocks", "or")
    patched(bare, siz + 4, 0x40, "HT code blocks", "or")  # Rsiz bit 14
    out.append(("HT code blocks", _insert_main(bytes(bare), b"\xff\x50\x00\x08\x00\x02\x00\x00\x00\x00")))  # CAP
    out.append(("RGN", _insert_main(bytes(bare), b"\xff\x5e\x00\x05\x00\x00\x01")))
    out.append(("POC", _insert_main(bytes(bare), b"\xff\x5f\x00\x09\x00\x00\x00\x01\x01\x03\x00")))
    out.append(("PPM", _insert_main(bytes(bare), b"\xff\x60\x00\x03\x00")))
    sot = _marker(bare, 0x90)
    sod = bare.index(b"\xff\x93", sot)
    psot = int.from_bytes(bare[sot + 6:sot + 10], "big") + 5
    out.append(("PPT", bytes(bare[:sot + 6]) + psot.to_bytes(4, "big") + bytes(bare[sot + 10:sod]) + b"\xff\x61\x00\x03\x00" + bytes(bare[sod:])))
    h = jp2.index(b"jp2h")
    hl = int.from_bytes(jp2[h - 4:h], "big")
    pclr = (8 + 3).to_bytes(4, "big") + b"pclr" + b"\x00\x01\x01"
    out.append(("palette", bytes(jp2[:h - 4]) + (hl + len(pclr)).to_bytes(4, "big") + bytes(jp2[h:h + 4]) + pclr + bytes(jp2[h + 4:])))
    c = jp2.index(b"colr")
    assert jp2[c + 4] == 1
    patched(jp2, c + 10, 18, "colour spaces")  # sYCC
    patched(bare, siz + 40, 0x87, "signed")
    patched(bare, siz + 40 + 3, 6, "differing precision")
    patched(bare, siz + 41, 2, "subsampled")
    five = bytearray(bare)
    five[siz + 2:siz + 4] = (38 + 15).to_bytes(2, "big")
    five[siz + 38:siz + 40] = (5).to_bytes(2, "big")
    five[siz + 49:siz + 49] = bytes(bare[siz + 40:siz + 43]) * 2
    out.append(("more than 4 components", bytes(five)))
    deep = bytearray(bare)
    for k in range(3):
        deep[siz + 40 + 3 * k] = 16
    out.append(("precision above 16", bytes(deep)))
    big = bytearray(bare)
    big[siz + 6:siz + 14] = (70000).to_bytes(4, "big") * 2
    out.append(("64 Mi", bytes(big)))
    return out


def test_what_is_out_of_scope_is_refused_with_its_reason(exe, tmp_path):
    cases = refusals()
    paths = []
    for i, (_, data) in enumerate(cases):
        p = tmp_path / ("r%02d.bin" % i)
        p.write_bytes(data)
        paths.append(str(p))
    r = subprocess.run([exe, "--why"] + paths, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(cases)
    for (text, _), line in zip(cases, lines):
        assert line.startswith("refused: ") and text in line, (text, line)


def test_truncated_and_damaged_files_neither_crash_nor_read_out_of_bounds(exe, tmp_path):
    """every prefix of three small files and single flipped bytes through the sanitizer build: exit status 0, each file either
    refused or decoded to the header's size.  No parity with OpenJPEG is claimed."""
    rs = np.random.RandomState(9)
    files = [encode(samples(rs, "RGB", 17, 9), no_jp2=True, num_resolutions=3), encode(samples(rs, "L", 16, 16), irreversible=True, quality_layers=[4, 1], quality_mode="rates"),
             encode(samples(rs, "RGBA", 9, 12), tile_size=(8, 8), num_resolutions=2, progression="RPCL")]
    sizes = [(17, 9), (16, 16), (9, 12)]
    args, owner = [], []
    for k, data in enumerate(files):
        variants = [data[:n] for n in range(len(data))]
        for at in rs.randint(0, len(data), 150):
            b = bytearray(data)
            b[at] ^= 1 << rs.randint(8)
            variants.append(bytes(b))
        for i, v in enumerate(variants):
            p = tmp_path / ("d%d_%04d.bin" % (k, i))
            p.write_bytes(v)
            args += [str(p), str(tmp_path / "out.bin")]
            owner.append((k, i < len(data)))
    lines, decoded_n = [], 0
    for start in range(0, len(owner), 400):
        r = subprocess.run([exe, "--try"] + args[2 * start:2 * (start + 400)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        lines += r.stdout.strip().splitlines()
    assert len(lines) == len(owner)
    for (k, prefix), line in zip(owner, lines):
        if line != "refused":
            size = tuple(int(v) for v in line.split())
            assert size == sizes[k] if prefix else len(size) == 2, line  # (a flipped header byte may state another size)
            decoded_n += 1
    print("variants %d, decoded %d, refused %d" % (len(owner), decoded_n, len(owner) - decoded_n))
    assert decoded_n > 0 and decoded_n < len(owner)
