"""BMP and PNM requests, host half (host/raw_decode.h): container parsers, run-length and ASCII expansion, and the host
pixel stage, which must return what cv::imdecode(IMREAD_COLOR) returns.  The expectation is built from the arrays a file
was written from (tests/raw_writer.py), never from the decoder; Pillow is compared where it reads a file and agrees by
design.  The device half is tests/test_gpu_raw.py."""
import io
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raw_writer as rw  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cpp-paddle-ocr_amd", "host")
TOOL = os.path.join(HOST, "decode_tool")
# they cross the byte and dword edges of the 1- and 4-bit rows and the 4-byte row padding
WIDTHS = [1, 7, 8, 9, 31, 32, 33]
DEPTHS = [1, 4, 8, 16, 24, 32]


def read_ppm(path):
    """decode_tool's output (binary P6, maxval 255) -> (h, w, 3) BGR"""
    d = open(path, "rb").read()
    tok = d.split(None, 4)
    assert tok[0] == b"P6" and tok[3] == b"255"
    w, h = int(tok[1]), int(tok[2])
    body = d[len(d) - 3 * w * h:]
    return np.frombuffer(body, np.uint8).reshape(h, w, 3)[:, :, ::-1]


def decode_files(cases, tmp_path, *flags, env=None):
    """all files through one decode_tool process; the decoded BGR arrays.  cases: [(name, file bytes, expected BGR)]"""
    args = []
    for i, (_, data, _) in enumerate(cases):
        src = tmp_path / ("r%04d.bin" % i)
        src.write_bytes(data)
        args += [str(src), str(tmp_path / ("r%04d.ppm" % i))]
    r = subprocess.run([TOOL, *flags] + args, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return [read_ppm(tmp_path / ("r%04d.ppm" % i)) for i in range(len(cases))]


def check_cases(cases, tmp_path, *flags, env=None):
    for (name, _, want), got in zip(cases, decode_files(cases, tmp_path, *flags, env=env)):
        assert got.shape == want.shape, (name, got.shape, want.shape)
        assert np.array_equal(got, want), (name, int(np.abs(got.astype(int) - want.astype(int)).max()))


def refused(tool, tmp_path, data, name="hostile"):
    src = tmp_path / (name + ".bin")
    src.write_bytes(data)
    r = subprocess.run([tool, str(src), str(tmp_path / (name + ".ppm"))], capture_output=True, text=True)
    assert r.returncode == 1 and "decode failed" in r.stderr, (name, r.returncode, r.stderr[-500:])


@pytest.fixture(scope="module")
def tool(built):
    subprocess.check_call(["make", "-s", "-C", HOST])
    return TOOL


def bmp_matrix(seed=1):
    """every depth x {bottom-up, top-down} x header {12, 40, 124} over the widths in turn.  The 12-byte OS/2 header stores
    an unsigned 16-bit height: it has no top-down form, those combinations do not exist."""
    rs = np.random.RandomState(seed)
    cases, k = [], 0
    for bpp in DEPTHS:
        for top_down in (False, True):
            for header in (12, 40, 124):
                if header == 12 and top_down:
                    continue
                for _ in range(3):
                    w = WIDTHS[k % len(WIDTHS)]
                    h = (1, 2, 5, 4)[k % 4]
                    k += 1
                    s = rw.random_bmp_samples(rs, h, w, bpp)
                    pal = rs.randint(0, 256, (1 << bpp, 3)) if bpp <= 8 else None
                    data = rw.write_bmp(s, bpp, header=header, top_down=top_down, palette=pal)
                    cases.append(("bmp %d bpp header %d %s %dx%d" % (bpp, header, "top-down" if top_down else "bottom-up", w, h), data,
                                  rw.expected_bmp(s, bpp, pal)))
    return cases


def pnm_matrix(seed=2):
    """P1 .. P6 x maxval {1, 15, 255, 256, 65535} (none for P1 / P4), comments in the header, over the widths in turn"""
    rs = np.random.RandomState(seed)
    cases, k = [], 0
    for ptype in range(1, 7):
        for maxval in ((1,) if ptype in (1, 4) else (1, 15, 255, 256, 65535)):
            for _ in range(2 if ptype in (1, 4) else 1):
                for w in (WIDTHS[k % len(WIDTHS)], WIDTHS[(k + 3) % len(WIDTHS)]):
                    h = (1, 3, 4)[k % 3]
                    k += 1
                    s = rs.randint(0, maxval + 1, (h, w, 3 if ptype in (3, 6) else 1))
                    cases.append(("P%d maxval %d %dx%d" % (ptype, maxval, w, h), rw.write_pnm(ptype, s, maxval), rw.expected_pnm(ptype, s, maxval)))
    return cases


def test_bmp_every_depth_row_order_and_header(tool, tmp_path):
    cases = bmp_matrix()
    assert len(cases) == 6 * 5 * 3
    check_cases(cases, tmp_path)


def test_pnm_every_type_and_maxval(tool, tmp_path):
    check_cases(pnm_matrix(), tmp_path)


def test_every_width_at_the_sub_byte_depths(tool, tmp_path):
    """1- and 4-bit BMP, P1 and P4 at every width of the list, more than one row"""
    rs = np.random.RandomState(3)
    cases = []
    for w in WIDTHS:
        for bpp in (1, 4):
            s = rw.random_bmp_samples(rs, 3, w, bpp)
            pal = rs.randint(0, 256, (1 << bpp, 3))
            cases.append(("bmp %d bpp %d wide" % (bpp, w), rw.write_bmp(s, bpp, palette=pal), rw.expected_bmp(s, bpp, pal)))
        for ptype in (1, 4):
            s = rs.randint(0, 2, (3, w, 1))
            cases.append(("P%d %d wide" % (ptype, w), rw.write_pnm(ptype, s), rw.expected_pnm(ptype, s)))
    check_cases(cases, tmp_path)


def rle_cases(seed=4):
    rs = np.random.RandomState(seed)
    cases = []
    for bpp in (8, 4):
        for w, h in ((1, 1), (7, 3), (33, 9), (300, 12), (64, 40)):
            idx = rs.randint(0, 1 << bpp, (h, w))
            if w >= 33:
                idx[:, w // 3:w // 2] = idx[:, w // 3:w // 3 + 1]  # flat stretches: long encoded runs
            pal = rs.randint(1, 256, (1 << bpp, 3))  # no entry is black: an unwritten pixel shows as palette[0], not by chance
            stream, want_idx = rw.rle_encode(idx, bpp, rs)
            cases.append(("rle%d %dx%d" % (bpp, w, h), rw.write_bmp(idx, bpp, palette=pal, compression=1 if bpp == 8 else 2, stream=stream),
                          rw.lookup(want_idx, pal)))
            for cut in (len(stream) // 2, len(stream) // 2 + 1, 3):
                s2, want2 = rw.rle_encode(idx, bpp, np.random.RandomState(seed + w), truncate_at=cut)
                cases.append(("rle%d %dx%d cut at %d" % (bpp, w, h, cut), rw.write_bmp(idx, bpp, palette=pal, compression=1 if bpp == 8 else 2, stream=s2),
                              rw.lookup(want2, pal)))
    return cases


def test_rle_with_moves_truncation_and_unwritten_pixels(tool, tmp_path):
    cases = rle_cases()
    # the encoder did skip pixels and did use every operation somewhere
    whole = [c for c in cases if "cut" not in c[0] and "300x12" in c[0]]
    for name, data, want in whole:
        off = struct.unpack("<I", data[10:14])[0]
        stream = data[off:]
        assert b"\x00\x02" in stream and b"\x00\x00" in stream and stream.endswith(b"\x00\x01"), name
    check_cases(cases, tmp_path)


def test_rle_runs_are_clipped_and_leaving_the_canvas_ends_the_decode(tool, tmp_path):
    pal = np.arange(1, 256 * 3 + 1).reshape(256, 3) % 251 + 1
    w, h = 5, 3
    # row 0 (bottom): a run of 9 of index 7 - clipped at 5; end of line; row 1: move by (6, 0) leaves the canvas: decode ends
    stream = bytes([9, 7, 0, 0, 2, 3, 0, 2, 6, 0, 5, 9, 0, 0, 5, 9, 0, 1])
    want = np.zeros((h, w), np.int64)
    want[2, :] = 7
    want[1, :2] = 3
    # rows past the top: end of line three times, then a run that has no row
    stream2 = bytes([5, 1, 0, 0, 5, 2, 0, 0, 5, 3, 0, 0, 5, 4, 0, 1])
    want2 = np.array([[3] * 5, [2] * 5, [1] * 5])
    # an absolute run of 4 pixels of RLE4 with its padding, then an encoded run of alternating nibbles over the row end
    stream3 = bytes([0, 4, 0x12, 0x34, 3, 0xAB, 0, 1])
    want3 = np.zeros((h, w), np.int64)
    want3[2] = [1, 2, 3, 4, 0xA]
    cases = [("clip and leave", rw.write_bmp(want, 8, palette=pal, compression=1, stream=stream), rw.lookup(want, pal)),
             ("past the top", rw.write_bmp(want2, 8, palette=pal, compression=1, stream=stream2), rw.lookup(want2, pal)),
             ("rle4 absolute", rw.write_bmp(want3, 4, palette=pal[:16], compression=2, stream=stream3), rw.lookup(want3, pal[:16]))]
    check_cases(cases, tmp_path)


def test_sixteen_bit_forms_and_masks(tool, tmp_path):
    """5-5-5 without masks, 5-5-5 and 5-6-5 through BITFIELDS (40-byte header: masks behind it; 124-byte: inside it); the
    expansion shifts and leaves the low bits zero - 0x7FFF is (248, 248, 248), not white; another mask triple is refused"""
    rs = np.random.RandomState(5)
    cases = []
    for w in (1, 7, 32, 33):
        s = rs.randint(0, 1 << 16, (3, w))
        s[0, 0] = 0x7FFF
        cases.append(("555 %d" % w, rw.write_bmp(s, 16), rw.expand16(s, False)))
        for header in (40, 124):
            cases.append(("555 masks %d header %d" % (w, header), rw.write_bmp(s, 16, header=header, compression=3, masks=(0x7C00, 0x03E0, 0x001F)), rw.expand16(s, False)))
            cases.append(("565 masks %d header %d" % (w, header), rw.write_bmp(s, 16, header=header, compression=3, masks=(0xF800, 0x07E0, 0x001F)), rw.expand16(s, True)))
    assert tuple(cases[0][2][0, 0]) == (248, 248, 248)
    check_cases(cases, tmp_path)
    refused(tool, tmp_path, rw.write_bmp(rs.randint(0, 1 << 16, (3, 4)), 16, compression=3, masks=(0x0F00, 0x00F0, 0x000F)), "masks444")


def test_thirty_two_bit_drops_alpha_and_skips_masks(tool, tmp_path):
    rs = np.random.RandomState(6)
    s = rs.randint(0, 256, (4, 9, 4))
    s[:, :, 3] = np.array([0, 128, 255])[np.arange(9) % 3][None, :]
    cases = [("bgra", rw.write_bmp(s, 32), s[:, :, :3].astype(np.uint8)),
             ("bgra masks", rw.write_bmp(s, 32, compression=3, masks=(0x000000FF, 0x0000FF00, 0x00FF0000)), s[:, :, :3].astype(np.uint8)),
             ("bgra top-down v5", rw.write_bmp(s, 32, header=124, top_down=True, compression=3, masks=(0xFF0000, 0xFF00, 0xFF)), s[:, :, :3].astype(np.uint8))]
    check_cases(cases, tmp_path)


def test_palette_shorter_than_the_indices_used(tool, tmp_path):
    """biClrUsed = 5 entries, indices up to 255 (and a grey palette still gives three channels): the entries the file does
    not have are black; and a biClrUsed beyond 1 << bpp is clamped"""
    rs = np.random.RandomState(7)
    idx = rs.randint(0, 256, (4, 9))
    pal = rs.randint(1, 256, (5, 3))
    grey = np.repeat(np.arange(0, 256, 16)[:, None], 3, 1)
    idx4 = rs.randint(0, 16, (3, 7))
    cases = [("short palette", rw.write_bmp(idx, 8, palette=pal), rw.lookup(idx, pal)),
             ("grey palette", rw.write_bmp(idx4, 4, palette=grey), rw.lookup(idx4, grey)),
             ("clamped count", rw.write_bmp(idx4, 4, palette=grey, clr_used=200), rw.lookup(idx4, grey))]
    assert (cases[0][2] == 0).all(axis=2).any()
    check_cases(cases, tmp_path)


def test_ascii_values_above_maxval_and_missing_numbers(tool, tmp_path):
    rs = np.random.RandomState(8)
    cases = []
    for ptype, c in ((2, 1), (3, 3)):
        for maxval in (15, 255, 300, 65535):
            s = rs.randint(0, 2 * maxval + 2, (3, 7, c))
            cases.append(("P%d maxval %d beyond" % (ptype, maxval), rw.write_pnm(ptype, s, maxval), rw.expected_pnm(ptype, s, maxval)))
    check_cases(cases, tmp_path)
    s = rs.randint(0, 256, (3, 7, 1))
    whole = rw.write_pnm(2, s, 255, comments=False)
    refused(tool, tmp_path, whole[:whole.rstrip().rfind(b" ")], "p2short")       # the last number is missing
    refused(tool, tmp_path, rw.write_pnm(1, s & 1)[:-6], "p1short")
    refused(tool, tmp_path, b"P7\nWIDTH 1\nHEIGHT 1\nDEPTH 1\nMAXVAL 255\nTUPLTYPE GRAYSCALE\nENDHDR\n\x00", "pam")
    refused(tool, tmp_path, b"P5\n2 2\n65536\n" + b"\0" * 8, "maxval65536")
    refused(tool, tmp_path, b"P5\n2 2\n0\n" + b"\0" * 4, "maxval0")
    refused(tool, tmp_path, rw.write_pnm(6, rs.randint(0, 256, (3, 7, 3)))[:-1], "p6short")


def test_what_the_service_took_before_decodes_to_the_same_bytes(tool, tmp_path):
    """24- and 32-bit BMP (both row orders, 32-bit with BITFIELDS, a gap in front of the rows) and P6 with maxval 255: the
    files the decoders before this one accepted give the bytes they gave - B,G,R as stored, rows in image order"""
    rs = np.random.RandomState(9)
    cases = []
    for w in WIDTHS:
        bgr = rs.randint(0, 256, (3, w, 3)).astype(np.uint8)
        bgra = np.concatenate([bgr, rs.randint(0, 256, (3, w, 1)).astype(np.uint8)], 2)
        cases += [("24 bottom-up %d" % w, rw.write_bmp(bgr, 24), bgr), ("24 top-down gap %d" % w, rw.write_bmp(bgr, 24, top_down=True, gap=5), bgr),
                  ("24 v4 header %d" % w, rw.write_bmp(bgr, 24, header=108), bgr),
                  ("32 %d" % w, rw.write_bmp(bgra, 32), bgr), ("32 bitfields top-down %d" % w, rw.write_bmp(bgra, 32, top_down=True, compression=3, masks=(0xFF0000, 0xFF00, 0xFF)), bgr),
                  ("P6 %d" % w, b"P6\n# c\n%d 3\n255\n" % w + bgr[:, :, ::-1].tobytes(), bgr)]
    check_cases(cases, tmp_path)


def test_pillow_reads_the_same_pixels(tool, tmp_path):
    """where Pillow reads the file and the rules agree by design: BMP at 1 / 4 / 8 / 24 / 32 bits with a full palette, PNM
    without a maxval or with maxval 255.  Left out on purpose: 16-bit BMP (Pillow replicates the high bits into the low
    ones, cv::imdecode shifts), PNM with another maxval (Pillow rescales by it, cv::imdecode does not), run-length streams
    with unwritten pixels and short palettes (undefined for Pillow)."""
    Image = pytest.importorskip("PIL.Image")
    cases = [c for c in bmp_matrix(seed=11) if " 16 bpp" not in c[0]] + [c for c in pnm_matrix(seed=12) if c[0][:2] in ("P1", "P4") or "maxval 255" in c[0]]
    got = decode_files(cases, tmp_path)
    compared = 0
    for (name, data, want), g in zip(cases, got):
        try:
            im = Image.open(io.BytesIO(data))
            im.load()
            ref = np.array(im.convert("RGB"))[:, :, ::-1]
        except Exception:  # this Pillow does not read the form
            continue
        compared += 1
        assert ref.shape == g.shape and np.array_equal(ref, g), name
    if compared == 0:
        pytest.skip("Pillow read none of the files")


def hostile_files():
    big = struct.pack("<IiiHHIIiiII", 40, 4, 4, 1, 24, 0, 0, 0, 0, 0, 0)

    def bmp(info, off=54, body=b"\0" * 64):
        return b"BM" + struct.pack("<IHHI", 14 + len(info) + len(body), 0, 0, off) + info + body

    return {
        "data offset past the end": bmp(big, off=100000),
        "stride overflow": bmp(struct.pack("<IiiHHIIiiII", 40, 0x7FFFFFFF, 1, 1, 32, 0, 0, 0, 0, 0, 0)),
        "stride overflow wide paletted": bmp(struct.pack("<IiiHHIIiiII", 40, 0x7FFFFFF9, 1, 1, 1, 0, 0, 0, 0, 0, 0)),
        "biClrUsed 0xFFFFFFFF": bmp(struct.pack("<IiiHHIIiiII", 40, 4, 4, 1, 8, 0, 0, 0, 0, 0xFFFFFFFF, 0), off=54, body=b"\1" * 8),
        "height INT32_MIN": bmp(struct.pack("<IiiHHIIiiII", 40, 4, -0x80000000, 1, 24, 0, 0, 0, 0, 0, 0)),
        "64 Mpixel and one more row": bmp(struct.pack("<IiiHHIIiiII", 40, 8192, 8193, 1, 8, 1, 0, 0, 0, 0, 0)),
        "P6 10^6 x 10^6": b"P6\n1000000 1000000\n255\n" + b"\0" * 64,
        "P3 8192 x 8192 with no numbers": b"P3\n8192 8192\n255\n1 2 3\n",
        "P5 16-bit 8000 x 8000 cut short": b"P5\n8000 8000\n65535\n" + b"\0" * 64,
        "header size 16": bmp(struct.pack("<I", 16) + big[4:]),
        "RLE8 top-down": bmp(struct.pack("<IiiHHIIiiII", 40, 4, -4, 1, 8, 1, 0, 0, 0, 0, 0)),
        "RLE8 at 4 bpp": bmp(struct.pack("<IiiHHIIiiII", 40, 4, 4, 1, 4, 1, 0, 0, 0, 0, 0)),
        "JPEG payload": bmp(struct.pack("<IiiHHIIiiII", 40, 4, 4, 1, 24, 4, 0, 0, 0, 0, 0)),
        "zero width": bmp(struct.pack("<IiiHHIIiiII", 40, 0, 4, 1, 24, 0, 0, 0, 0, 0, 0)),
        "2 bpp": bmp(struct.pack("<IiiHHIIiiII", 40, 4, 4, 1, 2, 0, 0, 0, 0, 0, 0)),
        "cut inside the header": b"BM" + b"\0" * 20,
    }


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    """host/raw_check.cpp as a plain host program: under AddressSanitizer and UBSan (its own main, the runtimes linked in
    statically), and without them for the run under an address-space limit"""
    d = tmp_path_factory.mktemp("rawcheck")
    san, plain = str(d / "raw_check_san"), str(d / "raw_check")
    src = os.path.join(HOST, "raw_check.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-o", san, src])
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", plain, src])
    return san, plain


def run_checker(exe, tmp_path, files, preexec_fn=None):
    bundle = tmp_path / "bundle.bin"
    bundle.write_bytes(b"".join(struct.pack("<I", len(f)) + f for f in files))
    r = subprocess.run([exe, str(bundle)], capture_output=True, text=True, preexec_fn=preexec_fn)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    verdicts = [l for l in r.stdout.splitlines() if l.startswith("verdicts ")][0][9:]
    assert len(verdicts) == len(files)
    return verdicts


def test_hostile_headers_are_refused_without_a_large_allocation(tool, checkers, tmp_path):
    """each is a decode failure of the service's decoder (decode_tool), and of raw_decode.h in a process that may not
    have more than 256 MiB of address space: a header's claim alone allocates nothing"""
    import resource
    files = hostile_files()
    for name, data in files.items():
        refused(tool, tmp_path, data, name.replace(" ", "_").replace("^", ""))

    def limit():
        resource.setrlimit(resource.RLIMIT_AS, (256 << 20, 256 << 20))

    assert run_checker(checkers[1], tmp_path, list(files.values()), preexec_fn=limit) == "R" * len(files)


def test_sanitized_decoder_over_fixtures_hostile_and_damaged_files(checkers, tmp_path):
    """raw_check under ASan + UBSan: every fixture file of this module is accepted, every hostile one refused, and every
    fixture cut short at many lengths or with bytes of its header overwritten is decoded or refused without a report"""
    rs = np.random.RandomState(13)
    good = [c[1] for c in bmp_matrix() + pnm_matrix() + rle_cases()]
    assert run_checker(checkers[0], tmp_path, good) == "A" * len(good)
    hostile = list(hostile_files().values())
    assert run_checker(checkers[0], tmp_path, hostile) == "R" * len(hostile)
    damaged = []
    for data in good[::3]:
        for cut in sorted(set([0, 1, 2, 13, 14, 17, 25, 26, 29, 53, 54, 65, 66] + rs.randint(0, len(data), 6).tolist())):
            damaged.append(data[:cut])
        for _ in range(12):
            b = bytearray(data)
            for _ in range(int(rs.randint(1, 4))):
                b[int(rs.randint(0, min(len(b), 70)))] = int(rs.choice([0, 1, 2, 3, 0x7F, 0x80, 0xFF, rs.randint(0, 256)]))
            damaged.append(bytes(b))
    run_checker(checkers[0], tmp_path, damaged)


def card_files(card):
    """{name: (file bytes, expected BGR)}: the card through a 200-colour palette as an 8-bit BMP, as a grey P5, and the
    same two pictures as 24-bit BMPs"""
    from PIL import Image
    pim = Image.fromarray(card[:, :, ::-1].copy()).quantize(200)
    pal = np.array(pim.getpalette()[:600], np.uint8).reshape(-1, 3)[:, ::-1]  # B,G,R
    idx = np.array(pim)
    grey = np.array(Image.fromarray(card[:, :, ::-1].copy()).convert("L"))[:, :, None]
    pal_bgr, grey_bgr = rw.lookup(idx, pal), rw.expected_pnm(5, grey)
    return {"bmp8": (rw.write_bmp(idx, 8, palette=pal), pal_bgr), "bmp8 as bmp24": (rw.write_bmp(pal_bgr, 24), pal_bgr),
            "p5": (rw.write_pnm(5, grey), grey_bgr), "p5 as bmp24": (rw.write_bmp(grey_bgr, 24), grey_bgr)}


def test_decode_image_returns_the_pixels_of_paletted_bmp_and_p5(tool, card, tmp_path):
    """the CPU half of the worker test (tests/test_gpu_raw.py): the service's decode_image on the card as an 8-bit paletted
    BMP and as a P5 file"""
    files = card_files(card)
    check_cases([(k, v[0], v[1]) for k, v in files.items()], tmp_path)


def test_descriptor_rules_are_refused_before_any_device_call(built, pkg):
    """every rule of ocr_raw_frame drives ocr_raw_decode to OCR_ERR_ARG with a message that names it - on a machine with
    or without a GPU: the check comes before the runtime is touched, so nothing was launched"""
    rows = np.zeros(5 * 12, np.uint8)

    def frame(**kw):
        f = pkg.RawFrame(kw.pop("w", 4), kw.pop("h", 5), kw.pop("kind", 5), kw.pop("bottom_up", 0), kw.pop("stride", 12), rows)
        for k, v in kw.items():
            setattr(f.c, k, v)
        return f

    def refused_as(f, what):
        with pytest.raises(pkg.OcrError, match=what) as e:
            f.decode()
        assert e.value.code == -1  # OCR_ERR_ARG

    refused_as(frame(kind=12), "kind")
    refused_as(frame(kind=-1), "kind")
    refused_as(frame(w=0), "positive")
    refused_as(frame(h=-3), "positive")
    refused_as(frame(w=70000, h=70000, stride=70000 * 3), "64 Mpixel")
    refused_as(frame(bottom_up=2), "bottom_up")
    refused_as(frame(stride=11), "row_stride is smaller")
    refused_as(frame(stride=(1 << 31) + 4), "2 GiB")
    refused_as(frame(data_len=59), "data_len")
    refused_as(frame(stride=13), "data_len")  # 4 * 13 + 12 = 64 > 60
    refused_as(frame(kind=10), "row_stride is smaller")  # RGB48BE needs 24 bytes a row
    refused_as(frame(data=None), "data_len")
