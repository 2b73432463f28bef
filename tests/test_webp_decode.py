"""Lossless WebP requests, host half (host/webp_decode.h): the container, prefix codes, LZ77, the colour cache and the host
pixel stage, which must return what cv::imdecode(IMREAD_COLOR) returns - the pixels of libwebp's WebPDecodeBGR.  The files are
written bit by bit (tests/webp_writer.py) and by libwebp's own encoder through Pillow; every decode is compared byte for byte
with the system's libwebp through ctypes and with the numpy statement of the inverse transforms (webp_writer.convert).  The
decoder runs in host/webp_check.cpp, a plain host program built with -fsanitize=address,undefined.  The device half is
tests/test_gpu_webp.py."""
import ctypes
import ctypes.util
import io
import itertools
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import webp_writer as ww  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cpp-paddle-ocr_amd", "host")
WIDTHS = [1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 65, 257]
HEIGHTS = [1, 2, 5, 17]
P, X, G, I = ww.PREDICTOR, ww.CROSS_COLOUR, ww.ADD_GREEN, ww.COLOUR_INDEXING
NOT_LOSSLESS = "lossy or animated WebP is not decoded"


def build_check(directory, *flags):
    exe = os.path.join(str(directory), "webp_check" + ("_san" if flags else ""))
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", *flags, "-o", exe, os.path.join(HOST, "webp_check.cpp")])
    return exe


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """host/webp_check.cpp with AddressSanitizer and UBSan: a stand-alone host program, nothing of it is loaded into Python"""
    return build_check(tmp_path_factory.mktemp("webpcheck"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


@pytest.fixture(scope="module")
def libwebp():
    name = ctypes.util.find_library("webp") or "libwebp.so.7"
    try:
        L = ctypes.CDLL(name)
    except OSError:
        pytest.skip("no libwebp on this machine")
    L.WebPDecodeBGR.restype = ctypes.c_void_p
    L.WebPDecodeBGR.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    L.WebPFree.argtypes = [ctypes.c_void_p]

    def decode(data):
        """WebPDecodeBGR: the (h, w, 3) image, None where libwebp refuses"""
        w, h = ctypes.c_int(), ctypes.c_int()
        p = L.WebPDecodeBGR(data, len(data), w, h)
        if not p:
            return None
        a = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), (h.value, w.value, 3)).copy()
        L.WebPFree(p)
        return a

    return decode


class Case:
    def __init__(self, name, data, want=None):
        self.name, self.data, self.want = name, data, want


def decode_all(exe, cases, directory):
    """every file through ONE webp_check --decode process; the decoded BGR arrays"""
    args = []
    for i, c in enumerate(cases):
        src = os.path.join(str(directory), "c%05d.webp" % i)
        with open(src, "wb") as f:
            f.write(c.data)
        args += [src, src + ".bgr"]
    r = subprocess.run([exe, "--decode"] + args, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    sizes = [tuple(int(v) for v in line.split()) for line in r.stdout.split("\n") if line]
    return [np.fromfile(os.path.join(str(directory), "c%05d.webp.bgr" % i), np.uint8).reshape(h, w, 3) for i, (w, h) in enumerate(sizes)]


def why(exe, data, directory, name="r.webp"):
    """webp_check --why: "ok w h device_ok" or "refused: reason"; the sanitizer build must exit without a report"""
    p = os.path.join(str(directory), name)
    with open(p, "wb") as f:
        f.write(data)
    r = subprocess.run([exe, "--why", p], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    return r.stdout.strip()


def legal_orders():
    """every file order of every subset of the four transforms"""
    out = [()]
    for n in range(1, 5):
        for sub in itertools.combinations((P, X, G, I), n):
            out += list(itertools.permutations(sub))
    return out


def case(rs, name, w, h, kinds, container="simple", **kw):
    """a writer file of random coded data and what it decodes to; meta=k: an entropy image of 2 + k % 4 prefix bits, 5 groups"""
    opts = {k: kw.pop(k) for k in ("values", "beyond", "bits", "modes", "colours") if k in kw}
    coded, transforms = ww.random_case(rs, w, h, kinds, **opts)
    if "meta" in kw:
        bits = 2 + kw.pop("meta") % 4
        kw["meta"] = (bits, rs.randint(0, 5, (ww.ceil_shift(h, bits), ww.ceil_shift(coded.shape[1], bits))))
    data = ww.write_webp(w, h, coded, transforms, container=container, rs=rs, **kw)
    return Case("%s %dx%d" % (name, w, h), data, ww.convert(w, h, coded, transforms))


def matrix(seed=1):
    """the writer's files, widths and heights taken in turn"""
    rs = np.random.RandomState(seed)
    sizes = itertools.cycle([(w, HEIGHTS[(i + j) % 4]) for j in range(4) for i, w in enumerate(WIDTHS)])
    cases = []

    def add(name, kinds, **kw):
        w, h = next(sizes)
        cases.append(case(rs, name, w, h, kinds, **kw))

    for mode in range(16):  # 14 and 15 are black, as 0
        for bits in (2, 3 + mode % 7):
            add("mode %d bits %d" % (mode, bits), (P,), modes=mode, bits=bits)
    for bits in range(2, 10):
        add("mode mix bits %d" % bits, (P,), bits=bits)
        add("cross bits %d" % bits, (X,), bits=bits)
    for order in legal_orders():
        for _ in range(2):
            add("order %s" % (order,), order, bits=2 + len(cases) % 4)
    for colours in (1, 2, 3, 4, 5, 16, 17, 256):
        for _ in range(3):
            add("%d colours" % colours, (I,), colours=colours)
        add("%d colours, indices beyond" % colours, (I,), colours=colours, beyond=True)
        add("%d colours under a predictor" % colours, (I, G, P), colours=colours)
    for cache_bits in (0, 1, 6, 11):
        for values in (3, 40):
            add("cache %d values %d" % (cache_bits, values), (), cache_bits=cache_bits, values=values)
            add("cache %d values %d with copies" % (cache_bits, values), (G,), cache_bits=cache_bits, values=values, lz=dict(codes=list(range(1, 130)), prob=0.3))
    for k in range(8):
        add("entropy image", (P,), meta=k, values=5 + 30 * (k % 2), cache_bits=(0, 4)[k % 2], lz=dict(codes=[1, 2, 121, 125], prob=0.2) if k % 3 == 0 else None)
    for k in range(6):
        add("code forms", (), values=(1, 2, 16, 16, 300, 3)[k], code_opts=dict(form=("auto", "normal")[k % 2], repeats=k < 4, max_symbol=k % 3 == 0, skew=k in (2, 3)))
    for k in range(4):
        add("vp8x", ((), (P,), (I,), (G, X, P))[k], container="vp8x", colours=7)
    return cases


@pytest.fixture(scope="module")
def decoded(checker, tmp_path_factory):
    cases = matrix()
    return cases, decode_all(checker, cases, tmp_path_factory.mktemp("webpfiles"))


def test_the_matrix_covers_the_case_list(tmp_path):
    cases = matrix()
    names = " | ".join(c.name for c in cases)
    assert len(legal_orders()) == 65
    for w in WIDTHS:
        assert (" %dx" % w) in names
    for what in ["mode 13 bits 2", "mode mix bits 9", "cross bits 9", "order (3, 2, 1, 0)", "256 colours, indices beyond", "cache 11 values 3 with copies",
                 "entropy image", "code forms", "vp8x"]:
        assert what in names
    # back references: each of the 120 short codes, long distances, overlaps (distance 1, longer copies) and copies across row ends
    rs = np.random.RandomState(5)
    used = set()
    px = rs.randint(0, 2, 40 * 50).astype(np.uint32)
    tokens = ww.tokenize(px, 40, 0, dict(codes=list(range(1, 140)), prob=0.9), rs, used)
    assert set(range(1, 121)) <= used and max(used) > 120
    copies = [t for t in tokens if t[0] == 1]
    assert any(t[1] > ww.plane_distance(t[2], 40) for t in copies), "an overlapping copy"
    pos, crossing = 0, 0
    for t in tokens:
        n = t[1] if t[0] == 1 else 1
        crossing += t[0] == 1 and pos // 40 != (pos + n - 1) // 40
        pos += n
    assert crossing > 0


def test_decoder_equals_the_numpy_rules(decoded):
    cases, got = decoded
    for c, g in zip(cases, got):
        assert g.shape == c.want.shape and np.array_equal(g, c.want), (c.name, int((g != c.want).sum()))


def test_decoder_equals_libwebp(decoded, libwebp):
    cases, got = decoded
    for c, g in zip(cases, got):
        ref = libwebp(c.data)
        assert ref is not None, c.name
        assert g.shape == ref.shape and np.array_equal(g, ref), (c.name, int((g != ref).sum()))


def test_every_short_distance_code_decodes_as_libwebp(checker, libwebp, tmp_path):
    """a two-valued 40 x 50 image coded with copies through every short code and long distances, with and without a cache"""
    cases = []
    for cache_bits in (0, 3):
        rs = np.random.RandomState(5)
        used = set()
        coded = rs.randint(0, 2, (50, 40)).astype(np.uint32) * np.uint32(0x00C0FFEE) | np.uint32(0xFF000000)
        data = ww.write_webp(40, 50, coded, (), rs=rs, cache_bits=cache_bits, lz=dict(codes=list(range(1, 140)), prob=0.9), used_codes=used)
        assert set(range(1, 121)) <= used
        cases.append(Case("short codes, cache %d" % cache_bits, data, ww.convert(40, 50, coded, ())))
    for c, g in zip(cases, decode_all(checker, cases, tmp_path)):
        assert np.array_equal(g, c.want) and np.array_equal(g, libwebp(c.data)), c.name


def pillow_images():
    rs = np.random.RandomState(11)
    card = np.load(os.path.join(ROOT, "tests", "golden", "card_jd_bgr.npy"))
    ramp = np.add.outer(np.arange(70) * 3, np.arange(130)).astype(np.uint8)
    few = lambda n, c=3: rs.randint(0, 256, (n, c)).astype(np.uint8)[rs.randint(0, n, (66, 65))]
    return {"rgb noise": rs.randint(0, 256, (33, 65, 3)).astype(np.uint8), "rgba noise": rs.randint(0, 256, (17, 31, 4)).astype(np.uint8),
            "gradient": np.stack([ramp, ramp.T[:70, :70].repeat(2, 1)[:, :130], 255 - ramp], 2), "card": np.ascontiguousarray(card[:120, :257, ::-1]),
            "2 colours": few(2), "4 colours": few(4), "16 colours": few(16), "200 colours": few(200), "16 colours with alpha": few(16, 4)}


def pillow_file(arr, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "WEBP", lossless=True, **kw)
    return buf.getvalue()


def test_files_of_libwebps_encoder(checker, libwebp, tmp_path):
    """Pillow's lossless encoder, methods 0 .. 6 x qualities 0 / 50 / 100 x exact on / off over noise, gradients, the text card
    and images of 2, 4, 16 and 200 colours: the decoder, libwebp and Pillow's own decode agree"""
    pytest.importorskip("PIL")
    from PIL import Image, features
    if not features.check("webp"):
        pytest.skip("Pillow without WebP")
    cases = []
    for name, arr in pillow_images().items():
        for method in range(7):
            for quality in (0, 50, 100):
                exact = (method + quality // 50) % 2 == 0
                cases.append(Case("%s method %d quality %d exact %d" % (name, method, quality, exact), pillow_file(arr, method=method, quality=quality, exact=exact)))
    got = decode_all(checker, cases, tmp_path)
    for c, g in zip(cases, got):
        ref = libwebp(c.data)
        assert ref is not None and g.shape == ref.shape and np.array_equal(g, ref), c.name
        pil = np.asarray(Image.open(io.BytesIO(c.data)).convert("RGB"))[:, :, ::-1]
        assert np.array_equal(g, pil), c.name
    r = subprocess.run([checker, "--why"] + [os.path.join(str(tmp_path), "c%05d.webp" % i) for i in range(len(cases))], capture_output=True, text=True)
    assert {line.split()[-1] for line in r.stdout.strip().split("\n")} == {"1"}, "every file of libwebp's encoder is in the device stage's scope"


def vp8l_of(w, h, rs, **kw):
    coded, transforms = ww.random_case(rs, w, h, (G, P), bits=2)
    return ww.write_vp8l(w, h, coded, transforms, rs=rs, **kw)


def test_lossy_and_animated_files_are_refused_in_so_many_words(checker, tmp_path):
    body = vp8l_of(4, 4, np.random.RandomState(2))
    anim = ww.riff([ww.vp8x(4, 4, 0x02), ww.chunk(b"ANIM", bytes(6)), ww.chunk(b"ANMF", bytes(16) + ww.chunk(b"VP8L", body))])
    assert NOT_LOSSLESS in why(checker, anim, tmp_path)
    unflagged = ww.riff([ww.vp8x(4, 4, 0), ww.chunk(b"ANMF", bytes(16) + ww.chunk(b"VP8L", body))])
    assert NOT_LOSSLESS in why(checker, unflagged, tmp_path)
    assert NOT_LOSSLESS in why(checker, ww.riff([ww.chunk(b"VP8 ", bytes(20))]), tmp_path)
    assert NOT_LOSSLESS in why(checker, ww.riff([ww.vp8x(4, 4, 0x10), ww.chunk(b"ALPH", bytes(5)), ww.chunk(b"VP8 ", bytes(20))]), tmp_path)
    PIL = pytest.importorskip("PIL")
    from PIL import Image, features
    if not features.check("webp"):
        pytest.skip("Pillow without WebP")
    rs = np.random.RandomState(3)
    rgb = rs.randint(0, 256, (20, 30, 3)).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "WEBP", quality=80)
    assert NOT_LOSSLESS in why(checker, buf.getvalue(), tmp_path)
    buf = io.BytesIO()
    Image.fromarray(np.dstack([rgb, rgb[:, :, :1]])).save(buf, "WEBP", quality=80)
    assert NOT_LOSSLESS in why(checker, buf.getvalue(), tmp_path)
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "WEBP", lossless=True, save_all=True, append_images=[Image.fromarray(255 - rgb)], duration=100)
    assert NOT_LOSSLESS in why(checker, buf.getvalue(), tmp_path)


def put_lengths(bw, lengths):
    """a normal-form code with exactly these lengths, no repeats"""
    ww.put_normal_code(bw, lengths, repeats=False)


def hand_image(width, height, green_lengths, tail_bits=64, version=0, transforms=()):
    """a file whose main image's green code has the given lengths (the other four codes are single symbols); zero bits follow"""
    bw = ww.Bits()
    ww.put_header(bw, width, height, 0, version)
    for kind in transforms:
        bw.put(1, 1); bw.put(kind, 2)
    bw.put(0, 1)  # no more transforms
    bw.put(0, 1)  # no cache
    bw.put(0, 1)  # no meta image
    put_lengths(bw, green_lengths + [0] * (280 - len(green_lengths)))
    for _ in range(4):
        bw.put(1, 1); bw.put(0, 1); bw.put(0, 1); bw.put(0, 1)
    for _ in range(tail_bits):
        bw.put(0, 1)
    return ww.riff([ww.chunk(b"VP8L", bw.bytes())])


def test_malformed_files_are_refused_as_libwebp_refuses_them(checker, libwebp, tmp_path):
    rs = np.random.RandomState(4)
    good = hand_image(3, 2, [1, 2, 2])
    assert why(checker, good, tmp_path).startswith("ok 3 2") and libwebp(good) is not None
    bad = {"over-subscribed": hand_image(3, 2, [1, 1, 1]), "incomplete": hand_image(3, 2, [1, 2, 3]), "no symbol": hand_image(3, 2, [0, 0, 0]),
           "version": hand_image(3, 2, [1, 2, 2], version=1), "repeated transform": hand_image(3, 2, [1, 2, 2], transforms=(G, G)),
           "data ends": hand_image(40, 40, [1, 2, 2], tail_bits=0)}
    # a distance before the start: the first token of the image is a copy
    bw = ww.Bits()
    ww.put_header(bw, 3, 2)
    bw.put(0, 3)
    hist = [0] * 280
    hist[256] = 1
    hist[5] = 1
    words = [ww.put_code(bw, h) for h in (hist, [1], [1], [1], [1])]
    bw.code(words[0][256])
    bw.put(0, 64)
    bad["distance before the start"] = ww.riff([ww.chunk(b"VP8L", bw.bytes())])
    body = vp8l_of(5, 4, rs)
    whole = ww.riff([ww.chunk(b"VP8L", body)])
    bad["chunk size beyond the file"] = whole[:16] + struct.pack("<I", len(body) + 7) + whole[20:]
    bad["riff size beyond the file"] = whole[:4] + struct.pack("<I", len(whole)) + whole[8:]
    bw = ww.Bits()
    ww.put_header(bw, 16384, 16384)
    bw.put(0, 64)
    bad["64 Mpixel"] = ww.riff([ww.chunk(b"VP8L", bw.bytes())])
    bad["canvas"] = ww.riff([ww.vp8x(5, 5), ww.chunk(b"VP8L", body)])
    bad["not a chunk in front"] = ww.riff([ww.chunk(b"JUNK", b"1234"), ww.chunk(b"VP8L", body)])
    for name, data in bad.items():
        assert why(checker, data, tmp_path).startswith("refused"), name
        if name not in ("64 Mpixel", "chunk size beyond the file", "riff size beyond the file"):
            assert libwebp(data) is None, name
    assert "twice" in why(checker, bad["repeated transform"], tmp_path) and "version" in why(checker, bad["version"], tmp_path)
    assert "before the image" in why(checker, bad["distance before the start"], tmp_path)
    assert "64 Mpixel" in why(checker, bad["64 Mpixel"], tmp_path) and "chunk size" in why(checker, bad["chunk size beyond the file"], tmp_path)
    # a single symbol of any length is a code (libwebp's rule): zero bits a pixel
    one = hand_image(3, 2, [0, 3], tail_bits=0)
    assert why(checker, one, tmp_path).startswith("ok") and libwebp(one) is not None


def test_a_file_cut_at_every_byte(checker, libwebp, tmp_path):
    """every proper prefix of a small VP8X file (metadata chunks in front of and behind the image) is refused, without a
    sanitizer report.  Where libwebp decides otherwise is recorded in `differs`: nowhere - WebPDecodeBGR holds a whole-buffer
    decode to the RIFF size too, so a cut behind the image chunk is refused by both, like every cut inside it"""
    rs = np.random.RandomState(6)
    coded, transforms = ww.random_case(rs, 9, 5, (G, X, P), bits=2, values=6)
    data = ww.write_webp(9, 5, coded, transforms, container="vp8x", rs=rs, cache_bits=2, lz=dict(codes=[1, 2, 3], prob=0.3))
    assert why(checker, data, tmp_path).startswith("ok 9 5")
    start = data.index(b"VP8L")
    end = start + 8 + struct.unpack("<I", data[start + 4:start + 8])[0]
    paths = []
    for n in range(len(data)):
        p = tmp_path / ("cut%04d" % n)
        p.write_bytes(data[:n])
        paths.append(str(p))
    r = subprocess.run([checker, "--why"] + paths, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(data) and all(line.startswith("refused") for line in lines)
    differs = [n for n in range(len(data)) if libwebp(data[:n]) is not None]
    assert all(n >= end for n in differs), "libwebp decodes no file cut inside the image chunk either"
    assert differs == [], "nor one cut behind it"


def webp_frame(pkg, **kw):
    """a sound 4 x 5 frame with add-green and a predictor, then the overrides"""
    w, h = kw.pop("w", 4), kw.pop("h", 5)
    transforms = kw.pop("transforms", [(G, 0, None), (P, 2, np.zeros((2, 1), np.uint32))])
    f = pkg.WebpFrame(w, h, np.zeros(kw.pop("coded", 20), np.uint32), transforms)
    for k, v in kw.items():
        setattr(f.c, k, v)
    return f


def test_descriptor_rules_are_refused_before_any_device_call(built, pkg):
    """every rule of ocr_webp_frame drives ocr_webp_decode to OCR_ERR_ARG with a message that names it - on a machine with or
    without a GPU: the check comes before the runtime is touched, so nothing was launched"""
    def refused_as(f, what):
        with pytest.raises(pkg.OcrError, match=what) as e:
            f.decode()
        assert e.value.code == -1  # OCR_ERR_ARG

    pal = np.zeros(3, np.uint32)
    sub = np.zeros(4, np.uint32)
    refused_as(webp_frame(pkg, width=0), "1 .. 16384")
    refused_as(webp_frame(pkg, height=-3), "1 .. 16384")
    refused_as(webp_frame(pkg, width=16385), "1 .. 16384")
    refused_as(webp_frame(pkg, width=16384, height=16384), "64 Mpixel")
    refused_as(webp_frame(pkg, ntransforms=5), "at most four")
    refused_as(webp_frame(pkg, ntransforms=-1), "at most four")
    refused_as(webp_frame(pkg, transforms=[(4, 0, None)]), "kind must be")
    refused_as(webp_frame(pkg, transforms=[(G, 0, None), (G, 0, None)]), "twice")
    refused_as(webp_frame(pkg, transforms=[(P, 1, sub)]), "block bits")
    refused_as(webp_frame(pkg, transforms=[(X, 10, sub)]), "block bits")
    refused_as(webp_frame(pkg, transforms=[(P, 2, np.zeros(1, np.uint32))]), "sub-image")
    refused_as(webp_frame(pkg, transforms=[(X, 2, None)]), "sub-image")
    refused_as(webp_frame(pkg, transforms=[(G, 1, None)]), "add-green")
    refused_as(webp_frame(pkg, transforms=[(I, 2, np.zeros(0, np.uint32))]), "palette")
    refused_as(webp_frame(pkg, transforms=[(I, 0, np.zeros(257, np.uint32))]), "palette")
    refused_as(webp_frame(pkg, transforms=[(I, 3, pal)]), "bundling bits")
    refused_as(webp_frame(pkg, transforms=[(G, 0, None), (I, 2, pal)]), "colour indexing must be the first")
    refused_as(webp_frame(pkg, coded=19), "fewer coded pixels")
    refused_as(webp_frame(pkg, argb=None), "fewer coded pixels")
    refused_as(webp_frame(pkg, transforms=[(I, 2, pal)], coded=4), "fewer coded pixels")  # 4 wide at 2 bits: one coded pixel a row, 5 rows
