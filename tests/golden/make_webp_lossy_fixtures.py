"""Writes tests/golden/webp_lossy/: lossy WebP files from libwebp's own encoder (through Pillow: quality 5, 50, 90 and 100,
methods 0, 4 and 6, over a photo-like, a flat two-tone and a text crop of the card, each plus noise, at 1 x 1, 15 x 17, 16 x 16,
17 x 33, 65 x 66, 130 x 33 and 257 x 49, one of them from an RGBA source so that a VP8X + ALPH file is in the set), each beside
the pixels WebPDecodeBGR returns for it (.npy).  The whole card at quality 90 is there twice, bare and wrapped into a VP8X
container: the service test sends it.  With these files the GPU suite sees real encoder output on a machine that has neither
libwebp nor Pillow's WebP support.

The script parses every file with host/vp8_check (built here when missing) and asserts that the set holds B_PRED macroblocks
in at least three files, a file with four segments and a file with skipped macroblocks.

    python tests/golden/make_webp_lossy_fixtures.py        (needs Pillow with WebP, libwebp and g++; the files are committed)
    python tests/golden/make_webp_lossy_fixtures.py --card960 <out.webp>
        only the file profiles/webp_lossy_pixel_stage.json was measured on: the card tiled to 960 x 960, quality 75, method 4
        (88 KB: made where it is needed, not committed)"""
import io
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_webp_fixtures import webp_decode_bgr  # noqa: E402

OUT = os.path.join(HERE, "webp_lossy")
HOST = os.path.join(HERE, "..", "..", "cpp-paddle-ocr_amd", "host")
SIZES = [(1, 1), (15, 17), (16, 16), (17, 33), (65, 66), (130, 33), (257, 49)]  # width x height
MB_DTYPE = np.dtype([("modes", "u1", 16), ("is_i4x4", "u1"), ("uvmode", "u1"), ("level", "u1"), ("ilevel", "u1"), ("hev", "u1"), ("inner", "u1"),
                     ("segment", "u1"), ("skip", "u1"), ("nz_y", "<u4"), ("nz_uv", "<u4"), ("present", "<u4"), ("coeff_off", "<u4")])


def checker():
    exe = os.path.join(HOST, "vp8_check")
    if not os.path.exists(exe):
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(HOST, "vp8_check.cpp")], check=True)
    return exe


def read_frames(blob):
    """the descriptors vp8_check --frame writes -> [{width, height, filter_type, partitions, segments, mbs, coeffs}]"""
    out, at = [], 0
    while at < len(blob):
        w, h, ft, parts, segs = struct.unpack_from("<5i", blob, at)
        n, = struct.unpack_from("<Q", blob, at + 20)
        mbs = np.frombuffer(blob, MB_DTYPE, n, at + 28)
        at += 28 + 40 * n
        m, = struct.unpack_from("<Q", blob, at)
        coeffs = np.frombuffer(blob, "<i2", m, at + 8)
        at += 8 + 2 * m
        out.append(dict(width=w, height=h, filter_type=ft, partitions=parts, segments=segs, mbs=mbs, coeffs=coeffs))
    return out


def frame_of(path):
    with tempfile.TemporaryDirectory() as tmp:
        dump = os.path.join(tmp, "f.bin")
        subprocess.run([checker(), "--frame", path, dump], check=True)
        with open(dump, "rb") as f:
            return read_frames(f.read())[0]


def crops():
    rs = np.random.RandomState(2025)
    card = np.load(os.path.join(HERE, "card_jd_bgr.npy"))[:, :, ::-1].astype(int)

    def fit(a, w, h):  # tile and cut to h x w
        reps = (-(-h // a.shape[0]), -(-w // a.shape[1]), 1)
        return np.tile(a, reps)[:h, :w]

    def photo(w, h):  # smooth gradients of the card's colours, enlarged
        small = card[::12, ::12][:9, :23]
        big = np.asarray(Image.fromarray(small.astype(np.uint8)).resize((max(w, 2), max(h, 2)), Image.BICUBIC)).astype(int)
        return big[:h, :w] + rs.randint(-10, 11, (h, w, 3))

    def flat(w, h):
        tone = np.array([[30, 60, 200], [220, 210, 40]])[(fit(card[10:90, 100:300], w, h).mean(2) > 128).astype(int)]
        return tone + rs.randint(-3, 4, (h, w, 3))

    def text(w, h):
        return fit(card[20:120, 30:320], w, h) + rs.randint(-6, 7, (h, w, 3))

    return {"photo": photo, "flat": flat, "text": text}


def vp8x_wrap(data, w, h):
    """a bare RIFF / WEBP / VP8 file -> the same image inside a VP8X container (no flags)"""
    assert data[12:16] == b"VP8 "
    body = data[12:]
    x = b"VP8X" + struct.pack("<I", 10) + bytes(4) + struct.pack("<I", w - 1)[:3] + struct.pack("<I", h - 1)[:3]
    return b"RIFF" + struct.pack("<I", 4 + len(x) + len(body)) + b"WEBP" + x + body


def main():
    os.makedirs(OUT, exist_ok=True)
    kinds = crops()
    rs = np.random.RandomState(7)
    plan = []
    qualities, methods, names = [5, 50, 90, 100], [0, 4, 6], ["photo", "flat", "text"]
    k = 0
    for (w, h) in SIZES:  # every size with every kind; qualities and methods go round
        for name in names:
            plan.append((name, w, h, qualities[k % 4], methods[(k // 4 + k) % 3], False))
            k += 1
    plan.append(("text", 130, 33, 50, 4, True))  # RGBA: VP8X + ALPH
    stats = dict(bpred=0, seg4=0, skipped=0)
    for name, w, h, q, m, alpha in plan:
        arr = np.clip(kinds[name](w, h), 0, 255).astype(np.uint8)
        if alpha:
            arr = np.dstack([arr, rs.randint(0, 256, (h, w, 1)).astype(np.uint8)])
        buf = io.BytesIO()
        Image.fromarray(arr).save(buf, "WEBP", quality=q, method=m)
        data = buf.getvalue()
        assert len(data) < 16384, (name, w, h, q, m, len(data))
        assert (b"ALPH" in data[:64]) == alpha
        stem = os.path.join(OUT, "%s%s_%dx%d_q%d_m%d" % (name, "_rgba" if alpha else "", w, h, q, m))
        with open(stem + ".webp", "wb") as f:
            f.write(data)
        np.save(stem + ".npy", webp_decode_bgr(data))
        fr = frame_of(stem + ".webp")
        stats["bpred"] += bool(fr["mbs"]["is_i4x4"].any())
        stats["seg4"] += len(set(fr["mbs"]["segment"].tolist())) == 4
        stats["skipped"] += bool(fr["mbs"]["skip"].any())
        print(os.path.basename(stem), len(data))
    card = np.load(os.path.join(HERE, "card_jd_bgr.npy"))[:, :, ::-1]
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(card)).save(buf, "WEBP", quality=90, method=4)
    bare = buf.getvalue()
    h, w = card.shape[:2]
    for stem, data in (("card_q90", bare), ("card_q90_vp8x", vp8x_wrap(bare, w, h))):
        with open(os.path.join(OUT, stem + ".webp"), "wb") as f:
            f.write(data)
        print(stem, len(data))
    np.save(os.path.join(OUT, "card_q90.npy"), webp_decode_bgr(bare))
    assert (webp_decode_bgr(vp8x_wrap(bare, w, h)) == webp_decode_bgr(bare)).all()
    print(stats)
    assert stats["bpred"] >= 3 and stats["seg4"] >= 1 and stats["skipped"] >= 1, stats


def card960(out):
    card = np.load(os.path.join(HERE, "card_jd_bgr.npy"))[:, :, ::-1]
    big = np.ascontiguousarray(np.tile(card, (6, 3, 1))[:960, :960])
    Image.fromarray(big).save(out, "WEBP", quality=75, method=4)
    print(out, os.path.getsize(out))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--card960":
        card960(sys.argv[2])
    else:
        main()
