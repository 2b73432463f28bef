"""Writes tests/golden/webp/: a dozen lossless WebP files from libwebp's own encoder (through Pillow: methods 0, 4 and 6 over an
RGB, an RGBA, a 2-colour and a 16-colour image, 65 x 66 and 130 x 33), each beside the pixels WebPDecodeBGR returns for it
(.npy).  With them the GPU suite sees real encoder output on a machine that has neither libwebp nor Pillow's WebP support.

    python tests/golden/make_webp_fixtures.py        (needs Pillow with WebP and libwebp; the files are committed)"""
import ctypes
import ctypes.util
import io
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "webp")


def webp_decode_bgr(data):
    L = ctypes.CDLL(ctypes.util.find_library("webp") or "libwebp.so.7")
    L.WebPDecodeBGR.restype = ctypes.c_void_p
    L.WebPDecodeBGR.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    L.WebPFree.argtypes = [ctypes.c_void_p]
    w, h = ctypes.c_int(), ctypes.c_int()
    p = L.WebPDecodeBGR(data, len(data), w, h)
    assert p
    a = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), (h.value, w.value, 3)).copy()
    L.WebPFree(p)
    return a


def images():
    rs = np.random.RandomState(2024)
    card = np.load(os.path.join(HERE, "card_jd_bgr.npy"))[:, :, ::-1]
    rgb = card[20:86, 30:95].astype(int) + rs.randint(-6, 7, (66, 65, 3))
    rgba = np.dstack([card[40:73, 10:140], rs.randint(0, 256, (33, 130, 1))])
    two = rs.randint(0, 256, (2, 3))[(card[10:76, 100:165].mean(2) > 128).astype(int)]
    sixteen = rs.randint(0, 256, (16, 3))[(card[30:63, 60:190].mean(2).astype(int) >> 4)]
    return {"rgb_65x66": rgb, "rgba_130x33": rgba, "two_65x66": two, "sixteen_130x33": sixteen}


def main():
    os.makedirs(OUT, exist_ok=True)
    for name, arr in images().items():
        for method in (0, 4, 6):
            buf = io.BytesIO()
            Image.fromarray(np.clip(arr, 0, 255).astype(np.uint8)).save(buf, "WEBP", lossless=True, method=method, quality=75, exact=True)
            data = buf.getvalue()
            assert len(data) < 16384, (name, method, len(data))
            stem = os.path.join(OUT, "%s_m%d" % (name, method))
            with open(stem + ".webp", "wb") as f:
                f.write(data)
            np.save(stem + ".npy", webp_decode_bgr(data))
            print(os.path.basename(stem), len(data))


if __name__ == "__main__":
    main()
