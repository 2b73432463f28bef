"""Writes tests/golden/jp2: small JPEG 2000 files of OpenJPEG's encoder (through Pillow) - reversible and irreversible, every
progression order, layers, precincts, code-block sizes, tiles with odd offsets, JP2 and bare codestreams, 8-bit grey / RGB /
RGBA and 16-bit grey - each with the pixels OpenJPEG's decoder returns for it as cv::imdecode(IMREAD_COLOR) would hand them on
(.npy: BGR, alpha dropped, 16 bits reduced by >> 8).  The card used for the other formats is there at 208 x 104, once per
transform (card_53.jp2, card_97_bare.j2k).  With them the GPU tests need neither OpenJPEG nor this script.

    python tests/golden/make_jp2_fixtures.py
    python tests/golden/make_jp2_fixtures.py --card960 <out stem>
        only the files profiles/j2k_pixel_stage.json was measured on: the card tiled to 960 x 960, <stem>_53.jp2 and <stem>_97.jp2, 6 resolutions
"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "jp2")


def encode(arr, **kw):
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG2000", **kw)
    return buf.getvalue()


def decoded_bgr(data):
    im = Image.open(io.BytesIO(data))
    im.load()
    a = np.asarray(im)
    if a.dtype != np.uint8:
        a = (a.astype(np.uint16) >> 8).astype(np.uint8)
    if a.ndim == 2:
        a = np.repeat(a[:, :, None], 3, 2)
    return np.ascontiguousarray(a[:, :, :3][:, :, ::-1])


def card(w, h):
    rgb = np.load(os.path.join(HERE, "card_jd_bgr.npy"))[:, :, ::-1]
    return np.asarray(Image.fromarray(np.ascontiguousarray(rgb)).resize((w, h), Image.LANCZOS))


def samples(rs, mode, w, h):
    base = np.asarray(Image.fromarray(card(208, 104)).resize((w, h), Image.BILINEAR)).astype(int)
    base = np.clip(base + rs.randint(-8, 9, base.shape), 0, 255)
    if mode == "L":
        return base[:, :, 1].astype(np.uint8)
    if mode == "I;16":
        return (base[:, :, 1] * 257 + rs.randint(0, 200, (h, w))).astype(np.uint16)
    if mode == "RGBA":
        return np.dstack([base, rs.randint(0, 256, (h, w, 1))]).astype(np.uint8)
    return base.astype(np.uint8)


PLAN = [  # (stem, mode, w, h, options)
    ("l_1x1", "L", 1, 1, {}),
    ("rgb_17x33_lrcp", "RGB", 17, 33, dict(progression="LRCP", quality_layers=[8, 2], quality_mode="rates", irreversible=True)),
    ("rgb_65x33_rlcp", "RGB", 65, 33, dict(progression="RLCP", num_resolutions=3)),
    ("rgb_129x65_rpcl", "RGB", 129, 65, dict(progression="RPCL", precinct_size=(32, 32), codeblock_size=(16, 16), num_resolutions=4)),
    ("rgb_64x64_pcrl", "RGB", 64, 64, dict(progression="PCRL", irreversible=True, precinct_size=(64, 64))),
    ("rgb_63x31_cprl", "RGB", 63, 31, dict(progression="CPRL", quality_layers=[20, 5, 1], quality_mode="rates")),
    ("rgba_31x5", "RGBA", 31, 5, {}),
    ("rgba_33x32_97", "RGBA", 33, 32, dict(irreversible=True)),
    ("g16_17x31", "I;16", 17, 31, {}),
    ("g16_64x16_97", "I;16", 64, 16, dict(irreversible=True)),
    ("l_257x3_cb1024", "L", 257, 3, dict(codeblock_size=(1024, 4))),
    ("l_3x257", "L", 3, 257, dict(codeblock_size=(4, 4))),
    ("rgb_9x9_res4", "RGB", 9, 9, dict(num_resolutions=4)),
    ("rgb_5x3_res2", "RGB", 5, 3, dict(num_resolutions=2)),
    ("rgb_32x32_res1", "RGB", 32, 32, dict(num_resolutions=1, irreversible=True)),
    ("rgb_65x64_tiles_odd", "RGB", 65, 64, dict(tile_size=(17, 13), offset=(3, 5), tile_offset=(1, 2))),
    ("rgb_65x64_tiles32", "RGB", 65, 64, dict(tile_size=(32, 32), offset=(1, 1), tile_offset=(1, 1), num_resolutions=3)),
    ("rgb_66x64_tiles32_97", "RGB", 66, 64, dict(tile_size=(32, 32), offset=(1, 1), tile_offset=(1, 1), irreversible=True, num_resolutions=3)),
    ("l_16x17_offset", "L", 16, 17, dict(offset=(1, 1), tile_offset=(0, 0), tile_size=(64, 64))),
    ("rgb_33x17_nomct", "RGB", 33, 17, dict(mct=0)),
    ("rgb_33x17_nomct_97", "RGB", 33, 17, dict(mct=0, irreversible=True)),
    ("rgb_17x16_bare", "RGB", 17, 16, dict(no_jp2=True)),
    ("l_33x33_bare_97", "L", 33, 33, dict(no_jp2=True, irreversible=True)),
    ("rgb_31x32_plt", "RGB", 31, 32, dict(plt=True)),
    ("rgb_130x65_cb64", "RGB", 130, 65, dict(codeblock_size=(64, 64), irreversible=True, quality_layers=[30], quality_mode="rates")),
]


def main():
    os.makedirs(OUT, exist_ok=True)
    rs = np.random.RandomState(2000)
    todo = [(stem, samples(rs, mode, w, h), kw) for stem, mode, w, h, kw in PLAN]
    c = card(208, 104)
    todo += [("card_53", c, {}), ("card_97_bare", c, dict(irreversible=True, no_jp2=True, quality_layers=[40], quality_mode="dB"))]
    for stem, arr, kw in todo:
        data = encode(arr, **kw)
        with open(os.path.join(OUT, stem + (".j2k" if kw.get("no_jp2") else ".jp2")), "wb") as f:
            f.write(data)
        np.save(os.path.join(OUT, stem + ".npy"), decoded_bgr(data))
        print(stem, len(data))


def card960(stem):
    rgb = np.load(os.path.join(HERE, "card_jd_bgr.npy"))[:, :, ::-1]
    big = np.ascontiguousarray(np.tile(rgb, (6, 3, 1))[:960, :960])
    for name, kw in (("_53", {}), ("_97", dict(irreversible=True, quality_layers=[40], quality_mode="dB"))):
        with open(stem + name + ".jp2", "wb") as f:
            f.write(encode(big, num_resolutions=6, **kw))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--card960":
        card960(sys.argv[2])
    else:
        main()
