"""JPEG 2000 coded descriptors for the tests: the file form host/j2k_check writes with --coded and reads with --tier1 (the frame
before tier-1: code-block records and one byte pool), and random code blocks.  The MQ decoder turns any bytes into some
coefficients, so random blocks need no encoder."""
import os
import struct
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import j2k_frames as jf  # noqa: E402

CBLK = np.dtype([("tc", "<u4"), ("at", "<u4"), ("byte_off", "<u8"), ("byte_len", "<u4"), ("w", "<u2"), ("h", "<u2"), ("orient", "u1"), ("numbps", "u1"),
                 ("passes", "u1"), ("reserved", "u1"), ("reserved2", "<u4")])
assert CBLK.itemsize == 32

# what the random-block test crosses
SIZES = [(1, 1), (1, 5), (5, 1), (3, 4), (4, 3), (7, 9), (16, 16), (33, 31), (64, 64), (64, 63), (1024, 4), (4, 1024), (2, 1000)]
NUMBPS = [1, 2, 9, 30]
PASSES = [1, 2, 3, 4, None]  # None: 3 * numbps - 2, all a block can have
SEGMENTS = ["empty", "one", "short", "ample", "zeros", "ff", "marker", "ends_ff"]


def write_coded(path, coded):
    with open(path, "wb") as f:
        for cd in coded:
            head = [cd.get(k, 0) for k in jf.HEAD]
            head[8:11] = list(cd["chan"])
            tcs = np.ascontiguousarray(cd["tcs"], jf.TC)
            steps = np.ascontiguousarray(cd["steps"], "<f4")
            cblks = np.ascontiguousarray(cd["cblks"], CBLK)
            data = np.ascontiguousarray(cd["bytes"], np.uint8)
            f.write(struct.pack("<24i", *head) + struct.pack("<Q", len(tcs)) + tcs.tobytes() + struct.pack("<Q", len(steps)) + steps.tobytes() +
                    struct.pack("<Q", cd["ncoeffs"]) + struct.pack("<Q", len(cblks)) + cblks.tobytes() + struct.pack("<Q", len(data)) + data.tobytes())


def read_coded(path):
    blob, out, at = open(path, "rb").read(), [], 0
    while at < len(blob):
        cd = dict(zip(jf.HEAD, struct.unpack_from("<24i", blob, at)))
        cd["chan"] = [cd.pop("chan0"), cd.pop("chan1"), cd.pop("chan2")]
        at += 96
        for key, dt, size in (("tcs", jf.TC, 40), ("steps", "<f4", 4)):
            n, = struct.unpack_from("<Q", blob, at)
            cd[key] = np.frombuffer(blob, dt, n, at + 8).copy()
            at += 8 + size * n
        cd["ncoeffs"], = struct.unpack_from("<Q", blob, at)
        at += 8
        for key, dt, size in (("cblks", CBLK, 32), ("bytes", np.uint8, 1)):
            n, = struct.unpack_from("<Q", blob, at)
            cd[key] = np.frombuffer(blob, dt, n, at + 8).copy()
            at += 8 + size * n
        out.append(cd)
    return out


def host_tier1(exe, directory, coded, name="coded"):
    """j2k::tier1 over coded descriptors (j2k_check --tier1): the frames, as jf.read_frames gives them"""
    src, out = os.path.join(str(directory), name + ".bin"), os.path.join(str(directory), name + ".frames")
    write_coded(src, coded)
    subprocess.check_call([exe, "--tier1", src, out])
    return jf.read_frames(out)


def to_binding(pkg, cd):
    return pkg.J2kCoded(cd["width"], cd["height"], cd["x0"], cd["y0"], cd["ncomp"], cd["prec"], cd["transform"], cd["mct"], cd["chan"], cd["tcs"], cd["steps"],
                        cd["ncoeffs"], cd["cblks"], cd["bytes"])


def segment(rs, kind, w, h, passes):
    """the bytes of a block whose decoding reads w * h * passes samples or so"""
    work = w * h * passes
    if kind == "empty":
        return b""
    if kind == "one":
        return bytes(rs.randint(0, 256, 1).astype(np.uint8))
    if kind == "short":  # two bytes: fewer than any block of more than a few samples consumes
        return bytes(rs.randint(0, 256, 2).astype(np.uint8))
    if kind == "ample":  # four bits a sample and pass: random bytes cost the decoder about one
        return bytes(rs.randint(0, 256, work // 2 + 64).astype(np.uint8))
    if kind == "zeros":
        return bytes(64)
    if kind == "ff":
        return b"\xff" * 64
    n = max(4, work // 16)
    b = bytearray(rs.randint(0, 256, n).astype(np.uint8).tobytes())
    if kind == "marker":  # ff 90 in the middle: the branch of bytein that does not consume
        b[n // 2], b[n // 2 + 1] = 0xff, 0x90
    else:
        assert kind == "ends_ff"
        b[-1] = 0xff
    return bytes(b)


def random_blocks(rs, plane_w=1100, ncomp=3, rounds=1):
    """One coded descriptor - an image of one tile, `ncomp` components, no decomposition level - whose planes hold every
    (size, segment kind, orientation) of SIZES x SEGMENTS x 0 .. 3, `rounds` times, laid out in shelves with gaps between the
    blocks and a margin around them.  numbps and passes go round so that every pair of them occurs with every size; passes is
    what the descriptor rule allows at most (min(passes, 3 * numbps - 2)).  Returns (descriptor, the cases in block order)."""
    cases, k = [], 0
    for _ in range(rounds):
        for si, (w, h) in enumerate(SIZES):
            for gi, seg in enumerate(SEGMENTS):
                for orient in range(4):
                    nb = NUMBPS[(k + k // 4) % 4]
                    pa = PASSES[(k // 4 + gi + si) % 5]
                    passes = min(pa, 3 * nb - 2) if pa else 3 * nb - 2
                    cases.append(dict(w=w, h=h, seg=seg, orient=orient, numbps=nb, passes=passes))
                    k += 1
    # shelves per component: tallest first, 3 samples between blocks, a margin of 2
    order = sorted(range(len(cases)), key=lambda i: (-cases[i]["h"], i))
    cur = [dict(x=2, y=2, shelf=0) for _ in range(ncomp)]
    for n, i in enumerate(order):
        c, comp = cases[i], n % ncomp
        p = cur[comp]
        if p["x"] + c["w"] + 2 > plane_w:
            p["x"], p["y"], p["shelf"] = 2, p["y"] + p["shelf"] + 3, 0
        c["tc"], c["x"], c["y"] = comp, p["x"], p["y"]
        p["x"] += c["w"] + 3
        p["shelf"] = max(p["shelf"], c["h"])
    plane_h = max(p["y"] + p["shelf"] for p in cur) + 2
    cblks, pool = np.zeros(len(cases), CBLK), bytearray(rs.randint(0, 256, 7).astype(np.uint8).tobytes())
    for i, c in enumerate(cases):
        data = segment(rs, c["seg"], c["w"], c["h"], c["passes"])
        cblks[i] = (c["tc"], c["y"] * plane_w + c["x"], len(pool), len(data), c["w"], c["h"], c["orient"], c["numbps"], c["passes"], 0, 0)
        pool += data
    n = plane_w * plane_h
    tcs = np.array([(0, 0, plane_w, plane_h, 0, c, c, 0, c * n) for c in range(ncomp)], jf.TC)
    cd = dict(width=plane_w, height=plane_h, x0=0, y0=0, ncomp=ncomp, prec=8, transform=0, mct=0, chan=[0, 1, 2] if ncomp == 3 else [0, 0, 0], tcs=tcs,
              steps=np.ones(ncomp, np.float32), ncoeffs=ncomp * n, cblks=cblks, bytes=np.frombuffer(bytes(pool), np.uint8))
    return cd, cases


def small_coded(rs):
    """a sound descriptor of two tiles, 3 components, 2 levels: a few random blocks in each tile-component"""
    fr = jf.random_frame(rs, 40, 21, 2, 1, 1, x0=1, y0=0, tiling=(32, 32, 0, 0))
    cblks, pool = [], bytearray()
    for t, tc in enumerate(fr["tcs"]):
        W, H = int(tc["x1"] - tc["x0"]), int(tc["y1"] - tc["y0"])
        for (x, y, w, h) in ((0, 0, min(W, 5), min(H, 4)), (W - 3, H - 6, 3, 6), (1, 7, 4, 5)):
            data = bytes(rs.randint(0, 256, 40).astype(np.uint8))
            cblks.append((t, y * W + x, len(pool), len(data), w, h, (t + x) % 4, 5, 9, 0, 0))
            pool += data
    cd = {k: v for k, v in fr.items() if k != "coeffs"}
    cd.update(ncoeffs=len(fr["coeffs"]), cblks=np.array(cblks, CBLK), bytes=np.frombuffer(bytes(pool), np.uint8))
    return cd
