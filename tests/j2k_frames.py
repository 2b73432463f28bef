"""JPEG 2000 frame descriptors for the tests: the file form host/j2k_check reads and writes (--frame, --pixels) and random sound
descriptors (what j2k::parse could hand over: any size, origin, tiling, level count, transform, coefficients up to what the
guard bits allow), which need no entropy coding."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cpp-paddle-ocr_amd", "host")
TC = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("levels", "<i4"), ("comp", "<i4"), ("step_off", "<u4"), ("reserved", "<u4"),
               ("coeff_off", "<u8")])
HEAD = ("width", "height", "x0", "y0", "ncomp", "prec", "transform", "mct", "chan0", "chan1", "chan2", "device_ok", "progression", "layers", "tiles_x",
        "tiles_y", "file_comps", "jp2", "qstyle", "cbw", "cbh", "precincts", "tileparts", "sop_eph")
WIDTHS = [1, 2, 3, 5, 17, 33, 65, 129, 257]
HEIGHTS = [1, 2, 3, 17, 65, 130]


def build_check(directory, *flags):
    exe = os.path.join(str(directory), "j2k_check" + ("_san" if flags else ""))
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", *flags, "-o", exe, os.path.join(HOST, "j2k_check.cpp")])
    return exe


def write_frames(path, frames):
    with open(path, "wb") as f:
        for fr in frames:
            head = [fr.get(k, 0) for k in HEAD]
            head[8:11] = list(fr["chan"])
            tcs = np.ascontiguousarray(fr["tcs"], TC)
            steps = np.ascontiguousarray(fr["steps"], "<f4")
            coeffs = np.ascontiguousarray(fr["coeffs"], "<i4")
            f.write(struct.pack("<24i", *head) + struct.pack("<Q", len(tcs)) + tcs.tobytes() + struct.pack("<Q", len(steps)) + steps.tobytes() +
                    struct.pack("<Q", len(coeffs)) + coeffs.tobytes())


def read_frames(path):
    blob, out, at = open(path, "rb").read(), [], 0
    while at < len(blob):
        fr = dict(zip(HEAD, struct.unpack_from("<24i", blob, at)))
        fr["chan"] = [fr.pop("chan0"), fr.pop("chan1"), fr.pop("chan2")]
        at += 96
        for key, dt, size in (("tcs", TC, 40), ("steps", "<f4", 4), ("coeffs", "<i4", 4)):
            n, = struct.unpack_from("<Q", blob, at)
            fr[key] = np.frombuffer(blob, dt, n, at + 8).copy()
            at += 8 + size * n
        out.append(fr)
    return out


def host_pixels(exe, directory, frames):
    """j2k::pixels over descriptors (j2k_check --pixels): the BGR images"""
    src, out = os.path.join(str(directory), "frames.bin"), os.path.join(str(directory), "pixels.bin")
    write_frames(src, frames)
    subprocess.check_call([exe, "--pixels", src, out])
    flat, res, pos = np.fromfile(out, np.uint8), [], 0
    for fr in frames:
        n = 3 * fr["width"] * fr["height"]
        res.append(flat[pos:pos + n].reshape(fr["height"], fr["width"], 3))
        pos += n
    assert pos == len(flat)
    return res


def random_frame(rs, width, height, levels, transform, mct, x0=0, y0=0, tiling=None, prec=8, ncomp=3, dense=True):
    """tiling: None (one tile) or (tile width, tile height, tile x origin <= x0, tile y origin <= y0).  Coefficients: integers with
    their half bit up to 2^(prec + 3) (two guard bits on top of the band gain of HH), steps between 2^-3 and 2."""
    if mct:
        ncomp = 3
    if tiling:
        tw, th, tx0, ty0 = tiling
        xs = sorted({x0, x0 + width} | {x for x in range(tx0, x0 + width, tw) if x > x0})
        ys = sorted({y0, y0 + height} | {y for y in range(ty0, y0 + height, th) if y > y0})
    else:
        xs, ys = [x0, x0 + width], [y0, y0 + height]
    tcs, steps, coeffs, at = [], [], [], 0
    top = 1 << (prec + 3)
    for ty in range(len(ys) - 1):
        for tx in range(len(xs) - 1):
            n = (xs[tx + 1] - xs[tx]) * (ys[ty + 1] - ys[ty])
            for c in range(ncomp):
                tcs.append((xs[tx], ys[ty], xs[tx + 1], ys[ty + 1], levels, c, len(steps), 0, at))
                steps += list(2.0 ** rs.uniform(-3, 1, 1 + 3 * levels))
                v = rs.randint(-top, top + 1, n)
                if not dense:
                    v[rs.rand(n) < 0.7] = 0
                coeffs.append(v)
                at += n
    chan = [0, 0, 0] if ncomp == 1 else [int(k) for k in rs.permutation(3)] if not mct else [0, 1, 2]
    return dict(width=width, height=height, x0=x0, y0=y0, ncomp=ncomp, prec=prec, transform=transform, mct=mct, chan=chan,
                tcs=np.array(tcs, TC), steps=np.array(steps, np.float32), coeffs=np.concatenate(coeffs).astype(np.int32))


def to_binding(pkg, fr):
    return pkg.J2kFrame(fr["width"], fr["height"], fr["x0"], fr["y0"], fr["ncomp"], fr["prec"], fr["transform"], fr["mct"], fr["chan"], fr["tcs"], fr["steps"],
                        fr["coeffs"])
