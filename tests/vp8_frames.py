"""VP8 frame descriptors for the tests: the file form host/vp8_check reads and writes (--frame, --pixels) and random sound
descriptors (what vp8::parse could hand over: any modes, any coefficients, any filter parameters), which need no bit stream."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cpp-paddle-ocr_amd", "host")
MB = np.dtype([("modes", "u1", 16), ("is_i4x4", "u1"), ("uvmode", "u1"), ("level", "u1"), ("ilevel", "u1"), ("hev", "u1"), ("inner", "u1"),
               ("segment", "u1"), ("skip", "u1"), ("nz_y", "<u4"), ("nz_uv", "<u4"), ("present", "<u4"), ("coeff_off", "<u4")])
WIDTHS = [1, 2, 15, 16, 17, 31, 33, 65, 257]
HEIGHTS = [1, 2, 15, 16, 17, 33, 49]


def build_check(directory, *flags):
    exe = os.path.join(str(directory), "vp8_check" + ("_san" if flags else ""))
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", *flags, "-o", exe, os.path.join(HOST, "vp8_check.cpp")])
    return exe


def write_frames(path, frames):
    with open(path, "wb") as f:
        for fr in frames:
            f.write(struct.pack("<5i", fr["width"], fr["height"], fr["filter_type"], fr.get("partitions", 1), fr.get("segments", 1)))
            mbs = np.ascontiguousarray(fr["mbs"], MB)
            coeffs = np.ascontiguousarray(fr["coeffs"], "<i2")
            f.write(struct.pack("<Q", len(mbs)) + mbs.tobytes() + struct.pack("<Q", len(coeffs)) + coeffs.tobytes())


def read_frames(path):
    blob, out, at = open(path, "rb").read(), [], 0
    while at < len(blob):
        w, h, ft, parts, segs = struct.unpack_from("<5i", blob, at)
        n, = struct.unpack_from("<Q", blob, at + 20)
        mbs = np.frombuffer(blob, MB, n, at + 28).copy()
        at += 28 + 40 * n
        m, = struct.unpack_from("<Q", blob, at)
        coeffs = np.frombuffer(blob, "<i2", m, at + 8).copy()
        at += 8 + 2 * m
        out.append(dict(width=w, height=h, filter_type=ft, partitions=parts, segments=segs, mbs=mbs, coeffs=coeffs))
    return out


def host_pixels(exe, directory, frames):
    """vp8::pixels over descriptors (vp8_check --pixels): the BGR images"""
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


def filter_params(level, sharpness):
    """interior limit and hev threshold of a level, as the key-frame header's sharpness makes them"""
    ilevel = level
    if sharpness > 0:
        ilevel >>= 2 if sharpness > 4 else 1
        ilevel = min(ilevel, 9 - sharpness)
    return max(ilevel, 1), 2 if level >= 40 else 1 if level >= 15 else 0


def random_frame(rs, width, height, pred="mix", filt="none", coef="dense"):
    """pred: "i16_<0..3>" (chroma mode the same), "b_<0..9>", "mix"; filt: "none", "simple", "normal1", "normal63", "sharp7",
    "deltas" (a level of its own per macroblock, 0 included); coef: "skipped", "dc", "dense", "extreme" (any int16)"""
    n = ((width + 15) >> 4) * ((height + 15) >> 4)
    mbs = np.zeros(n, MB)
    blocks = []
    for i in range(n):
        m = mbs[i]
        if pred.startswith("i16_"):
            m["is_i4x4"], m["modes"][0], m["uvmode"] = 0, int(pred[4:]), int(pred[4:])
        elif pred.startswith("b_"):
            m["is_i4x4"], m["modes"], m["uvmode"] = 1, int(pred[2:]), rs.randint(4)
        else:
            m["is_i4x4"], m["uvmode"] = rs.randint(2), rs.randint(4)
            m["modes"] = rs.randint(10, size=16) if m["is_i4x4"] else rs.randint(4)
        if filt != "none":
            level = {"simple": 20, "normal1": 1, "normal63": 63, "sharp7": 40}.get(filt)
            if level is None:
                level = int(rs.choice([0, 1, 9, 15, 33, 40, 63]))
            sharpness = 7 if filt == "sharp7" else int(rs.choice([0, 3])) if filt == "deltas" else 0
            m["level"] = level
            if level:
                m["ilevel"], m["hev"] = filter_params(level, sharpness)
            m["inner"] = 1 if m["is_i4x4"] else rs.randint(2)
        m["coeff_off"] = len(blocks)
        if coef == "skipped":
            continue
        present = 0
        for b in range(25 if not m["is_i4x4"] else 24):
            if rs.rand() < (0.3 if coef != "dc" else 0.6):
                continue
            blk = np.zeros(16, np.int64)
            if coef == "dc":
                blk[0] = rs.randint(-900, 901) or 5
            elif coef == "dense":
                k = rs.randint(1, 17)
                blk[:k] = rs.randint(-300, 301, k)
            else:
                blk[:] = rs.choice([-32768, 32767, 0, 1, -1, 16384, -16384] + rs.randint(-32768, 32768, 4).tolist(), 16)
            if not blk.any():
                blk[0] = 1
            present |= 1 << b
            blocks.append(blk)
        m["present"] = present
        if coef != "dc":  # any class per block: 0, 2 or 3
            m["nz_y"] = int(sum(int(rs.choice([0, 2, 3])) << (2 * k) for k in range(16)))
            m["nz_uv"] = int(sum(int(rs.choice([0, 0, 2, 3])) << (2 * k) for k in range(8)))
    coeffs = np.array(blocks, np.int16).reshape(-1) if blocks else np.zeros(0, np.int16)
    return dict(width=width, height=height, filter_type={"none": 0, "simple": 1}.get(filt, 2), mbs=mbs, coeffs=coeffs)
