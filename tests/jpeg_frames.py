"""JPEG frame descriptors for the tests: the file form host/jpeg_check reads and writes (--frame, --pixels), random sound
descriptors (what Decoder::decode_coefficients could hand over: any size, sampling, colour space, orientation, quantisation
table and coefficients inside the domain of tools/jpeg_ref.py), which need no Huffman coding, and CASES, the table that
tests/test_jpeg_ref.py (host == reference, mutations) and tests/test_gpu_jpeg_ops.py (device == reference) share."""
import os
import struct
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cpp-paddle-ocr_amd", "host")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import jpeg_ref as ref  # noqa: E402
import jpeg_writer as jw  # noqa: E402

SIZES = [1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 63, 64, 65, 129]
COLORS = {"grey": 0, "ycbcr": 1, "rgb": 2, "cmyk": 3, "ycck": 4}
FORMS = ["zero", "dc", "single", "dense", "extreme"]
# (h, v) per component; a fourth component takes luma's factors where the colour space has one
SAMPLINGS = {
    "1x1": [(1, 1), (1, 1), (1, 1)],
    "2x1": [(2, 1), (1, 1), (1, 1)],
    "2x2": [(2, 2), (1, 1), (1, 1)],
    "1x2": [(1, 2), (1, 1), (1, 1)],
    "4x1": [(4, 1), (1, 1), (1, 1)],
    "1x4": [(1, 4), (1, 1), (1, 1)],
    "4x2": [(4, 2), (1, 1), (1, 1)],
    "3x1": [(3, 1), (1, 1), (1, 1)],
    "4x4": [(4, 4), (1, 1), (1, 1)],
    "subsampled luma": [(1, 1), (2, 2), (2, 2)],
    "four components": [(2, 2), (1, 1), (1, 1), (2, 2)],   # the sampling of the YCCK files of tests/test_jpeg_formats.py
}
HEAD = ("rows", "cols", "ncomp", "orientation", "color", "reserved")
COMP = ("h", "v", "bw", "bh", "dw", "dh")


def build_check(directory, *flags):
    exe = os.path.join(str(directory), "jpeg_check" + ("_san" if flags else ""))
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", *flags, "-o", exe, os.path.join(HOST, "jpeg_check.cpp")])
    return exe


def write_frames(path, frames):
    with open(path, "wb") as f:
        for fr in frames:
            f.write(struct.pack("<6i", fr["rows"], fr["cols"], len(fr["comps"]), fr["orientation"], fr["color"], fr.get("reserved", 0)))
            for c in fr["comps"]:
                coef = np.ascontiguousarray(c["coef"], "<i2").reshape(-1)
                f.write(struct.pack("<6i", *[c[k] for k in COMP]) + np.ascontiguousarray(c["quant"], "<u2").tobytes() + struct.pack("<Q", len(coef)) +
                        coef.tobytes())


def read_frames(path):
    blob, out, at = open(path, "rb").read(), [], 0
    while at < len(blob):
        fr = dict(zip(HEAD, struct.unpack_from("<6i", blob, at)))
        at += 24
        fr["comps"] = []
        for _ in range(fr.pop("ncomp")):
            c = dict(zip(COMP, struct.unpack_from("<6i", blob, at)))
            c["quant"] = np.frombuffer(blob, "<u2", 64, at + 24).copy()
            n, = struct.unpack_from("<Q", blob, at + 152)
            c["coef"] = np.frombuffer(blob, "<i2", n, at + 160).copy()
            at += 160 + 2 * n
            fr["comps"].append(c)
        out.append(fr)
    return out


def out_shape(fr):
    return (fr["cols"], fr["rows"], 3) if fr["orientation"] >= 5 else (fr["rows"], fr["cols"], 3)


def host_pixels(exe, directory, frames):
    """Decoder::pixels over descriptors (jpeg_check --pixels): the oriented BGR images"""
    src, out = os.path.join(str(directory), "frames.bin"), os.path.join(str(directory), "pixels.bin")
    write_frames(src, frames)
    subprocess.check_call([exe, "--pixels", src, out])
    flat, res, pos = np.fromfile(out, np.uint8), [], 0
    for fr in frames:
        shape = out_shape(fr)
        n = shape[0] * shape[1] * 3
        res.append(flat[pos:pos + n].reshape(shape))
        pos += n
    assert pos == len(flat)
    return res


def geometry(rows, cols, sampling, color):
    """the components of a frame without tables and coefficients: block counts from whole MCUs, as a file has them"""
    ncomp = {0: 1, 1: 3, 2: 3, 3: 4, 4: 4}[color]
    factors = [(1, 1)] if ncomp == 1 else list(sampling[:ncomp]) + [sampling[0]] * (ncomp - len(sampling))
    hmax, vmax = max(h for h, _ in factors), max(v for _, v in factors)
    mcux, mcuy = -(-cols // (8 * hmax)), -(-rows // (8 * vmax))
    return [dict(h=h, v=v, bw=mcux * h, bh=mcuy * v, dw=-(-cols * h // hmax), dh=-(-rows * v // vmax)) for h, v in factors]


# the positions a "single" frame goes through first: the first AC in each direction, the corners of the last row and column
SINGLE_FIRST = [1, 8, 63, 7, 56, 9, 62, 55]


def random_frame(rs, rows, cols, sampling, color, orient, coef):
    """sampling: a key of SAMPLINGS or a list of (h, v); color: a key of COLORS; coef: one of FORMS -
    zero; dc (any table, flat blocks from far below 0 to far above 255); single (one AC per block: positions 1, 8, 63, 7, 56
    ... first, then random ones); dense (the quality-50 table, amplitudes falling with frequency as in a file of that quality);
    extreme (per component, in turn, a table of 255s under coefficients from the whole int16 range, and a table of 1s under -1, 0, 1).
    Every frame is inside the domain of the reference (tools/jpeg_ref.py, DEQUANT_BOUND)."""
    comps = geometry(rows, cols, SAMPLINGS[sampling] if isinstance(sampling, str) else sampling, COLORS[color])
    q50 = jw.quant_table(50)
    flip = int(rs.randint(2))
    for i, c in enumerate(comps):
        n = c["bw"] * c["bh"]
        blocks = np.zeros((n, 64), np.int64)
        quant = rs.randint(1, 256, 64)
        if coef == "dc":
            quant[0] = rs.choice([1, 2, 8, 16, 255])
            top = 2400 // int(quant[0])   # the flat value 128 + dc * q / 8 runs over about -170 .. 430
            blocks[:, 0] = rs.randint(-top, top + 1, n)
        elif coef == "single":
            quant = q50
            pos = np.array((SINGLE_FIRST + rs.randint(1, 64, n).tolist())[:n]) if n > 1 else rs.choice(SINGLE_FIRST, 1)
            amp = rs.randint(1, 2000, n) // quant[pos] + 1
            blocks[np.arange(n), pos] = amp * rs.choice([-1, 1], n)
        elif coef == "dense":
            quant = q50
            u, v = np.meshgrid(np.arange(8), np.arange(8))
            blocks = np.rint(rs.laplace(0, 1, (n, 64)) * (40.0 / (1 + u + v).reshape(64))).astype(np.int64)
            blocks[:, 0] = rs.randint(-1000 // int(quant[0]), 1000 // int(quant[0]) + 1, n)
        elif coef == "extreme":
            if (i + flip) % 2 == 0:
                quant = np.full(64, 255)
                blocks = rs.choice([-32768, 32767, 0, 1, -1, 16384, -16384] + rs.randint(-32768, 32768, 4).tolist(), (n, 64))
                blocks[rs.rand(n) < 0.25] = 32767    # a block of one sign in every position, and its negative
                blocks[rs.rand(n) < 0.1] = -32768
            else:
                quant = np.ones(64, np.int64)
                blocks = rs.randint(-1, 2, (n, 64))
        else:
            assert coef == "zero", coef
        c["quant"] = np.asarray(quant, np.uint16)
        c["coef"] = blocks.astype(np.int16).reshape(-1)
    fr = dict(rows=rows, cols=cols, color=COLORS[color], orientation=orient, comps=comps)
    assert ref.in_domain(fr), "a frame outside the domain of the reference"
    return fr


def flat_frame(rows, cols, sampling, color, orient, values):
    """every block DC-only: with quant[0] = 8 and dc = v - 128 a block is flat at v (tests/test_jpeg_ref.py checks that identity).
    values: per component a number or an array (bh, bw) of sample values 0..255"""
    comps = geometry(rows, cols, SAMPLINGS[sampling] if isinstance(sampling, str) else sampling, COLORS[color])
    for c, v in zip(comps, values):
        blocks = np.zeros((c["bh"] * c["bw"], 64), np.int16)
        blocks[:, 0] = (np.broadcast_to(np.asarray(v, np.int64), (c["bh"], c["bw"])) - 128).reshape(-1)
        c["quant"] = np.full(64, 1, np.uint16)
        c["quant"][0] = 8
        c["coef"] = blocks.reshape(-1)
    return dict(rows=rows, cols=cols, color=COLORS[color], orientation=orient, comps=comps)


def to_binding(pkg, fr):
    return pkg.JpegFrame(fr["rows"], fr["cols"], fr["color"], fr["orientation"], fr["comps"])


# ------------------------------------------------------------------------------------------------------------- CASES
def _case(group, name, rows, cols, sampling, color, orient, coef, seed, branches=()):
    return dict(group=group, name=name, rows=rows, cols=cols, sampling=sampling, color=color, orient=orient, coef=coef, seed=seed, branches=tuple(branches))


def _cases():
    out = []
    # the numbered branches of the per-pixel upsampling rules, each case named for what it is there for (jpeg_ref.BRANCHES)
    targeted = [
        # rows, cols, sampling, color, branches: chroma of 2x1 / 2x2 has dw = ceil(cols / 2), dh = ceil(rows / 2)
        (9, 1, "2x1", "ycbcr", ["box.narrow_dw1", "copy"]),
        (9, 2, "2x1", "ycbcr", ["box.narrow_dw1"]),
        (9, 3, "2x1", "ycbcr", ["box.narrow_dw2"]),
        (9, 4, "2x1", "ycbcr", ["box.narrow_dw2"]),
        (9, 5, "2x1", "ycbcr", ["h2v1.dw3", "h2v1.first", "h2v1.even", "h2v1.odd", "h2v1.ends_even"]),
        (9, 6, "2x1", "ycbcr", ["h2v1.dw3", "h2v1.last"]),
        (5, 2, "2x2", "ycbcr", ["box.narrow_dw1"]),
        (5, 4, "2x2", "ycbcr", ["box.narrow_dw2"]),
        (1, 5, "2x2", "ycbcr", ["h2v2.dw3", "h2v2.dh1", "h2v2.top_clamped", "h2v2.first", "h2v2.even", "h2v2.odd", "h2v2.ends_even"]),
        (2, 6, "2x2", "ycbcr", ["h2v2.dw3", "h2v2.dh1", "h2v2.top_clamped", "h2v2.bottom_clamped", "h2v2.last"]),
        (3, 7, "2x2", "ycbcr", ["h2v2.dh2", "h2v2.top_clamped", "h2v2.ends_even"]),
        (4, 8, "2x2", "ycbcr", ["h2v2.dh2", "h2v2.bottom_clamped", "h2v2.last"]),
        (18, 22, "2x2", "ycbcr", ["h2v2.bottom_clamped", "h2v2.last"]),       # even sizes off the block grid: the padding is next to the edge
        (1, 3, "1x2", "ycbcr", ["h1v2.dh1", "h1v2.top_clamped", "h1v2.upper"]),
        (2, 3, "1x2", "rgb", ["h1v2.dh1", "h1v2.bottom_clamped", "h1v2.lower"]),
        (7, 9, "1x2", "ycbcr", ["h1v2.upper", "h1v2.lower", "h1v2.top_clamped"]),
        (6, 9, "1x2", "ycbcr", ["h1v2.bottom_clamped"]),
        (5, 9, "4x1", "ycbcr", ["box.other"]),
        (9, 5, "1x4", "rgb", ["box.other"]),
        (9, 9, "4x2", "ycbcr", ["box.other"]),
        (7, 7, "3x1", "ycbcr", ["box.other"]),
        (9, 9, "4x4", "ycbcr", ["box.other"]),
        (6, 10, "subsampled luma", "ycbcr", ["h2v2.last", "h2v2.bottom_clamped", "copy"]),
        (9, 6, "subsampled luma", "rgb", ["h2v2.dw3"]),
        (9, 12, "four components", "ycck", ["h2v2.last", "copy"]),
        (10, 11, "four components", "cmyk", ["h2v2.bottom_clamped"]),
        (9, 4, "four components", "cmyk", ["box.narrow_dw2"]),
        (17, 15, "1x1", "grey", ["copy"]),
    ]
    for k, (rows, cols, sampling, color, branches) in enumerate(targeted):
        for form in ("dense", "extreme"):
            out.append(_case("branch", "%s %s %dx%d %s" % (sampling, color, rows, cols, form), rows, cols, sampling, color, 1 + (k % 8 if form == "extreme" else 0), form,
                             1000 + k, branches))
    # every size as rows and as cols with every sampling, colour, orientation and form going round
    k = 0
    for si, (sampling, factors) in enumerate(SAMPLINGS.items()):
        for i, rows in enumerate(SIZES):
            cols = SIZES[(5 * i + si) % len(SIZES)]
            color = ("ycck", "cmyk")[i % 2] if len(factors) == 4 else ("grey", "ycbcr", "rgb", "ycbcr")[k % 4] if sampling == "1x1" else ("ycbcr", "ycbcr", "rgb")[k % 3]
            out.append(_case("grid", "grid %s %s %dx%d" % (sampling, color, rows, cols), rows, cols, sampling, color, 1 + k % 8, FORMS[(k // 8 + k) % 5], 2000 + k))
            k += 1
    # the transposing orientations around the edges of the 64 x 64 LDS tile, through the classic kernels (2x2, 1x1 grey) and the general ones
    edge = [63, 64, 65, 128, 129]
    for i, rows in enumerate(edge):
        for orient in (5, 6, 7, 8):
            cols = edge[(i + orient + 1) % 5]
            for sampling, color in (("2x2", "ycbcr"), ("1x1", "grey"), ("1x2", "ycbcr"), ("four components", "cmyk"))[(i + orient) % 2::2]:
                out.append(_case("tiles", "tiles %s %s %dx%d tag %d" % (sampling, color, rows, cols, orient), rows, cols, sampling, color, orient, "dense",
                                 3000 + 10 * i + orient))
    # planes of 1, 31, 32, 33 and 65 blocks in one column of blocks (bw == 1): the IDCT kernel's 32 blocks per workgroup
    for n in (1, 31, 32, 33, 65):
        for color in ("grey", "ycbcr"):
            out.append(_case("layout", "layout %d blocks %s" % (n, color), 8 * n - 3, 5, "1x1", color, 1, "dense", 4000 + n))
    return out


CASES = _cases()
# the case on which each mutation of the reference shows (tests/test_jpeg_ref.py asserts it, tests/test_gpu_jpeg_ops.py
# compares the mutated reference with the device's bytes there)
WITNESS = {
    "h2v2_bias_swapped": "2x2 ycbcr 1x5 extreme",
    "h1v2_bias_swapped": "1x2 ycbcr 7x9 dense",
    "h2v1_edge_fancy": "2x1 ycbcr 9x6 dense",
    "narrow_fancy": "2x1 ycbcr 9x3 dense",
    "lower_clamp_off_by_one": "2x2 ycbcr 2x6 dense",
    "box_y_uses_hexp": "4x2 ycbcr 9x9 dense",
    "pass1_no_round": "1x1 grey 17x15 dense",
    "pass2_no_round": "1x1 grey 17x15 dense",
    "idct_wrap": "1x1 grey 17x15 extreme",
    "orient_5_7_swapped": "tiles 1x1 grey 63x64 tag 5",
    "orient_6_8_swapped": "tiles 2x2 ycbcr 63x65 tag 6",
    "cmyk_div255": "four components cmyk 10x11 dense",
    "green_constants_swapped": "grid 1x1 ycbcr 2x6",
    "plane_search": "layout 33 blocks ycbcr",
}


def colour_table_frame(kind):
    """2048 x 2048, every component 1x1, every block flat: block (by, bx) carries the pair (bx, by) in the two components a
    colour function takes its table index from.  "ycbcr a" / "ycbcr b": Cb = bx, Cr = by, Y = bx ^ by and its complement - Y runs
    over 0..255 in every row of blocks and the two images together hold all eight corners of (Y, Cb, Cr); "cmyk": C = bx, K = by
    (M, Y: other walks through 0..255); "ycck": Cb = bx, Cr = by, Y = bx ^ by, K = (bx + 3 * by) mod 256"""
    by, bx = np.mgrid[0:256, 0:256]
    if kind.startswith("ycbcr"):
        y = bx ^ by
        return flat_frame(2048, 2048, "1x1", "ycbcr", 1, [y if kind.endswith("a") else 255 - y, bx, by])
    if kind == "cmyk":
        return flat_frame(2048, 2048, "1x1", "cmyk", 1, [bx, 255 - bx, (bx * 7 + by) & 255, by])
    assert kind == "ycck", kind
    return flat_frame(2048, 2048, "1x1", "ycck", 1, [bx ^ by, bx, by, (bx + 3 * by) & 255])


def frame_of(case):
    return random_frame(np.random.RandomState(case["seed"]), case["rows"], case["cols"], case["sampling"], case["color"], case["orient"], case["coef"])


def case_named(name):
    return next(c for c in CASES if c["name"] == name)
