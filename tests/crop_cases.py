"""The cases of the crop geometry between detector and recognizer (warp_crop_kernel, rotate180_groups_kernel of
csrc/kernels_pre.hip, plan_rotate_crop of csrc/crop.h, the grouping of csrc/rot_groups.h), shared by tests/test_crop_ref.py
(crop_ref == oracle wherever the oracle can express a case, CPU) and tests/test_gpu_crop_ops.py (device == crop_ref, byte for
byte).  The shapes are the smallest at which each branch exists; the largest buffer is 1027 x 35 pixels."""
import numpy as np

from pre_cases import image

TAIL = 16      # bytes behind the last source crop: a read past the end stays inside the buffer
OUT_TAIL = 64  # bytes of the output behind the last crop, in front of the library's own guard
GAP = 5        # bytes between two source crops of one launch


# ---------------------------------------------------------------------------------------- warp launches, given matrices
def block_width(dw, dh):
    return min(1024 // min(16, dh), dw)


def _crop(kind, sw, sh, dw, dh, m, rot=0, bw0=None, off=0, stride_extra=0, seed=0):
    return dict(kind=kind, sw=sw, sh=sh, dw=dw, dh=dh, m=[float(v) for v in m], rot=rot, bw0=block_width(dw, dh) if bw0 is None else bw0,
                off=off, stride_extra=stride_extra, seed=seed)


def _affine(tx=0.0, ty=0.0):
    return [1, 0, tx, 0, 1, ty, 0, 0, 1]


def _w_of(m, x, y, bw0):
    """the W of destination pixel (x, y) with the block base at a multiple of bw0 (bw0 = 1: evaluated at the pixel itself)"""
    xb = (x // bw0) * bw0
    return (m[6] * xb + m[7] * y + m[8]) + m[6] * (x - xb)


def seam_matrix(dw, dh, other_bw0):
    """A perspective matrix whose W at one pixel (xt, yt) is EXACTLY 0 under one of the two rules - blocks of the true width, blocks
    of `other_bw0` columns (1: the direct evaluation) - and a rounding residue (1e-17 or so) under the other: the exact rule reads
    source pixel (0, 0) there, the other one saturates (the pixel is 0).  Away from that pixel the warp reads near source point
    (3 + 0.02 / W, 1 + 0.004 / W), inside a 7 x 3 source for most pixels.  -> (m, (xt, yt), the block width whose W is 0)"""
    bw0 = block_width(dw, dh)
    m6, m7 = 2.0 ** -8 / 3, 2.0 ** -4 / 7
    for exact, residue in ((other_bw0, bw0), (bw0, other_bw0)):
        for yt in range(dh - 1, -1, -1):
            for xt in range(dw - 1, 0, -1):
                xb = (xt // exact) * exact
                m8 = -((m6 * xb + m7 * yt) + m6 * (xt - xb))
                m = [3 * m6, 3 * m7, 3 * m8 + 0.02, m6, m7, m8 + 0.004, m6, m7, m8]
                if _w_of(m, xt, yt, exact) == 0.0 and _w_of(m, xt, yt, residue) != 0.0:
                    return m, (xt, yt), exact
    return None, None, None


def _launch(name, *crops, max_pixels=None):
    return dict(name=name, crops=list(crops), max_pixels=max(c["dw"] * c["dh"] for c in crops) if max_pixels is None else max_pixels)


SEAMS = ((63, 16), (64, 16), (65, 16), (129, 16), (342, 3), (1025, 1))
# dh = 1: y = 0, so "block base + offset" IS the direct evaluation ((0 + m2) + m0 x against (m0 x + 0) + m2, and x1 = 0 in the
# second block): no matrix can tell the two apart at 1025 x 1.  What that size can tell apart is the block WIDTH: 1024 against
# the 64 columns every other test runs with.
SEAM_OTHER = {(1025, 1): 64}


def _warp_launches():
    L = []
    for sw, sh in ((5, 4), (7, 3)):
        t = "_%dx%d" % (sw, sh)
        for kind in ("rand", "ramp", "check1"):
            L.append(_launch("identity" + t + "_" + kind, _crop(kind, sw, sh, sw, sh, _affine())))
        for k in (1, 16, 31):
            L.append(_launch("trans_%d_32%s" % (k, t), _crop("rand", sw, sh, sw, sh, _affine(k / 32, k / 32))))
            L.append(_launch("trans_%d_32%s_check1" % (k, t), _crop("check1", sw, sh, sw, sh, _affine(k / 32, 0))))
        # sx (sy) of destination column (row) 0 at -2, -1, sw - 1, sw, with a fraction that gives every tap a weight
        for tag, v in (("m2", -2), ("m1", -1), ("swm1", sw - 1), ("sw", sw)):
            L.append(_launch("shift_x_%s%s" % (tag, t), _crop("rand", sw, sh, sw, sh, _affine(v + 11 / 32, 0))))
        for tag, v in (("m2", -2), ("m1", -1), ("shm1", sh - 1), ("sh", sh)):
            L.append(_launch("shift_y_%s%s" % (tag, t), _crop("rand", sw, sh, sw, sh, _affine(0, v + 21 / 32))))
        L.append(_launch("shift_x_m1_int" + t, _crop("rand", sw, sh, sw, sh, _affine(-1, 0))))          # fx = 0: the tap at -1 has weight 0
        L.append(_launch("shift_xy_last_int" + t, _crop("ramp", sw, sh, sw, sh, _affine(sw - 1, sh - 1))))
        L.append(_launch("w_zero" + t, _crop("rand", sw, sh, sw, sh, [1, 0, 0, 0, 1, 0, 1, 0, -3])))   # W == 0 at x = 3: source pixel (0, 0)
        L.append(_launch("sat_pos" + t, _crop("rand", sw, sh, sw, sh, [1, 0, 1, 0, 1, 1, 0, 0, 2.0 ** -40])))     # both coordinates > INT_MAX
        L.append(_launch("sat_neg" + t, _crop("rand", sw, sh, sw, sh, [-1, 0, -1, 0, -1, -1, 0, 0, 2.0 ** -40])))  # both < INT_MIN
        L.append(_launch("sat_mixed" + t, _crop("rand", sw, sh, sw, sh, [1, 0, 1, 0, -1, -1, 0, 0, 2.0 ** -40])))
        L.append(_launch("nan" + t, _crop("rand", sw, sh, sw, sh, [1, 0, 0, 0, 1, 0, 0, 0, 5e-324])))    # 32 / W = inf, X0 = 0 at x = 0: 0 * inf
        L.append(_launch("neg_frac" + t, _crop("rand", sw, sh, sw, sh, _affine(-11 / 32, -5 / 32))))    # X = -11: -11 >> 5 = -1, -11 & 31 = 21
        L.append(_launch("tie_1_64" + t, _crop("check1", sw, sh, sw, sh, _affine(1 / 64, 1 / 64))))     # fX = 32 x + 0.5: to the even 32 x
        L.append(_launch("tie_3_64" + t, _crop("check1", sw, sh, sw, sh, _affine(3 / 64, 3 / 64))))     # fX = 32 x + 1.5: to 32 x + 2
        L.append(_launch("tie_m1_64" + t, _crop("check1", sw, sh, sw, sh, _affine(-1 / 64, -3 / 64))))  # -0.5 -> 0, -1.5 -> -2
    for dw, dh in SEAMS:
        m = seam_matrix(dw, dh, SEAM_OTHER.get((dw, dh), 1))[0]
        L.append(_launch("seam_%dx%d" % (dh, dw), _crop("rand", 7, 3, dw, dh, m, seed=3)))
    for dw, dh in ((1, 2), (3, 7), (2, 3)):
        L.append(_launch("turn_%dx%d" % (dw, dh), _crop("rand", 5, 4, dw, dh, [0.9, 0.1, 0.3, -0.1, 0.4, 0.6, 0, 0, 1], rot=1)))
    L.append(_launch("strided_odd_offset", _crop("rand", 5, 4, 6, 5, [0.8, 0.1, -0.4, 0.05, 0.8, -0.3, 0, 0, 1], off=7, stride_extra=4)))
    L.append(_launch("strided_odd_offset_turn", _crop("ramp", 7, 3, 2, 3, _affine(0.5, 0.25), rot=1, off=1, stride_extra=1)))
    # one launch, three descriptors of 1, 300 and 257 pixels: grid.x comes from the largest, the others leave early
    small = _crop("rand", 5, 4, 1, 1, _affine(1.5, 1.25), seed=1)
    big = _crop("rand", 7, 3, 20, 15, [0.3, 0.02, 0.1, 0.01, 0.2, -0.2, 0.001, 0.002, 1], off=3, stride_extra=2, seed=2)
    mid = _crop("check1", 5, 4, 257, 1, [1 / 64, 0, 0.25, 0, 1, 1.5, 0, 0, 1], off=1)
    L.append(_launch("three_crops", small, big, mid))
    L.append(_launch("three_crops_reordered", big, dict(mid, rot=1), small))
    return L


WARP_LAUNCHES = _warp_launches()
WARP_BY_NAME = {c["name"]: c for c in WARP_LAUNCHES}


def crop_source(c):
    return image(c["kind"], c["sh"], c["sw"], seed=c["seed"])


def warp_layout(L):
    """per crop (first byte, stride) of its source in the launch's buffer, the buffer's size, per crop its output offset, and the
    output's size (crops packed back to back, OUT_TAIL bytes behind the last)"""
    src, at = [], 0
    for c in L["crops"]:
        stride = 3 * c["sw"] + c["stride_extra"]
        src.append((at + c["off"], stride))
        at += c["off"] + (c["sh"] - 1) * stride + 3 * c["sw"] + GAP
    out_off = np.cumsum([0] + [c["dw"] * c["dh"] * 3 for c in L["crops"]])
    return src, at - GAP + TAIL, [int(o) for o in out_off[:-1]], int(out_off[-1]) + OUT_TAIL


def warp_buffer(L, outside):
    """the flat source buffer of a launch: every byte that is not a pixel of a source crop is `outside`"""
    src, size, _, _ = warp_layout(L)
    buf = np.full(size, outside, np.uint8)
    for c, (first, stride) in zip(L["crops"], src):
        im = crop_source(c)
        for y in range(c["sh"]):
            buf[first + y * stride:first + y * stride + 3 * c["sw"]] = im[y].reshape(-1)
    return buf


def warp_descs(L):
    src, _, _, _ = warp_layout(L)
    return [dict(c, src_off=first, sstride=stride) for c, (first, stride) in zip(L["crops"], src)]


# well-conditioned FORWARD matrices (source -> destination), which the oracle inverts itself: (name, kind, sw, sh, dw, dh, M)
FORWARD = [
    ("fwd_scale", "rand", 7, 3, 12, 6, [1.7, 0.1, 0.4, -0.05, 1.9, 0.3, 0, 0, 1]),
    ("fwd_persp", "rand", 5, 4, 9, 7, [1.5, 0.2, 1.0, 0.1, 1.4, 0.5, 0.01, 0.02, 1]),
    ("fwd_persp_blocks", "ramp", 7, 3, 130, 16, [17.0, 0.5, 3.0, 0.3, 4.5, 1.0, 0.02, 0.01, 1]),
    ("fwd_shrink", "check1", 7, 3, 3, 2, [0.4, 0.0, 0.2, 0.0, 0.6, 0.1, 0.001, 0, 1]),
]

# ------------------------------------------------------------------------------------ through ocr_rotate_crop / the plan
PLAN_ROWS, PLAN_COLS = 22, 24
PLAN_QUADS = {
    "corner_on_the_edge": [[4, 3], [24, 3], [24, 22], [4, 22]],          # x == cols and y == rows: the box ends at the last pixel
    "corner_on_the_edge_tilted": [[6, 2], [24, 5], [22, 22], [3, 19]],
    "counter_clockwise": [[4, 3], [4, 12], [14, 12], [14, 3]],
    "self_crossing": [[2, 2], [12, 10], [12, 2], [2, 10]],
    "collinear": [[2, 2], [6, 2], [10, 2], [2, 8]],                      # the singular solve: all-zero minv
    "turn_2x3": [[1, 1], [3, 1], [3, 4], [1, 4]],                        # dh == 1.5 dw exactly
    "turn_10x15": [[1, 1], [11, 1], [11, 16], [1, 16]],
    "no_turn_10x14": [[1, 1], [11, 1], [11, 15], [1, 15]],
    "sides_3_4_5": [[6, 2], [9, 6], [5, 9], [2, 5]],                     # sqrt(25) exactly
    "sides_below_an_integer": [[5, 1], [17, 13], [13, 21], [1, 9]],      # sqrt(288) = 16.97 -> 16, sqrt(80) = 8.94 -> 8
    "zero_width": [[5, 5], [5, 5], [9, 12], [5, 12]],                    # cw == 0: the output takes the box's size
}
PLAN_SHAPES = {"turn_2x3": (2, 3, 1), "turn_10x15": (10, 15, 1), "no_turn_10x14": (10, 14, 0), "sides_3_4_5": (5, 5, 0),
               "sides_below_an_integer": (16, 8, 0), "zero_width": (4, 7, 1)}  # (dw, dh, rot)
PLAN_REFUSED = {"empty": [[5, 5], [5, 5], [5, 5], [5, 5]], "left_of_the_image": [[-1, 5], [10, 5], [10, 9], [-1, 9]],
                "below_the_image": [[1, 5], [10, 5], [10, 23], [1, 23]], "zero_height": [[1, 5], [10, 5], [10, 5], [1, 5]]}


def plan_image(kind="rand"):
    return image(kind, PLAN_ROWS, PLAN_COLS, seed=5)


# ------------------------------------------------------------------------------------------- rotation, one ROI per group
ROT_WS, ROT_HS = (1, 2, 3, 63, 64, 65, 511, 512, 513, 1025), (1, 2, 3, 16, 17, 32, 33)


def _rot_pairs():
    odd_h, even_h = [h for h in ROT_HS if h & 1], [h for h in ROT_HS if not h & 1]
    pairs = []
    for i, w in enumerate(ROT_WS):
        pairs += [(w, odd_h[i % len(odd_h)]), (w, even_h[i % len(even_h)])]
    for h in ROT_HS:  # every h meets an odd and an even w
        if not any(p[1] == h and p[0] & 1 for p in pairs):
            pairs.append((3, h))
        if not any(p[1] == h and not p[0] & 1 for p in pairs):
            pairs.append((2, h))
    return pairs


ROT_PAIRS = _rot_pairs()


def _rot(name, w, h, stride_extra=0, view_off=0):
    """one ROI at (1, 1) of a (w + 2) x (h + 2) view: a pixel of margin on every side, every pixel address odd or even by turns"""
    return dict(name=name, cols=w + 2, rows=h + 2, stride_extra=stride_extra, view_off=view_off, rois=[(1, 1, w, h)], seg=[0, 1])


ROT_CASES = [_rot("rot_%dx%d" % (h, w), w, h) for w, h in ROT_PAIRS]
ROT_CASES += [_rot("rot_3x65_stride", 65, 3, stride_extra=7, view_off=5), _rot("rot_2x513_stride", 513, 2, stride_extra=1, view_off=1)]

# groups: rois in LAUNCH order with the caller's seg; `request` = the same ROIs in request order (what the reference applies)
A, B, C_ = (2, 2, 12, 6), (10, 4, 12, 7), (18, 8, 9, 5)     # a chain: A meets B, B meets C, A and C are apart
ROT_GROUPS = [
    dict(name="chain", rois=[A, B, C_], seg=[0, 3]),
    dict(name="same_roi_twice", rois=[A, A], seg=[0, 2]),
    dict(name="same_roi_three_times", rois=[B, B, B], seg=[0, 3]),
    dict(name="nested", rois=[(3, 3, 20, 14), (8, 6, 7, 5), (9, 7, 3, 2)], seg=[0, 3]),
    dict(name="several_groups", rois=[A, B, C_, (30, 1, 7, 7), (31, 2, 5, 3), (2, 16, 5, 3), (30, 12, 1, 9), (24, 18, 3, 1)], seg=[0, 3, 5, 6, 7, 8]),
    dict(name="no_group", rois=[A], seg=[0]),
]
for g in ROT_GROUPS:
    g.update(cols=40, rows=22, stride_extra=2, view_off=0)
ROT_ALL = ROT_CASES + ROT_GROUPS
ROT_BY_NAME = {c["name"]: c for c in ROT_ALL}


def rot_geometry(c):
    """(stride, buffer size)"""
    stride = 3 * c["cols"] + c["stride_extra"]
    return stride, c["view_off"] + c["rows"] * stride + TAIL


def rot_buffer(c):
    """every byte of the buffer is random: what lies outside the ROIs must come back as it went in"""
    return np.random.RandomState(2000 + len(c["name"]) + c["cols"]).randint(0, 256, rot_geometry(c)[1]).astype(np.uint8)


def rot_rows(c):
    """rows of (byte offset of the view, stride, x, y, w, h) in launch order"""
    stride, _ = rot_geometry(c)
    return [(c["view_off"], stride) + tuple(q) for q in c["rois"]]


def rot_applied(c):
    """the rows the launch applies: those inside seg"""
    return rot_rows(c)[:c["seg"][-1]]


# ------------------------------------------------------------------------------------------------------------ grouping
def _parity_lists():
    """the five rectangle lists of tests/test_gpu_parity.py::test_rotations_of_overlapping_rois_keep_request_order"""
    rs = np.random.RandomState(77)
    rs.randint(0, 256, (240, 330, 3))
    cases = [[(10, 10, 100, 40), (60, 30, 120, 41), (150, 50, 51, 33), (10, 10, 100, 40), (0, 0, 330, 240)],
             [(5, 5, 1, 1), (5, 5, 2, 1), (5, 5, 1, 2), (7, 3, 9, 1), (3, 7, 1, 9), (0, 0, 3, 3)],
             [(x, y, 37, 21) for y in range(0, 200, 13) for x in range(0, 280, 29)],
             [(x, y, 20, 10) for y in range(0, 230, 10) for x in range(0, 320, 20)]]
    rnd = []
    for _ in range(200):
        w, h = rs.randint(1, 120), rs.randint(1, 60)
        rnd.append((int(rs.randint(0, 330 - w + 1)), int(rs.randint(0, 240 - h + 1)), int(w), int(h)))
    cases.append(rnd)
    return cases


def _grouping_cases():
    G = {"parity_%d" % i: (r, [0] * len(r)) for i, r in enumerate(_parity_lists())}
    G["two_views_same_rects"] = ([A, B, A, B, C_, C_], [0, 0, 1, 1, 0, 1])
    G["two_views_interleaved_chain"] = ([A, A, B, C_, B, C_], [3, 9, 9, 3, 3, 9])
    G["late_merge"] = ([(0, 0, 10, 10), (30, 0, 10, 10), (0, 30, 4, 4), (60, 0, 10, 10), (5, 5, 60, 3)], [0] * 5)  # the last ROI joins three roots
    G["late_merge_of_chains"] = ([(0, 0, 10, 10), (30, 0, 10, 10), (8, 8, 5, 5), (28, 8, 5, 5), (12, 10, 17, 2)], [0] * 5)
    G["touching_is_not_intersecting"] = ([(0, 0, 10, 10), (10, 0, 10, 10), (0, 10, 10, 10)], [0] * 3)
    G["one"] = ([(3, 4, 5, 6)], [7])
    for g in ROT_GROUPS:
        if len(g["seg"]) > 1:
            G["launch_" + g["name"]] = (g["rois"], [0] * len(g["rois"]))
    return G


GROUPING = _grouping_cases()

# the case that kills each mutation of crop_ref.MUTATIONS: (family, case name); None: crop_ref.EQUIVALENT has the reason
ODD_ROW = next(c["name"] for c in ROT_CASES if c["rois"][0][3] & 1 and c["rois"][0][3] > 1 and c["rois"][0][2] >= 3)
KILLED_BY = {
    "direct": ("warp", "seam_16x65"),
    "block_64": ("warp", "seam_1x1025"),
    "round_half_away": ("warp", "tie_1_64_5x4"),
    "truncate": ("warp", "tie_3_64_5x4"),
    "w0_inf": ("warp", "w_zero_5x4"),
    "nan_int_min": None,
    "outside_sx_lt0": ("warp", "shift_x_m1_5x4"),
    "outside_sx1_ge_sw": ("warp", "shift_x_swm1_5x4"),
    "border_replicate": ("warp", "shift_y_m1_7x3"),
    "no_round_bias": ("warp", "trans_16_32_5x4"),
    "turn_wrong_flip": ("warp", "turn_3x7"),
    "no_short_clamp": None,
    "rot_middle_row_full": ("rot", ODD_ROW),
    "rot_reverse_order": ("rot", "chain"),
    "rot_half_up": None,
}
# the launches on which an EQUIVALENT mutation's rule is reached: there the mutated reference must still equal the device
REACHED_BY = {
    "nan_int_min": [n for n in WARP_BY_NAME if n.startswith("nan_")],
    "no_short_clamp": [n for n in WARP_BY_NAME if n.startswith(("sat_", "nan_", "w_zero_"))] + ["seam_16x65"],
    "rot_half_up": [c["name"] for c in ROT_CASES if (c["rois"][0][2] * c["rois"][0][3]) & 1],
}
