"""The cases of the resize-and-normalise kernels (csrc/kernels_pre.hip), shared by tests/test_pre_ref.py (pre_ref == oracle on
every one of them, CPU) and tests/test_gpu_pre_ops.py (device == pre_ref, bit for bit).  The shapes are the smallest at which
each branch and seam of resize_px_scaled and of the three kernels exists; the largest source image is 333x500."""
import numpy as np

IMG_H = 48


# ------------------------------------------------------------------------------------------------------------- images
def image(kind, h, w, seed=0):
    """u8 [h, w, 3]: RandomState bytes, or a structured image that makes a tap error visible"""
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "rand":
        return np.random.RandomState(1000 + seed).randint(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == "ramp":  # a horizontal, a vertical and a diagonal ramp
        return np.stack([xx * 255 // max(1, w - 1), yy * 255 // max(1, h - 1), (xx + yy) * 255 // max(1, h + w - 2)], -1).astype(np.uint8)
    if kind in ("check1", "check2"):  # 0 / 255 checkerboards of period 1 and 2 (the third channel inverted)
        p = 1 if kind == "check1" else 2
        c = (((yy // p) + (xx // p)) & 1) * 255
        return np.stack([c, c, 255 - c], -1).astype(np.uint8)
    raise ValueError(kind)


# ----------------------------------------------------------------------------------------------------------- detector
def _det(name, sh, sw, dh, dw, N=1, off=0, stride_extra=0, image_extra=0, kind="rand"):
    return dict(name=name, sh=sh, sw=sw, dh=dh, dw=dw, N=N, off=off, stride_extra=stride_extra, image_extra=image_extra, kind=kind)


def _det_cases():
    c = []
    for (h, w) in ((32, 32), (32, 64)):
        for n in (1, 3):
            c.append(_det("id_%dx%d_n%d" % (h, w, n), h, w, h, w, N=n))                                    # the 12-byte fast path
            for off in (1, 2, 3):
                c.append(_det("id_%dx%d_n%d_off%d" % (h, w, n, off), h, w, h, w, N=n, off=off))           # the fallback
            c.append(_det("id_%dx%d_n%d_stride1" % (h, w, n), h, w, h, w, N=n, stride_extra=1))
    c.append(_det("id_32x32_n3_imgbytes1", 32, 32, 32, 32, N=3, image_extra=1))                            # images 1, 2 unaligned
    c.append(_det("id_32x64_n3_imgbytes2", 32, 64, 32, 64, N=3, image_extra=2, kind="ramp"))
    c += [_det("half_64x64", 64, 64, 32, 32), _det("half_64x128", 64, 128, 32, 64), _det("half_64x64_check1", 64, 64, 32, 32, kind="check1"),
          _det("half_64x128_n2_off1_ramp", 64, 128, 32, 64, N=2, off=1, kind="ramp")]
    c += [_det("halfy_64x32", 64, 32, 32, 32), _det("halfx_32x64", 32, 64, 32, 32), _det("halfy_64x32_check2", 64, 32, 32, 32, kind="check2")]
    for (h, w) in ((1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (5, 7), (31, 31)):
        c.append(_det("up_%dx%d" % (h, w), h, w, 32, 32))
    c += [_det("up_2x2_off3", 2, 2, 32, 32, off=3), _det("up_3x3_n3_off1", 3, 3, 32, 32, N=3, off=1), _det("up_5x7_ramp", 5, 7, 32, 32, kind="ramp"),
          _det("up_31x31_check1", 31, 31, 32, 32, kind="check1")]
    c += [_det("down_75x100", 75, 100, 32, 64), _det("down_333x500", 333, 500, 96, 160), _det("down_97x33", 97, 33, 64, 32),
          _det("down_33x65", 33, 65, 32, 64), _det("down_75x100_n2_off1_stride1_ramp", 75, 100, 32, 64, N=2, off=1, stride_extra=1, kind="ramp"),
          _det("down_33x65_check2", 33, 65, 32, 64, kind="check2"), _det("down_97x33_check1", 97, 33, 64, 32, kind="check1"),
          # (every scale above is a dyadic fraction, whose coefficients are exact: 50 / 96 and 70 / 36 are not)
          _det("nondyadic_50x70", 50, 70, 96, 36)]
    c += [_det("px1_33x35", 33, 35, 31, 30), _det("px1_64x62_halving", 64, 62, 32, 31), _det("px1_id_31x30", 31, 30, 31, 30),
          _det("px1_id_31x30_n2_off2", 31, 30, 31, 30, N=2, off=2)]
    return c


DET_CASES = _det_cases()
DET_BY_NAME = {c["name"]: c for c in DET_CASES}
DET_TAIL = 16  # bytes behind the last image: a read past the end stays inside the buffer and shows in the outside-bytes check


def det_images(c):
    return [image(c["kind"], c["sh"], c["sw"], seed=i) for i in range(c["N"])]


def det_geometry(c):
    """(src_stride, src_image_bytes, buffer size)"""
    stride = 3 * c["sw"] + c["stride_extra"]
    img_bytes = c["sh"] * stride + c["image_extra"]
    return stride, img_bytes, c["off"] + (c["N"] - 1) * img_bytes + (c["sh"] - 1) * stride + 3 * c["sw"] + DET_TAIL


def det_buffer(c, outside):
    """the flat parent buffer of a case: every byte that is not a pixel of an image is `outside`"""
    stride, img_bytes, size = det_geometry(c)
    buf = np.full(size, outside, np.uint8)
    for i, im in enumerate(det_images(c)):
        for y in range(c["sh"]):
            at = c["off"] + i * img_bytes + y * stride
            buf[at:at + 3 * c["sw"]] = im[y].reshape(-1)
    return buf


# -------------------------------------------------------------------------------------------------------------- lines
PARENT_H, PARENT_W, PARENT_STRIDE = 120, 400, 3 * 400 + 5
ROIS = {  # name -> (x, y, w, h)
    "full": (0, 0, 400, 120),
    "right_bottom": (250, 70, 150, 50),
    "odd_x": (37, 11, 200, 40),
    "1x1": (5, 5, 1, 1),
    "1x300": (50, 60, 300, 1),       # (rows x cols)
    "100x1": (399, 20, 1, 100),
    "2x2": (10, 10, 2, 2),
    "13x37": (101, 33, 37, 13),
}


def natural_w(h, w, imgH, imgW):
    """CrnnResizeImg / ClsResizeImg: resize_w = min(ceil(imgH * cols / rows), imgW) in float32"""
    v = int(np.ceil(np.float32(imgH) * (np.float32(w) / np.float32(h))))
    return min(v, imgW)


def parent_image(kind="rand"):
    return image(kind, PARENT_H, PARENT_W, seed=77)


def parent_rows(img, lines, outside=None):
    """u8 [rows, stride]: the parent with its row padding; outside = None: the image as it is, pad bytes 0x5a; else every
    byte outside the ROIs of `lines` (pad bytes included) set to `outside`"""
    rows = np.full((PARENT_H, PARENT_STRIDE), 0x5A if outside is None else outside, np.uint8)
    px = rows[:, :3 * PARENT_W].reshape(PARENT_H, PARENT_W, 3)
    if outside is None:
        px[:] = img
    else:
        for q in lines:
            x, y, w, h = (int(v) for v in q[:4])
            px[y:y + h, x:x + w] = img[y:y + h, x:x + w]
    return rows


def parent_view(rows):
    return rows[:, :3 * PARENT_W].reshape(PARENT_H, PARENT_W, 3)


def _launch(name, imgW, pad, stage, nslots, lines, kind="rand"):
    return dict(name=name, imgW=imgW, pad=pad, stage=stage, nslots=nslots, lines=[tuple(ROIS[r] if isinstance(r, str) else r) + (rw, s) for r, rw, s in lines],
                kind=kind)


def _line_launches():
    out = []
    for W, pad, stage in ((320, 0, "rec"), (192, 1, "cls"), (321, 0, "rec"), (321, 1, "rec"), (323, 0, "rec"), (323, 1, "rec")):
        tag = "w%d_%s_pad%d" % (W, stage, pad)
        # six lines into reversed slots: the full parent at its natural width, no pad column, one pad column, widths 1, 2, 3
        out.append(_launch(tag + "_a", W, pad, stage, 6, [("full", natural_w(120, 400, IMG_H, W), 5), ("right_bottom", W, 4), ("odd_x", W - 1, 3),
                                                         ("1x1", 1, 2), ("1x300", 2, 1), ("100x1", 3, 0)]))
        # permuted slots: upscale of 2x2 to the whole width, a natural width, the area switch, two identities, width 3
        out.append(_launch(tag + "_b", W, pad, stage, 6, [("2x2", W, 2), ("13x37", natural_w(13, 37, IMG_H, W), 0), ((3, 7, 200, 96), 100, 3),
                                                         ((21, 30, W, 48), W, 5), ((20, 61, W - 1, 48), W - 1, 1), ("13x37", 3, 4)]))
        # three lines into slots {4, 0, 2} of a five-slot tensor: slots 1 and 3 keep the fill
        out.append(_launch(tag + "_c", W, pad, stage, 5, [((40, 24, 320, 96), 160, 4), ("odd_x", 1, 0), ("1x300", W, 2)]))
    out.append(_launch("w320_rec_pad0_ramp", 320, 0, "rec", 4, [("full", 160, 1), ((3, 7, 200, 96), 100, 3), ((21, 30, 319, 48), 319, 0), ("100x1", 2, 2)], kind="ramp"))
    out.append(_launch("w192_cls_pad1_check1", 192, 1, "cls", 3, [("odd_x", 191, 2), ((0, 0, 384, 96), 192, 0), ("1x300", 3, 1)], kind="check1"))
    out.append(_launch("w323_rec_pad0_check2", 323, 0, "rec", 3, [("right_bottom", 144, 0), ("13x37", 322, 2), ("2x2", 2, 1)], kind="check2"))
    return out


LINE_LAUNCHES = _line_launches()
LINE_BY_NAME = {c["name"]: c for c in LINE_LAUNCHES}


def _ragged(name, widths, rws, kind="rand"):
    rois = list(ROIS.values()) + [(3, 7, 200, 96), (21, 30, 40, 48)]
    lines = []
    for i, (tw, rw) in enumerate(zip(widths, rws)):
        roi = rois[(i * 3 + len(widths)) % len(rois)]
        if rw == "id":       # the identity: 48 x resize_w
            roi, rw = (9 + i, 17 + i, tw, IMG_H), tw
        elif rw == "area":   # the area switch: 96 x (2 * resize_w)
            roi, rw = (5 + i, 3 + i, 2 * (tw // 2), 2 * IMG_H), tw // 2
        lines.append(tuple(roi) + (rw, tw))
    return dict(name=name, lines=lines, kind=kind)


EIGHT = (4, 5, 4, 7, 4, 4, 6, 4)  # one 256-thread workgroup spans more than two lines: the forward walk runs several steps
RAGGED_LAUNCHES = [
    _ragged("r_320_333_40_full", (320, 333, 40), (320, 333, 40)),
    _ragged("r_320_333_40_one", (320, 333, 40), (1, 1, 1)),
    _ragged("r_320_333_40_mixed", (320, 333, 40), (160, "area", "id"), kind="ramp"),
    _ragged("r_320_full", (320,), (320,)),
    _ragged("r_320_mid", (320,), (137,)),
    _ragged("r_320_one", (320,), (1,), kind="check1"),
    _ragged("r_323_321_full", (323, 321), (323, 321)),
    _ragged("r_323_321_mixed", (323, 321), (2, 320)),
    _ragged("r_eight_full", EIGHT, EIGHT),
    _ragged("r_eight_one", EIGHT, (1,) * 8),
    _ragged("r_eight_mixed", EIGHT, (4, 1, 3, 7, 2, "id", 5, "area"), kind="check2"),
]
RAGGED_BY_NAME = {c["name"]: c for c in RAGGED_LAUNCHES}

# the case that kills each mutation of pre_ref.MUTATIONS: (family, case name); None: pre_ref.EQUIVALENT has the reason
KILLED_BY = {
    "coef_truncate": ("det", "nondyadic_50x70"),
    "no_area": None,
    "area_one_axis": ("det", "halfy_64x32"),
    "no_right_edge": ("det", "up_5x7"),
    "no_vclamp": ("det", "up_31x31"),
    "rec_pad_after_norm": ("line", "w320_rec_pad0_a"),
    "cls_pad_before_norm": ("line", "w192_cls_pad1_a"),
    "slot_ignored": ("line", "w320_rec_pad0_c"),
    "ragged_first_pixel": ("ragged", "r_eight_full"),
}
HALVINGS = [c["name"] for c in DET_CASES if c["sh"] == 2 * c["dh"] and c["sw"] == 2 * c["dw"]]
