"""Plain numpy restatement of the contract of the resize-and-normalise kernels (csrc/kernels_pre.hip: det_pre_kernel,
line_pre_kernel, line_pre_ragged_kernel, all on resize_px_scaled), in the spirit of net_ref.py: written from the rules, not
from the kernels, proved equal to the oracle library bit for bit on the CPU (tests/test_pre_ref.py) and then used as the
yardstick of the device (tests/test_gpu_pre_ops.py), which lets those tests carry its mutations.

The rules:
  resize = cv::resize(src, dst, Size(dw, dh)) on CV_8UC3, default INTER_LINEAR
    * dsize == ssize: a copy
    * scale = 1 / ((double)dst / src) per axis; both scales exactly 2: INTER_LINEAR silently becomes the 2x2 area mean
      (a + b + c + d + 2) >> 2
    * else per destination index d: f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= s (float32 operations)
        x: s < 0 -> s = 0, f = 0 (left clamp); s + 1 >= sw -> the pixel is S[sw - 1] * 2048 alone (dx >= xmax)
        y: the fraction is kept, the two ROWS s and s + 1 are clipped into the image
      coefficients saturate_cast<short>(cvRound(c * 2048)): to nearest (even), clamped to int16
      v = ((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2 >> 2, S = p0 * a0 + p1 * a1 per source row
  normalise = per channel fmaf((float)v * (float)(1 / 255.), scale, (float)(-mean * scale)) (make_norm_lut)
  pad: recognizer - byte 0 BEFORE normalising (= lut[0]); classifier - 0.0f AFTER normalising
  layouts: detector [N][dh][dw][3]; lines [slot][imgH][imgW][3]; ragged - line i [imgH][tensor_w_i][3] at pixel
  imgH * (tensor widths before it)

MUTATIONS: each switches ONE rule wrong.  EQUIVALENT names those that cannot change any result, with the reason."""
from fractions import Fraction

import numpy as np

MUTATIONS = ("coef_truncate", "no_area", "area_one_axis", "no_right_edge", "no_vclamp", "rec_pad_after_norm", "cls_pad_before_norm",
             "slot_ignored", "ragged_first_pixel")
# coef_truncate:       coefficients truncated instead of rounded to nearest
# no_area:             an exact 2x2 decimation stays bilinear
# area_one_axis:       the area mean is taken as soon as ONE axis is exactly halved (its 2x2 window clamped into the image)
# no_right_edge:       the right-edge rule dropped: the fraction is kept and the second tap wraps to column 0
# no_vclamp:           the two rows are not clipped: they wrap around the image
# rec_pad_after_norm:  the recognizer's pad is 0.0f after normalising
# cls_pad_before_norm: the classifier's pad is byte 0 before normalising
# slot_ignored:        line i is written to slot i
# ragged_first_pixel:  the first pixel of every ragged line but the first is looked up in the line before it (and takes that
#                      line's last row, column 0)
EQUIVALENT = {
    "no_area": "at an exact halving f = 0.5 on both axes, so all four coefficients are 1024 and the bilinear formula is "
               "((1024 * (1024 * a >> 4) >> 16) + (1024 * (1024 * b >> 4) >> 16) + 2) >> 2 = (a + b + 2) >> 2 with a, b the sums of "
               "the two taps of a row: the area mean, bit for bit, for every input (tests/test_pre_ref.py proves it over all a, b)",
}

FILL = 0xA5  # OCR_SELFTEST_FILL: what the self-test entry points leave where no descriptor writes
PAD_REC, PAD_CLS = 0, 1
STAGES = {  # (mean, scale) float32 literals: ocr_det.h:121-122, ocr_rec.h:108-109, ocr_cls.h:93-94
    "det": ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)),
    "rec": ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)),
    "cls": ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)),
}
DBL_EPSILON = 2.220446049250313e-16


# ------------------------------------------------------------------------------------------------------ normalisation
def _round_f32(fr):
    """the float32 nearest to the rational fr, ties to even (no double rounding through float64)"""
    c = np.float32(float(fr))
    cands = (np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf)))
    return min(cands, key=lambda q: (abs(Fraction(float(q)) - fr), int(np.float32(q).view(np.uint32)) & 1))


def norm_constants(stage):
    """(e, a[3], b[3]) float32: the three rounded constants of Normalize::Run for a stage"""
    mean, std = STAGES[stage]
    e = np.float32(1.0 / 255.0)
    a = [np.float32(1) / np.float32(s) for s in std]                                  # 1 / 0.229f: a float32 division
    b = [np.float32(-np.float64(np.float32(m)) * np.float64(k)) for m, k in zip(mean, a)]  # the f32 x f32 product is exact in f64
    return e, a, b


_LUTS = {}


def norm_lut(stage):
    """float32 [3, 256]: make_norm_lut's table - one float32 product, one exactly rounded fused multiply-add"""
    if stage not in _LUTS:
        e, a, b = norm_constants(stage)
        lut = np.zeros((3, 256), np.float32)
        for c in range(3):
            for v in range(256):
                f = np.float32(v) * e
                lut[c, v] = _round_f32(Fraction(float(f)) * Fraction(float(a[c])) + Fraction(float(b[c])))
        _LUTS[stage] = lut
    return _LUTS[stage]


def normalise(u8, stage):
    lut = norm_lut(stage)
    return np.stack([lut[c][u8[..., c]] for c in range(3)], -1)


# ------------------------------------------------------------------------------------------------------------- resize
def _positions(n_dst, scale):
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    return s, (f - s.astype(np.float32)).astype(np.float32)


def _fixed(c, mut):
    v = (c * np.float32(2048)).astype(np.float32)
    r = np.trunc(v) if "coef_truncate" in mut else np.rint(v)  # cvRound: to nearest, ties to even
    return np.clip(r, -32768, 32767).astype(np.int64)


def _area(src, dh, dw):
    """2x2 mean whose window is clamped into the image (inside it whenever both axes are exactly halved)"""
    sh, sw = src.shape[:2]
    y0, x0 = np.minimum(2 * np.arange(dh), sh - 1), np.minimum(2 * np.arange(dw), sw - 1)
    y1, x1 = np.minimum(2 * np.arange(dh) + 1, sh - 1), np.minimum(2 * np.arange(dw) + 1, sw - 1)
    s = src.astype(np.int64)
    return ((s[y0][:, x0] + s[y0][:, x1] + s[y1][:, x0] + s[y1][:, x1] + 2) >> 2).astype(np.uint8)


def resize(src, dh, dw, mut=()):
    """cv::resize(src [sh, sw, 3] u8, Size(dw, dh)), INTER_LINEAR -> u8 [dh, dw, 3]"""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 3 and src.shape[2] == 3
    sh, sw = src.shape[:2]
    if sh == dh and sw == dw:
        return src.copy()
    scale_x, scale_y = 1.0 / (np.float64(dw) / sw), 1.0 / (np.float64(dh) / sh)
    ix, iy = int(np.rint(scale_x)), int(np.rint(scale_y))
    hx, hy = abs(scale_x - ix) < DBL_EPSILON and ix == 2, abs(scale_y - iy) < DBL_EPSILON and iy == 2
    if "no_area" not in mut and ((hx and hy) or ("area_one_axis" in mut and (hx or hy))):
        return _area(src, dh, dw)
    sx, fx = _positions(dw, scale_x)
    sy, fy = _positions(dh, scale_y)
    left = sx < 0
    sx, fx = np.where(left, 0, sx), np.where(left, np.float32(0), fx)
    edge = sx + 1 >= sw  # dx >= xmax
    if "no_right_edge" in mut:
        x1 = (sx + 1) % sw
        edge = np.zeros_like(edge)
    else:
        sx, fx = np.where(edge, sw - 1, sx), np.where(edge, np.float32(0), fx)
        x1 = np.minimum(sx + 1, sw - 1)
    a0, a1 = _fixed(np.float32(1) - fx, mut), _fixed(fx, mut)
    b0, b1 = _fixed(np.float32(1) - fy, mut), _fixed(fy, mut)
    if "no_vclamp" in mut:
        y0, y1 = sy % sh, (sy + 1) % sh
    else:
        y0, y1 = np.clip(sy, 0, sh - 1), np.clip(sy + 1, 0, sh - 1)
    s = src.astype(np.int64)
    rows = np.where(edge[None, :, None], s[:, sx] * 2048, s[:, sx] * a0[None, :, None] + s[:, x1] * a1[None, :, None])  # [sh, dw, 3]
    v = (((b0[:, None, None] * (rows[y0] >> 4)) >> 16) + ((b1[:, None, None] * (rows[y1] >> 4)) >> 16) + 2) >> 2
    return np.clip(v, 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------ layouts
def det_pre(imgs, dh, dw, mut=()):
    """N same-size images -> (f32 [N, dh, dw, 3], u8 tap [N, dh, dw, 3])"""
    tap = np.stack([resize(im, dh, dw, mut) for im in imgs])
    return normalise(tap, "det"), tap


def _line(parent, q, imgH, tensor_w, pad_mode, stage, mut):
    x, y, w, h, resize_w = (int(v) for v in q[:5])
    assert 1 <= resize_w <= tensor_w and 0 <= x and 0 <= y and x + w <= parent.shape[1] and y + h <= parent.shape[0]
    u8 = resize(parent[y:y + h, x:x + w], imgH, resize_w, mut)
    out = np.empty((imgH, tensor_w, 3), np.float32)
    out[:, :resize_w] = normalise(u8, stage)
    after = pad_mode == PAD_CLS
    if pad_mode == PAD_REC and "rec_pad_after_norm" in mut:
        after = True
    if pad_mode == PAD_CLS and "cls_pad_before_norm" in mut:
        after = False
    out[:, resize_w:] = np.float32(0) if after else norm_lut(stage)[:, 0]
    return out, u8


def filled(shape):
    """float32 array whose every byte is FILL"""
    return np.full(tuple(shape) + (4,), FILL, np.uint8).view(np.float32).reshape(shape)


def line_pre(parent, lines, imgH, imgW, nslots, pad_mode, stage="rec", mut=()):
    """parent u8 [rows, cols, 3] (any row stride); lines: rows of (x, y, w, h, resize_w, slot) -> f32 [nslots, imgH, imgW, 3];
    slots no line names hold the fill"""
    out = filled((nslots, imgH, imgW, 3))
    for i, q in enumerate(lines):
        out[i if "slot_ignored" in mut else int(q[5])] = _line(parent, q, imgH, imgW, pad_mode, stage, mut)[0]
    return out


def line_pre_ragged(parent, lines, imgH, stage="rec", mut=()):
    """lines: rows of (x, y, w, h, resize_w, tensor_w) -> list of f32 [imgH, tensor_w, 3], the recognizer's pad"""
    outs = [_line(parent, q, imgH, int(q[5]), PAD_REC, stage, mut)[0] for q in lines]
    if "ragged_first_pixel" in mut:
        first = [o[imgH - 1, 0].copy() for o in outs]
        for i in range(1, len(outs)):
            outs[i][0, 0] = first[i - 1]
    return outs


def bits(a):
    """what the tests compare: float32 as uint32 (so that -0.0 and NaN cannot slip through), anything else as it is"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a
