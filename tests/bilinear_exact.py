"""An independent evaluation of cv::resize INTER_LINEAR on 8-bit data, shared by tests/test_oracle_imgproc.py and
tests/test_pre_ref.py: the same sample positions (float32 arithmetic on the coordinates, as OpenCV) but the interpolation
itself in exact rational arithmetic, plus a plain-Python big-int restatement of the fixed-point formula (written from the
formula, not from the oracle's C)."""
from fractions import Fraction

import numpy as np


def coords(n_dst, n_src, scale, clamp):
    """x: positions left of the first / right of the last pixel centre take that pixel alone (weight 0 on the
    neighbour); y: the fraction is kept and the two ROWS are clipped instead (resize.cpp, resizeGeneric_)"""
    out = []
    for d in range(n_dst):
        f = np.float32((d + 0.5) * scale - 0.5)
        s = int(np.floor(f))
        f = np.float32(f - np.float32(s))
        if clamp and s < 0:
            s, f = 0, np.float32(0)
        if clamp and s >= n_src - 1:
            s, f = n_src - 1, np.float32(0)
        out.append((s, f))
    return out


def _sat(v):
    return int(max(-32768, min(32767, int(np.rint(np.float32(v))))))


def fixed_against_exact(img, got, dh, dw, points=None):
    """img [sh, sw, 3] u8 resized to got [dh, dw, 3] (not an identity, not an exact halving of both axes).  At every (y, x) of
    `points` (None: all): asserts that `got` equals the big-int restatement of the fixed-point formula, and returns
    (worst, exact_hits, total) of |got - exactly rounded rational bilinear value| over the visited bytes."""
    sh, sw = img.shape[:2]
    sx_, sy_ = 1.0 / (np.float64(dw) / sw), 1.0 / (np.float64(dh) / sh)   # resize.cpp: scale = 1 / inv_scale
    cx, cy = coords(dw, sw, sx_, True), coords(dh, sh, sy_, False)
    if points is None:
        points = [(y, x) for y in range(dh) for x in range(dw)]
    worst, exact_hits, total = 0, 0, 0
    for y, x in points:
        (sy, fy), (sx, fx) = cy[y], cx[x]
        x1 = min(sx + 1, sw - 1)
        y0, y1 = min(max(sy, 0), sh - 1), min(max(sy + 1, 0), sh - 1)
        a0, a1 = _sat((np.float32(1) - fx) * np.float32(2048)), _sat(fx * np.float32(2048))
        b0, b1 = _sat((np.float32(1) - fy) * np.float32(2048)), _sat(fy * np.float32(2048))
        FX, FY = Fraction(float(fx)), Fraction(float(fy))
        for c in range(3):
            p00, p01, p10, p11 = (int(img[y0, sx, c]), int(img[y0, x1, c]), int(img[y1, sx, c]), int(img[y1, x1, c]))
            # plain big-int restatement of the fixed-point formula
            r0, r1 = p00 * a0 + p01 * a1, p10 * a0 + p11 * a1
            v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2
            assert got[y, x, c] == max(0, min(255, v)), (y, x, c)
            # exact rational bilinear at the same float32 sample offsets
            e = (p00 * (1 - FX) + p01 * FX) * (1 - FY) + (p10 * (1 - FX) + p11 * FX) * FY
            r = int(e + Fraction(1, 2))
            worst = max(worst, abs(int(got[y, x, c]) - r))
            exact_hits += int(got[y, x, c]) == r
            total += 1
    return worst, exact_hits, total


def float64_bilinear(img, dh, dw):
    """the same interpolation in float64 (error far below 1e-9 of a grey level): a screen for images too large for the
    rational evaluation at every pixel - see tests/test_pre_ref.py"""
    sh, sw = img.shape[:2]
    sx_, sy_ = 1.0 / (np.float64(dw) / sw), 1.0 / (np.float64(dh) / sh)
    cx, cy = coords(dw, sw, sx_, True), coords(dh, sh, sy_, False)
    sx, fx = np.array([c[0] for c in cx]), np.array([np.float64(c[1]) for c in cx])
    sy, fy = np.array([c[0] for c in cy]), np.array([np.float64(c[1]) for c in cy])
    x1 = np.minimum(sx + 1, sw - 1)
    y0, y1 = np.clip(sy, 0, sh - 1), np.clip(sy + 1, 0, sh - 1)
    s = img.astype(np.float64)
    rows = s[:, sx] * (1 - fx)[None, :, None] + s[:, x1] * fx[None, :, None]
    return rows[y0] * (1 - fy)[:, None, None] + rows[y1] * fy[:, None, None]
