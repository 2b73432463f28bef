"""Plain NumPy / Python-float restatement of the crop geometry between detector and recognizer: plan_rotate_crop (csrc/crop.h),
warp_crop_kernel and rotate180_groups_kernel (csrc/kernels_pre.hip) and the properties of the grouping of rot_groups.h, in the
spirit of pre_ref.py: written from the rules, not from the kernels, proved equal to the oracle library on the CPU wherever the
oracle can express a case (tests/test_crop_ref.py) and then used as the yardstick of the device (tests/test_gpu_crop_ops.py),
which lets those tests carry its mutations.  Python floats are IEEE doubles and nothing here is contracted into a fused
multiply-add, so the inverse homography must equal the library's bit for bit.

The rules (Utility::GetRotateCropImage; cv::getPerspectiveTransform, cv::warpPerspective, cv::rotate of OpenCV 4.x):
  plan   bounding box of the four corners; refused when it is empty or leaves the image
         cw = int(sqrt(dx^2 + dy^2)) of corners 0-1, ch of corners 0-3; cw or ch 0: the output takes the box's size
         dh >= 1.5 dw: the result is turned by 90 degrees; bw0 = min(1024 / min(16, dh), dw)
         8x8 system of the four correspondences, LU with row pivoting, singular below 100 eps: all-zero solution;
         M[8] = 1; 3x3 closed-form inverse, determinant exactly 0: all zeros
  warp   per destination pixel (x, y), with xb the start of its bw0-column block and x1 = x - xb:
           X0 = m0 xb + m1 y + m2, Y0 = m3 xb + m4 y + m5, W0 = m6 xb + m7 y + m8 (left to right)
           W = W0 + m6 x1; W = W != 0 ? 32 / W : 0
           fX = max(INT_MIN, min(INT_MAX, (X0 + m0 x1) W)) with std::min(a, b) = b < a ? b : a and std::max(a, b) = a < b ? b : a:
           a NaN becomes INT_MAX; the same for fY
           X = nearest-even integer, sx = clamp_short(X >> 5) (arithmetic shift), fx = X & 31; the same for Y
           the four taps (sy, sx), (sy, sx + 1), (sy + 1, sx), (sy + 1, sx + 1), 0 where a tap lies outside the source, weights
           (32 - fy)(32 - fx) 32 ..., v = (sum + (1 << 14)) >> 15; sx >= sw, sx + 1 < 0, sy >= sh or sy + 1 < 0: 0 at once
         turn: pixel (x, y) of the warp is row dw - 1 - x, column y of the dw x dh result
  rotate ROI after ROI in request order: pixel i <-> total - 1 - i of the ROI's raster order for i < total / 2

MUTATIONS: each switches ONE rule wrong.  EQUIVALENT names those that cannot change any result, with the reason."""
import math

import numpy as np

MUTATIONS = ("direct", "block_64", "round_half_away", "truncate", "w0_inf", "nan_int_min", "outside_sx_lt0", "outside_sx1_ge_sw",
             "border_replicate", "no_round_bias", "turn_wrong_flip", "no_short_clamp", "rot_middle_row_full", "rot_reverse_order",
             "rot_half_up")
# direct:              m0 x + m1 y + m2 evaluated at the pixel itself, without the block base
# block_64:            the block is 64 columns wide whatever dh is (what the product-level tests exercise)
# round_half_away:     a tie is rounded away from zero instead of to the even integer
# truncate:            the coordinate is truncated
# w0_inf:              W == 0 gives an infinite scale instead of 0
# nan_int_min:         a NaN coordinate becomes INT_MIN
# outside_sx_lt0:      a pixel counts as outside as soon as sx < 0 (sy < 0)
# outside_sx1_ge_sw:   a pixel counts as outside as soon as sx + 1 >= sw (sy + 1 >= sh)
# border_replicate:    taps outside the source take the nearest source pixel
# no_round_bias:       no + (1 << 14) before the >> 15
# turn_wrong_flip:     the turn writes row x instead of row dw - 1 - x
# no_short_clamp:      sx, sy are not clamped to int16
# rot_middle_row_full: the middle row of an odd height is swapped over its full width (every pair twice: the row stays)
# rot_reverse_order:   the ROIs are applied last to first
# rot_half_up:         total / 2 rounded up
EQUIVALENT = {
    "no_short_clamp": "X is already clamped to int32, so |X >> 5| < 2^26 and the short clamp only moves values beyond +-32767, which lie outside "
                      "every source of up to 8192 columns with or without it",
    "nan_int_min": "INT_MAX gives sx = 32767 >= sw and INT_MIN gives sx = -32768 with sx + 1 < 0: the pixel is 0 either way",
    "rot_half_up": "the one extra pair of an odd total is the centre pixel with itself",
}

FILL = 0xA5  # OCR_SELFTEST_FILL
INT_MAX, INT_MIN = 2147483647.0, -2147483648.0
EPS100 = 2.220446049250313e-16 * 100


# --------------------------------------------------------------------------------------------------------------- plan
def solve8(a, b):
    """Gaussian elimination with row pivoting, one right-hand side, in place; False: singular"""
    for col in range(8):
        piv = col
        for r in range(col + 1, 8):
            if abs(a[r][col]) > abs(a[piv][col]):
                piv = r
        if abs(a[piv][col]) < EPS100:
            return False
        if piv != col:
            for c in range(col, 8):
                a[col][c], a[piv][c] = a[piv][c], a[col][c]
            b[col], b[piv] = b[piv], b[col]
        ninv = -1 / a[col][col]
        for r in range(col + 1, 8):
            f = a[r][col] * ninv
            for c in range(col + 1, 8):
                a[r][c] += f * a[col][c]
            b[r] += f * b[col]
    for r in range(7, -1, -1):
        acc = b[r]
        for c in range(r + 1, 8):
            acc -= a[r][c] * b[c]
        b[r] = acc / a[r][r]
    return True


def inverse3(m):
    c00, c01, c02 = m[4] * m[8] - m[5] * m[7], m[3] * m[8] - m[5] * m[6], m[3] * m[7] - m[4] * m[6]
    det = m[0] * c00 - m[1] * c01 + m[2] * c02
    if det == 0.0:
        return [0.0] * 9
    s = 1.0 / det
    return [c00 * s, (m[2] * m[7] - m[1] * m[8]) * s, (m[1] * m[5] - m[2] * m[4]) * s,
            (m[5] * m[6] - m[3] * m[8]) * s, (m[0] * m[8] - m[2] * m[6]) * s, (m[2] * m[3] - m[0] * m[5]) * s,
            c02 * s, (m[1] * m[6] - m[0] * m[7]) * s, (m[0] * m[4] - m[1] * m[3]) * s]


def block_width(dw, dh):
    return min(1024 // min(16, dh), dw)


def plan(rows, cols, box):
    """dict(left, top, sw, sh, dw, dh, rot, orows, ocols, bw0, minv, fwd) of a box (4 x 2 or 8 ints), or None where it is refused"""
    b = [int(v) for v in np.asarray(box).reshape(8)]
    xs, ys = b[0::2], b[1::2]
    x0, x1, y0, y1 = min(xs), max(xs), min(ys), max(ys)
    if x0 < 0 or y0 < 0 or x1 > cols or y1 > rows or x1 <= x0 or y1 <= y0:
        return None
    cw = int(math.sqrt(float(b[0] - b[2]) ** 2 + float(b[1] - b[3]) ** 2))
    ch = int(math.sqrt(float(b[0] - b[6]) ** 2 + float(b[1] - b[7]) ** 2))
    dw, dh = (cw, ch) if cw > 0 and ch > 0 else (x1 - x0, y1 - y0)
    rot = int(float(dh) >= float(dw) * 1.5)
    tx, ty = (0.0, float(cw), float(cw), 0.0), (0.0, 0.0, float(ch), float(ch))
    a = [[0.0] * 8 for _ in range(8)]
    rhs = [0.0] * 8
    for i in range(4):
        sx, sy = float(b[2 * i] - x0), float(b[2 * i + 1] - y0)
        a[i][0] = a[i + 4][3] = sx
        a[i][1] = a[i + 4][4] = sy
        a[i][2] = a[i + 4][5] = 1.0
        a[i][6], a[i][7] = -sx * tx[i], -sy * tx[i]
        a[i + 4][6], a[i + 4][7] = -sx * ty[i], -sy * ty[i]
        rhs[i], rhs[i + 4] = tx[i], ty[i]
    if not solve8(a, rhs):
        rhs = [0.0] * 8
    fwd = rhs + [1.0]
    return dict(left=x0, top=y0, sw=x1 - x0, sh=y1 - y0, dw=dw, dh=dh, rot=rot, orows=dw if rot else dh, ocols=dh if rot else dw,
                bw0=block_width(dw, dh), minv=inverse3(fwd), fwd=fwd)


def bits64(v):
    """doubles as uint64: what a bit-for-bit comparison looks at (-0.0 and NaN cannot slip through)"""
    return np.asarray(v, np.float64).view(np.uint64)


# --------------------------------------------------------------------------------------------------------------- warp
def _to_int(f, mut):
    if "nan_int_min" in mut and f != f:
        f = INT_MIN
    f = f if f < INT_MAX else INT_MAX      # std::min(INT_MAX, f): b < a ? b : a
    f = f if INT_MIN < f else INT_MIN      # std::max(INT_MIN, f): a < b ? b : a
    if "truncate" in mut:
        return int(f)
    if "round_half_away" in mut:
        return int(math.copysign(math.floor(abs(f) + 0.5), f))
    return int(round(f))                   # Python rounds a float to the nearest integer, ties to even


def source_point(m, x, y, bw0, mut=()):
    """(X, Y): the source position of destination pixel (x, y) in 1/32 pixel, as int32 values"""
    if "block_64" in mut:
        bw0 = 64
    xb = x if "direct" in mut else (x // bw0) * bw0
    x1 = x - xb
    X0 = m[0] * xb + m[1] * y + m[2]
    Y0 = m[3] * xb + m[4] * y + m[5]
    W0 = m[6] * xb + m[7] * y + m[8]
    W = W0 + m[6] * x1
    if W != 0.0:
        W = 32.0 / W
    elif "w0_inf" in mut:
        W = math.inf
    else:
        W = 0.0
    return _to_int((X0 + m[0] * x1) * W, mut), _to_int((Y0 + m[3] * x1) * W, mut)


def _short(v, mut):
    return v if "no_short_clamp" in mut else min(32767, max(-32768, v))


def warp(src, m, dw, dh, rot, bw0, mut=()):
    """src u8 [sh, sw, 3], m the 9 doubles destination -> source -> u8 [dh, dw, 3], or [dw, dh, 3] when rot"""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 3 and src.shape[2] == 3
    sh, sw = src.shape[:2]
    s = src.astype(np.int64)
    m = [float(v) for v in m]
    out = np.zeros((dw, dh, 3) if rot else (dh, dw, 3), np.uint8)
    replicate = "border_replicate" in mut

    def tap(yy, xx):
        if replicate:
            return s[min(max(yy, 0), sh - 1), min(max(xx, 0), sw - 1)]
        return s[yy, xx] if 0 <= xx < sw and 0 <= yy < sh else 0

    for y in range(dh):
        for x in range(dw):
            X, Y = source_point(m, x, y, bw0, mut)
            sx, sy, fx, fy = _short(X >> 5, mut), _short(Y >> 5, mut), X & 31, Y & 31
            if "outside_sx_lt0" in mut:
                outside = sx >= sw or sx < 0 or sy >= sh or sy < 0
            elif "outside_sx1_ge_sw" in mut:
                outside = sx + 1 >= sw or sx + 1 < 0 or sy + 1 >= sh or sy + 1 < 0
            else:
                outside = sx >= sw or sx + 1 < 0 or sy >= sh or sy + 1 < 0
            if outside and not replicate:
                v = np.zeros(3, np.int64)
            else:
                v = (tap(sy, sx) * ((32 - fy) * (32 - fx) * 32) + tap(sy, sx + 1) * ((32 - fy) * fx * 32) + tap(sy + 1, sx) * (fy * (32 - fx) * 32)
                     + tap(sy + 1, sx + 1) * (fy * fx * 32) + (0 if "no_round_bias" in mut else 1 << 14)) >> 15
            px = np.clip(v, 0, 255).astype(np.uint8)
            if rot:
                out[x if "turn_wrong_flip" in mut else dw - 1 - x, y] = px
            else:
                out[y, x] = px
    return out


def rotate_crop(img, box, mut=()):
    """Utility::GetRotateCropImage of one box of img u8 [rows, cols, 3], or None where the box is refused"""
    p = plan(img.shape[0], img.shape[1], box)
    if p is None:
        return None
    return warp(img[p["top"]:p["top"] + p["sh"], p["left"]:p["left"] + p["sw"]], p["minv"], p["dw"], p["dh"], p["rot"], p["bw0"], mut)


# ------------------------------------------------------------------------------------------------------------- rotate
def rotate180(buf, rois, mut=()):
    """buf: flat u8; rois: rows of (byte offset of the view, stride, x, y, w, h), applied one after the other -> the buffer afterwards"""
    buf = np.array(buf, np.uint8).reshape(-1)
    rois = [tuple(int(v) for v in q) for q in rois]
    for off, stride, x0, y0, w, h in (reversed(rois) if "rot_reverse_order" in mut else rois):
        yy, xx = np.mgrid[0:h, 0:w]
        at = (off + (y0 + yy) * stride + (x0 + xx) * 3).reshape(-1)   # byte address of every pixel, raster order
        total = w * h
        spans = [(0, (total + 1) // 2 if "rot_half_up" in mut else total // 2)]
        if "rot_middle_row_full" in mut and h & 1:
            spans.append((total // 2, (h // 2) * w + w))               # the rest of the middle row, swapped a second time
        for lo, hi in spans:
            i = np.arange(lo, hi)
            a, b = at[i], at[total - 1 - i]
            for c in range(3):
                t = buf[a + c].copy()
                buf[a + c] = buf[b + c]
                buf[b + c] = t
    return buf


# ----------------------------------------------------------------------------------------------------------- grouping
def intersects(e, q):
    return e[0] < q[0] + q[2] and q[0] < e[0] + e[2] and e[1] < q[1] + q[3] and q[1] < e[1] + e[3]


def grouping_faults(rects, views, order, seg):
    """the properties a grouping (order, seg) of n rectangles must have, checked one by one (no second union-find): the names of
    those it lacks"""
    n = len(rects)
    order, seg = [int(k) for k in order], [int(s) for s in seg]
    bad = []
    if sorted(order) != list(range(n)) or not seg or seg[0] != 0 or seg[-1] != n or any(b <= a for a, b in zip(seg, seg[1:])):
        return ["partition"]
    groups = [order[a:b] for a, b in zip(seg, seg[1:])]
    of = {k: g for g, ks in enumerate(groups) for k in ks}
    if any(ks != sorted(ks) for ks in groups):
        bad.append("request order inside a group")
    if any(intersects(rects[i], rects[j]) and views[i] == views[j] and of[i] != of[j] for i in range(n) for j in range(i + 1, n)):
        bad.append("intersecting ROIs of one view share a group")
    if any(len({views[k] for k in ks}) > 1 for ks in groups):
        bad.append("one view per group")
    for ks in groups:
        seen, todo = {ks[0]}, [ks[0]]
        while todo:
            i = todo.pop()
            for j in ks:
                if j not in seen and views[i] == views[j] and intersects(rects[i], rects[j]):
                    seen.add(j)
                    todo.append(j)
        if len(seen) != len(ks):
            bad.append("every group is connected")
            break
    firsts = [min(ks) for ks in groups]
    if firsts != sorted(firsts):
        bad.append("groups ordered by their first ROI")
    return bad
