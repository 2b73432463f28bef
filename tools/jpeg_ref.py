"""The pixel half of JPEG decoding as exact integer arithmetic on whole planes (numpy int64): what csrc/kernels_jpeg.hip and
host/jpeg_decode.h must compute from a coefficient descriptor.  Written from libjpeg-turbo's sources, not from either of them:
  jidctint.c  jpeg_idct_islow: dequantise, two 8-point passes with CONST_BITS = 13 and PASS1_BITS = 2, pass 1 down the
              columns into an int workspace (DESCALE by 11), pass 2 along the rows (DESCALE by 18), range_limit = + 128 and a
              clamp to 0..255.  DESCALE(x, n) = (x + (1 << (n - 1))) >> n.
  jdsample.c  jinit_upsampler's choice per component from (hexp, vexp) = (max_h / h, max_v / v) and downsampled_width:
              (1, 1) fullsize (copy); (2, 1) h2v1_fancy when downsampled_width > 2 else h2v1 replication; (1, 2) h1v2_fancy;
              (2, 2) h2v2_fancy when downsampled_width > 2 else h2v2 replication; any other integral pair int_upsample (box).
              Context rows above the first and below the last real row are that row again (jdmainct.c); the fancy forms
              run over downsampled_width samples, first and last column by their own formulas.
  jdcolor.c   build_ycc_rgb_table / ycc_rgb_convert with SCALEBITS = 16, FIX(x) = (int)(x * 65536 + 0.5); ycck_cmyk_convert:
              C, M, Y = 255 - R, G, B of those tables, K as stored; grey and RGB as stored.
  OpenCV      icvCvt_CMYK2BGR_8u_C4C3R (imgcodecs/src/utils.cpp) on libjpeg's samples: channel = k - (((255 - c) * k) >> 8).
  EXIF        orientation 1..8 applied to the finished stored image, as cv::imdecode turns it.

A frame is the dict tests/jpeg_frames.py makes: rows, cols (the stored size), color (0 grey, 1 YCbCr, 2 RGB, 3 CMYK, 4 YCCK),
orientation, comps = [dict(h, v, bw, bh, dw, dh, quant[64], coef[bw * bh * 64])], blocks row-major, natural order inside.
decode(frame) -> the oriented image as packed BGR.

Domain.  libjpeg's C path keeps products in JLONG (64 bits) and the pass-1 workspace in int (32 bits); so do the host (long /
int after descale) and the kernel (long long / int).  Everything here is exact, so all of them agree as long as no value
leaves those widths.  Let A = max |coef * quant| of a block.  One 8-point pass maps inputs bounded by A to outputs bounded by
G * A, G = GAIN = the largest absolute row sum of the pass's integer matrix (computed below from unit vectors: 61214 <
2^16; every partial sum inside the pass is bounded by the same kind of sum, below 2^17 * A).  The workspace therefore holds at
most G * A / 2^11 + 1, which fits an int when A <= DEQUANT_BOUND = (2^31 - 2) * 2^11 // G (71847069 > 2^26).  Pass 2 then
sees |ws| < 2^31 and stays below 2^31 * 2^17 = 2^48, far inside 64 bits.  An 8-bit table (quant <= 255) with any int16
coefficient gives A <= 32768 * 255 = 8355840 < DEQUANT_BOUND: the full coefficient range is inside the domain.  Beyond the
bound libjpeg's C path wraps where its SIMD path saturates; nothing is claimed there, and tests/jpeg_frames.random_frame
asserts that its frames stay inside (in_domain).

MUTATIONS: each switches ONE rule wrong (decode(frame, mut=name)).  EQUIVALENT names those that cannot change a result."""
import numpy as np

GREY, YCBCR, RGB, CMYK, YCCK = range(5)
COPY, H2V1, H2V2, H1V2, BOX = "copy", "h2v1", "h2v2", "h1v2", "box"

MUTATIONS = ("h2v2_bias_swapped", "h1v2_bias_swapped", "h2v1_edge_fancy", "narrow_fancy", "lower_clamp_off_by_one", "box_y_uses_hexp",
             "pass1_no_round", "pass2_no_round", "idct_wrap", "orient_5_7_swapped", "orient_6_8_swapped", "cmyk_div255",
             "green_constants_swapped", "plane_search")
# h2v2_bias_swapped:       h2v2_fancy rounds with 7 where libjpeg has 8 and the other way round
# h1v2_bias_swapped:       h1v2_fancy rounds the upper row with 2 and the lower with 1
# h2v1_edge_fancy:         the last column of h2v1_fancy goes through the interior formula, (3 * in[dw-1] + in[dw] + 2) >> 2 with the
#                          stored sample right of the component (block padding), instead of being copied
# narrow_fancy:            the downsampled_width > 2 condition dropped: a component 1 or 2 samples wide takes the fancy form
# lower_clamp_off_by_one:  the row below the last real row of h2v2 / h1v2 is the next stored row (block padding), not the last real row
# box_y_uses_hexp:         int_upsample repeats rows hexp times instead of vexp times
# pass1_no_round:          pass 1 shifts right by 11 without adding 1 << 10
# pass2_no_round:          pass 2 shifts right by 18 without adding 1 << 17
# idct_wrap:               the sample + 128 is cut to its low byte instead of clamped
# orient_5_7_swapped:      orientation 5 turns as 7 and 7 as 5
# orient_6_8_swapped:      orientation 6 turns as 8 and 8 as 6
# cmyk_div255:             (255 - c) * k / 255 instead of >> 8
# green_constants_swapped: green takes 0.71414 with Cb and 0.34414 with Cr
# plane_search:            the first block of the second plane is decoded from the last block of the first plane (its
#                          coefficients and table): a block attributed to the neighbouring plane
EQUIVALENT = {}

CONST_BITS, PASS1_BITS = 13, 2


def FIX13(x):
    return int(x * (1 << CONST_BITS) + 0.5)


F0298, F0390, F0541, F0765, F0899, F1175 = FIX13(0.298631336), FIX13(0.390180644), FIX13(0.541196100), FIX13(0.765366865), FIX13(0.899976223), FIX13(1.175875602)
F1501, F1847, F1961, F2053, F2562, F3072 = FIX13(1.501321110), FIX13(1.847759065), FIX13(1.961570560), FIX13(2.053119869), FIX13(2.562915447), FIX13(3.072711026)


def idct_pass(s):
    """one 8-point pass of jpeg_idct_islow along the last axis (int64, before DESCALE)"""
    s = [s[..., k] for k in range(8)]
    z2, z3 = s[2], s[6]
    z1 = (z2 + z3) * F0541
    tmp2 = z1 + z3 * (-F1847)
    tmp3 = z1 + z2 * F0765
    z2, z3 = s[0], s[4]
    tmp0 = (z2 + z3) * (1 << CONST_BITS)
    tmp1 = (z2 - z3) * (1 << CONST_BITS)
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = s[7], s[5], s[3], s[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * F1175
    tmp0, tmp1, tmp2, tmp3 = tmp0 * F0298, tmp1 * F2053, tmp2 * F3072, tmp3 * F1501
    z1, z2, z3, z4 = z1 * (-F0899), z2 * (-F2562), z3 * (-F1961), z4 * (-F0390)
    z3, z4 = z3 + z5, z4 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    return np.stack([tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3], -1)


GAIN = int(np.abs(idct_pass(np.eye(8, dtype=np.int64))).sum(0).max())  # the largest absolute row sum of the pass's matrix
DEQUANT_BOUND = ((1 << 31) - 2) * (1 << (CONST_BITS - PASS1_BITS)) // GAIN


def in_domain(frame):
    """every |coef * quant| of the frame is within DEQUANT_BOUND (module docstring)"""
    for c in frame["comps"]:
        blocks = np.asarray(c["coef"], np.int64).reshape(-1, 64) * np.asarray(c["quant"], np.int64)
        if blocks.size and int(np.abs(blocks).max()) > DEQUANT_BOUND:
            return False
    return True


def descale(x, n, rounded=True):
    return (x + (1 << (n - 1)) if rounded else x) >> n


def idct_blocks(coef, quant, mut=None, raw=False):
    """(n, 64) coefficients -> (n, 8, 8) samples; raw: before + 128 and the clamp"""
    d = (np.asarray(coef, np.int64).reshape(-1, 64) * np.asarray(quant, np.int64).reshape(64)).reshape(-1, 8, 8)
    # pass 1: columns (the transform runs along the last axis, so turn rows into the last axis and back)
    ws = descale(idct_pass(d.transpose(0, 2, 1)), CONST_BITS - PASS1_BITS, mut != "pass1_no_round").transpose(0, 2, 1)
    assert ws.size == 0 or int(np.abs(ws).max()) < (1 << 31), "outside the domain of the reference"
    out = descale(idct_pass(ws), CONST_BITS + PASS1_BITS + 3, mut != "pass2_no_round")
    if raw:
        return out
    return (out + 128) & 255 if mut == "idct_wrap" else np.clip(out + 128, 0, 255)


def planes(frame, mut=None, raw=False):
    """per component its stored plane, (bh * 8, bw * 8)"""
    out = []
    for i, c in enumerate(frame["comps"]):
        coef, quant = np.asarray(c["coef"], np.int64).reshape(-1, 64), c["quant"]
        px = idct_blocks(coef, quant, mut, raw)
        if mut == "plane_search" and i == 1:
            first = frame["comps"][0]
            px[0] = idct_blocks(np.asarray(first["coef"], np.int64).reshape(-1, 64)[-1:], first["quant"], None, raw)[0]
        bw, bh = c["bw"], c["bh"]
        out.append(px.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8))
    return out


def factors(frame):
    comps = frame["comps"]
    return max(c["h"] for c in comps), max(c["v"] for c in comps)


def method_of(hexp, vexp, dw, mut=None):
    """jinit_upsampler's choice"""
    wide = dw > 2 or mut == "narrow_fancy"
    if hexp == 1 and vexp == 1:
        return COPY
    if hexp == 2 and vexp == 1:
        return H2V1 if wide else BOX
    if hexp == 1 and vexp == 2:
        return H1V2
    if hexp == 2 and vexp == 2:
        return H2V2 if wide else BOX
    return BOX


def _neighbour_rows(plane, dh, mut):
    """for vertical factor 2: per output row the near input row and the far one (above for even rows, below for odd rows,
    the first / last real row again at the edges)"""
    r = np.arange(2 * dh) >> 1
    odd = (np.arange(2 * dh) & 1) == 1
    last = min(dh, plane.shape[0] - 1) if mut == "lower_clamp_off_by_one" else dh - 1
    far = np.where(odd, np.minimum(r + 1, last), np.maximum(r - 1, 0))
    return plane[r], plane[far], odd


def _h2_fancy(near3, dw, bias_even, bias_odd, scale, shift, edge=None):
    """the horizontal half of h2v1 / h2v2 fancy over rows `near3` (already 3 * near + far for h2v2, the samples for h2v1):
    out[2x] = (3 v[x] + v[x-1] + bias_even) >> shift, out[2x+1] = (3 v[x] + v[x+1] + bias_odd) >> shift, the first and last
    output column (scale * v + bias) >> shift"""
    v = near3[:, :dw]
    out = np.empty((v.shape[0], 2 * dw), np.int64)
    out[:, 0] = (v[:, 0] * scale + bias_even) >> shift
    out[:, 2 * dw - 1] = (v[:, dw - 1] * scale + bias_odd) >> shift
    if dw > 1:
        out[:, 2::2] = (3 * v[:, 1:] + v[:, :-1] + bias_even) >> shift
        out[:, 1:-1:2] = (3 * v[:, :-1] + v[:, 1:] + bias_odd) >> shift
    if edge is not None:
        out[:, 2 * dw - 1] = (3 * v[:, dw - 1] + edge + bias_odd) >> shift
    return out


def upsample(plane, comp, hmax, vmax, rows, cols, mut=None):
    """the component at full resolution, (rows, cols)"""
    hexp, vexp, dw, dh = hmax // comp["h"], vmax // comp["v"], comp["dw"], comp["dh"]
    method = method_of(hexp, vexp, dw, mut)
    if method == COPY:
        return plane[:rows, :cols]
    if method == BOX:
        ry = hexp if mut == "box_y_uses_hexp" else vexp
        yy = np.minimum(np.arange(rows) // ry, plane.shape[0] - 1)
        return plane[yy][:, np.arange(cols) // hexp]
    if method == H1V2:
        near, far, odd = _neighbour_rows(plane, dh, mut)
        lo, hi = (2, 1) if mut == "h1v2_bias_swapped" else (1, 2)
        return ((3 * near + far + np.where(odd, hi, lo)[:, None]) >> 2)[:rows, :cols]
    if method == H2V1:
        edge = plane[:dh, dw] if mut == "h2v1_edge_fancy" and dw < plane.shape[1] else None
        # first and last column are copies: (4 v + bias) >> 2 = v for bias 1 and 2
        return _h2_fancy(plane[:dh], dw, 1, 2, 4, 2, edge)[:rows, :cols]
    near, far, _ = _neighbour_rows(plane, dh, mut)
    even, odd = (7, 8) if mut == "h2v2_bias_swapped" else (8, 7)
    return _h2_fancy(3 * near + far, dw, even, odd, 4, 4)[:rows, :cols]


def FIX16(x):
    return int(x * 65536 + 0.5)


def ycc_to_rgb(y, cb, cr, mut=None):
    """jdcolor.c: (r, g, b) of int64 arrays"""
    xb, xr = cb - 128, cr - 128
    crr = (FIX16(1.40200) * xr + 32768) >> 16
    cbb = (FIX16(1.77200) * xb + 32768) >> 16
    gb, gr = (FIX16(0.71414), FIX16(0.34414)) if mut == "green_constants_swapped" else (FIX16(0.34414), FIX16(0.71414))
    g = y + ((-gb * xb + 32768 - gr * xr) >> 16)
    return np.clip(y + crr, 0, 255), np.clip(g, 0, 255), np.clip(y + cbb, 0, 255)


def ycc_to_rgb_float(y, cb, cr):
    """the same conversion from the decimal constants in float64, rounded as jdcolor.c rounds (every product of a 17-bit
    constant with an 8-bit value and the sums are exact in float64, so this is an exact statement too)"""
    y, xb, xr = (np.asarray(a, np.float64) for a in (y, np.asarray(cb) - 128, np.asarray(cr) - 128))
    fix = lambda c: np.floor(c * 65536.0 + 0.5)  # noqa: E731
    r = y + np.floor((fix(1.40200) * xr + 32768.0) / 65536.0)
    g = y + np.floor((-fix(0.34414) * xb + 32768.0 - fix(0.71414) * xr) / 65536.0)
    b = y + np.floor((fix(1.77200) * xb + 32768.0) / 65536.0)
    return tuple(np.clip(v, 0, 255).astype(np.int64) for v in (r, g, b))


def cmyk_channel(c, k, mut=None):
    """OpenCV's CMYK -> BGR, one channel"""
    return k - ((255 - c) * k // 255 if mut == "cmyk_div255" else ((255 - c) * k) >> 8)


def colour(full, color, mut=None):
    """full-resolution components -> (rows, cols, 3) B, G, R"""
    if color == GREY:
        r = g = b = full[0]
    elif color == RGB:
        r, g, b = full[:3]
    elif color == YCBCR:
        r, g, b = ycc_to_rgb(full[0], full[1], full[2], mut)
    else:
        if color == CMYK:
            c, m, y = full[:3]
        else:  # ycck_cmyk_convert
            r, g, b = ycc_to_rgb(full[0], full[1], full[2], mut)
            c, m, y = 255 - r, 255 - g, 255 - b
        k = full[3]
        r, g, b = cmyk_channel(c, k, mut), cmyk_channel(m, k, mut), cmyk_channel(y, k, mut)
    return np.stack([b, g, r], -1)


def orient(img, orientation, mut=None):
    """EXIF orientation 1..8 (0 as 1) of an array (rows, cols, ...)"""
    o = orientation or 1
    if mut == "orient_5_7_swapped":
        o = {5: 7, 7: 5}.get(o, o)
    if mut == "orient_6_8_swapped":
        o = {6: 8, 8: 6}.get(o, o)
    if o == 1:
        return img
    if o == 2:
        return img[:, ::-1]            # mirrored left to right
    if o == 3:
        return img[::-1, ::-1]         # turned by 180 degrees
    if o == 4:
        return img[::-1]               # mirrored top to bottom
    if o == 5:
        return np.swapaxes(img, 0, 1)  # transposed
    if o == 6:
        return np.rot90(img, -1)       # 90 degrees clockwise
    if o == 7:
        return np.swapaxes(img[::-1, ::-1], 0, 1)  # transverse
    if o == 8:
        return np.rot90(img, 1)        # 90 degrees counter-clockwise
    raise ValueError("orientation %r" % (orientation,))


def stored(frame, mut=None):
    """the stored image, (rows, cols, 3) BGR, int64"""
    rows, cols = frame["rows"], frame["cols"]
    hmax, vmax = factors(frame)
    full = [upsample(p, c, hmax, vmax, rows, cols, mut) for p, c in zip(planes(frame, mut), frame["comps"])]
    return colour(full, frame["color"], mut)


def decode(frame, mut=None):
    """the oriented image as packed BGR uint8"""
    assert mut is None or mut in MUTATIONS, mut
    return np.ascontiguousarray(orient(stored(frame, mut), frame["orientation"], mut)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------- branch census
BRANCHES = ("copy", "box.narrow_dw1", "box.narrow_dw2", "box.other", "h2v1.first", "h2v1.last", "h2v1.even", "h2v1.odd",
            "h2v2.first", "h2v2.last", "h2v2.even", "h2v2.odd", "h2v2.top_clamped", "h2v2.bottom_clamped", "h2v2.dh1", "h2v2.dh2",
            "h2v2.dw3", "h2v1.dw3", "h2v1.ends_even", "h2v2.ends_even", "h1v2.upper", "h1v2.lower", "h1v2.top_clamped", "h1v2.bottom_clamped", "h1v2.dh1")


def branch_counts(frame):
    """{branch: output pixels of the stored image that take it}, summed over the components - which rule of the per-pixel
    form of jdsample.c a pixel (x, y) meets, from the geometry alone"""
    rows, cols = frame["rows"], frame["cols"]
    hmax, vmax = factors(frame)
    n = dict.fromkeys(BRANCHES, 0)
    x, y = np.arange(cols), np.arange(rows)
    for c in frame["comps"]:
        hexp, vexp, dw, dh = hmax // c["h"], vmax // c["v"], c["dw"], c["dh"]
        m = method_of(hexp, vexp, dw)
        if m == COPY:
            n["copy"] += rows * cols
        elif m == BOX:
            n["box.narrow_dw1" if hexp == 2 and vexp <= 2 and dw == 1 else "box.narrow_dw2" if hexp == 2 and vexp <= 2 and dw == 2 else "box.other"] += rows * cols
        if m in (H2V1, H2V2):
            first, last = x == 0, x == 2 * dw - 1
            for key, sel in (("first", first), ("last", last), ("even", ~first & ~last & (x % 2 == 0)), ("odd", ~first & ~last & (x % 2 == 1))):
                n[m + "." + key] += int(sel.sum()) * rows
            n[m + ".dw3"] += rows * cols * (dw == 3)
            n[m + ".ends_even"] += rows * (cols == 2 * dw - 1)  # the last column by the interior rule for even columns
        if m in (H2V2, H1V2):
            n[m + ".top_clamped"] += int((y == 0).sum()) * cols
            n[m + ".bottom_clamped"] += int((y == 2 * dh - 1).sum()) * cols
            n[m + ".dh1"] += rows * cols * (dh == 1)
        if m == H2V2:
            n["h2v2.dh2"] += rows * cols * (dh == 2)
        if m == H1V2:
            n["h1v2.upper"] += int((y % 2 == 0).sum()) * cols
            n["h1v2.lower"] += int((y % 2 == 1).sum()) * cols
    return n
