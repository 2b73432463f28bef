"""The probability maps of the detector's post-processing stages (csrc/kernels_post.hip) and their references, shared by
tests/test_post_ref.py (every branch below is really in the maps: asserted on the oracle alone, CPU) and
tests/test_gpu_post_stages.py (ocr_det_post_stages == the oracle, stage by stage).  Maps are at most 192 x 256, box_thresh is
0.5 with blob levels scattered around it, every map has fewer than 1000 borders (the candidate cut has its own test).

Probabilities outside [0, 1] and NaN are out of contract and left out: `(unsigned char)(p * 255)` is undefined for them in the
reference and on the device alike."""
import math

import numpy as np

# (unclip ratio 1.2: UnClip's offset of a 3 x 1 or 4 x 1 mini box is then below half a pixel and rounds away, so that small blobs
# land on both sides of the `ssid < min_size + 2` gate; from 1.34 on every box that passed `ssid >= 3` grows to 5 or more)
THRESH, BOX_THRESH, UNCLIP = 0.3, 0.5, 1.2
ITHRESH = int(math.floor(THRESH * 255))  # 76: a pixel is foreground when trunc(p * 255) > 76
SORT_LDS_CAP = 512                       # border_box_kernel<512, ..>: longer borders are sorted in global memory
CONFIGS = [(mode, compat, dil) for mode in ("fast", "slow") for compat in (45, 410) for dil in (False, True)]


def config_id(cfg):
    return "%s-cv%d-%s" % (cfg[0], cfg[1], "dilate" if cfg[2] else "plain")


# ---------------------------------------------------------------------------------------------------------------- maps
def _level(rs, m):
    """a blob's pixels: a level near box_thresh plus per-pixel noise (all well above THRESH)"""
    return (rs.uniform(0.48, 0.66) + rs.uniform(-0.12, 0.12, int(m.sum()))).astype(np.float32)


N_ROT_RECTS = [0]


def _rot_rects():
    """rotated rectangles at many angles; four of them poke out of the map, one through each edge"""
    H, W = 192, 256
    rs = np.random.RandomState(11)
    f = np.full((H, W), 0.25, np.float32)   # (below THRESH; the box masks reach into it)
    yy, xx = np.mgrid[0:H, 0:W]
    boxes = [(28 + 48 * (i % 5), 28 + 45 * (i // 5), 16, 5, -1.45 + 0.15 * i) for i in range(20)]
    boxes += [(2, 100, 14, 5, 0.35), (253, 139, 10, 4, -0.4), (148, 1, 5, 13, 0.3), (148, 190, 5, 12, -0.35)]
    N_ROT_RECTS[0] = len(boxes)
    for cx, cy, a, b, t in boxes:
        u = (xx - cx) * np.cos(t) + (yy - cy) * np.sin(t)
        v = -(xx - cx) * np.sin(t) + (yy - cy) * np.cos(t)
        m = (np.abs(u) <= a) & (np.abs(v) <= b)
        f[m] = _level(rs, m)
    return f


def _nested():
    """holes with components inside, single pixels, one-pixel lines, diagonal staircases, blobs around the size gates"""
    H, W = 96, 160
    rs = np.random.RandomState(12)
    f = np.full((H, W), 0.25, np.float32)
    bm = np.zeros((H, W), bool)
    bm[6:50, 6:70] = True       # a ring ...
    bm[12:44, 12:64] = False
    bm[18:38, 18:58] = True     # ... a ring inside its hole ...
    bm[23:33, 24:52] = False
    bm[26:30, 30:46] = True     # ... and a blob inside that one's hole
    bm[60, 8] = bm[64, 12] = bm[70, 5] = True                 # single pixels: borders of one vertex
    bm[58, 20:40] = True                                      # one-pixel lines: borders of two vertices
    bm[62:80, 44] = True
    for i in range(14):
        bm[60 + i, 50 + i] = True                             # a pure diagonal: 8-connected only, two vertices
    for i in range(10):
        bm[60 + i, 70 + 2 * i:72 + 2 * i] = True              # a staircase of 2-pixel treads, corners touching diagonally
    for i in range(9):
        bm[84 - i, 100 + i] = True                            # an anti-diagonal joined to ...
    bm[84, 90:101] = True                                     # ... a line: one 8-connected component, more than 2 vertices
    x = 80
    for (h, w) in ((2, 2), (3, 3), (3, 4), (4, 4), (2, 4), (2, 5), (3, 5), (4, 6), (5, 5), (2, 7), (3, 8)):
        bm[8:8 + h, x:x + w] = True                           # minAreaRect sides h-1, w-1: ssid on both sides of 3 and,
        x += w + 3                                            # after UnClip, of 5
    bm[30:52, 90:150] = True                                  # a block with several holes: hole borders in a row
    bm[34:40, 95:105] = bm[34:48, 110:118] = bm[42:48, 125:145] = False
    lab = np.zeros((H, W), np.float32)
    lab[bm] = _level(rs, bm)
    lab[8:14, 80:160][bm[8:14, 80:160]] = 0.9                 # the small blobs score high: the size gates decide, not the score
    f[bm] = lab[bm]
    return f


def _comb():
    """a two-sided zigzag comb: one border of more than SORT_LDS_CAP vertices (sorted in global memory), beside ordinary ones;
    one-pixel teeth every third column, so that the 2x2 dilate leaves gaps between them"""
    H, W = 64, 256
    rs = np.random.RandomState(13)
    bm = np.zeros((H, W), bool)
    bm[20:23, 4:252] = True
    bm[17:20, 4:252:3] = True   # teeth up ...
    bm[23:26, 5:252:3] = True   # ... and down
    bm[40:52, 10:60] = True
    bm[44:48, 20:50] = False
    bm[38:56, 100:104] = True
    f = np.full((H, W), 0.25, np.float32)
    f[bm] = _level(rs, bm)
    return f


def _frame():
    """foreground in the first and last row and the first and last column: borders that run along the map's frame"""
    H, W = 48, 80
    rs = np.random.RandomState(14)
    bm = np.zeros((H, W), bool)
    bm[0, :] = bm[-1, :] = bm[:, 0] = bm[:, -1] = True
    bm[0:3, 0:30] = True
    bm[10:30, 10:40] = True
    bm[15:25, 15:35] = False
    bm[18:22, 20:30] = True
    bm[36:48, 50:80] = True     # a block in the corner of the frame
    bm[5:9, 70:79] = True
    f = np.full((H, W), 0.0, np.float32)
    f[bm] = _level(rs, bm)
    return f


EDGE_VALUES = None


def _edges():
    """blocks at k/255 and one float32 step to either side for k around ITHRESH, and at 0.0 and 1.0"""
    global EDGE_VALUES
    vals = []
    for k in range(ITHRESH - 1, ITHRESH + 3):
        v = np.float32(k) / np.float32(255)
        vals += [np.nextafter(v, np.float32(0)), v, np.nextafter(v, np.float32(1))]
    vals += [np.float32(0.0), np.float32(1.0)]
    EDGE_VALUES = np.array(vals, np.float32)
    H, W = 48, 112
    f = np.full((H, W), 0.01, np.float32)
    for i, v in enumerate(vals):
        y, x = 4 + 14 * (i // 5), 4 + 22 * (i % 5)
        f[y:y + 7 + (i % 3), x:x + 12 + (i % 4)] = v
    f[40:46, 70:108] = np.float32(0.5)   # a block exactly at box_thresh
    return f


_MAKERS = dict(rot_rects=_rot_rects, nested=_nested, comb=_comb, frame=_frame, edges=_edges)
NAMES = list(_MAKERS)
_maps = {}


def prob(name):
    if name not in _maps:
        m = np.ascontiguousarray(_MAKERS[name](), dtype=np.float32)
        assert m.shape[0] <= 192 and m.shape[1] <= 256
        m.setflags(write=False)
        _maps[name] = m
    return _maps[name]


# ---------------------------------------------------------------------------------------------------------- references
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ulp_apart(a, b):
    """distance in float32 steps between two finite floats of one sign"""
    return abs(int(bits(np.float32(a)).reshape(())) - int(bits(np.float32(b)).reshape(())))


def _clamp(v, lo, hi):
    return hi if v > hi else (lo if v < lo else v)


def fast_mask_geometry(corners, H, W):
    """BoxScoreFast: the clamped bounding box of the float corners and the int-truncated corners relative to it"""
    xs, ys = corners[:, 0], corners[:, 1]
    xmin, xmax = _clamp(int(math.floor(xs.min())), 0, W - 1), _clamp(int(math.ceil(xs.max())), 0, W - 1)
    ymin, ymax = _clamp(int(math.floor(ys.min())), 0, H - 1), _clamp(int(math.ceil(ys.max())), 0, H - 1)
    local = np.stack([xs.astype(np.int32) - xmin, ys.astype(np.int32) - ymin], 1).astype(np.int32)  # astype: truncation, as (int)
    return xmin, ymin, xmax, ymax, local


def slow_mask_geometry(contour, H, W):
    """PolygonScoreAcc: the clamped bounding box of the contour and the contour relative to it"""
    xmin, xmax = _clamp(int(contour[:, 0].min()), 0, W - 1), _clamp(int(contour[:, 0].max()), 0, W - 1)
    ymin, ymax = _clamp(int(contour[:, 1].min()), 0, H - 1), _clamp(int(contour[:, 1].max()), 0, H - 1)
    return xmin, ymin, xmax, ymax, (contour - np.array([xmin, ymin], np.int32)).astype(np.int32)


def exact_score(pred, geom, O, compat, outline=True, masked=True):
    """(pixel count of the fillPoly mask, float32(fsum(pred[mask]) / count)): the mean exactly summed"""
    xmin, ymin, xmax, ymax, local = geom
    mask = O.fill_poly(local, xmax - xmin + 1, ymax - ymin + 1, compat, outline=outline).astype(bool)
    if not masked:
        mask = np.ones_like(mask)
    vals = pred[ymin:ymax + 1, xmin:xmax + 1][mask]
    cnt = int(mask.sum())
    return cnt, np.float32(math.fsum(float(v) for v in vals) / cnt) if cnt else np.float32(0)


_ref = {}


def borders(name, dil, O):
    """bitmap, contours and their start pixels, and per contour of more than two vertices (corners, ssid, raw corners)"""
    key = ("b", name, dil)
    if key not in _ref:
        bm = O.bitmap(prob(name), THRESH, dil)
        cs, starts = O.contours(bm)
        mini = [O.mini_box(c) if len(c) > 2 else None for c in cs]
        _ref[key] = dict(bitmap=bm, contours=cs, starts=starts, mini=mini)
    return _ref[key]


def scores(name, cfg, O, **mut):
    """per contour None (not scored: <= 2 vertices or ssid < 3) or (cnt, exact score) under cfg's mode and fill rule"""
    mode, compat, dil = cfg
    key = ("s", name, cfg, tuple(sorted(mut.items())))
    if key not in _ref:
        b = borders(name, dil, O)
        p = prob(name)
        H, W = p.shape
        compat = {45: 410, 410: 45}[compat] if mut.pop("other_rule", False) else compat
        out = []
        for c, m in zip(b["contours"], b["mini"]):
            if m is None or m[1] < 3:
                out.append(None)
                continue
            geom = slow_mask_geometry(c, H, W) if mode == "slow" else fast_mask_geometry(m[0], H, W)
            out.append(exact_score(p, geom, O, compat, **mut))
        _ref[key] = out
    return _ref[key]


def kept(name, cfg, O):
    """(boxes, contour index of each) the whole oracle keeps"""
    mode, compat, dil = cfg
    key = ("k", name, cfg)
    if key not in _ref:
        p = prob(name)
        _ref[key] = O.det_post_candidates(p, THRESH, BOX_THRESH, UNCLIP, p.shape[0], p.shape[1], use_dilation=dil,
                                          slow=mode == "slow", cv_compat=compat)
    return _ref[key]
