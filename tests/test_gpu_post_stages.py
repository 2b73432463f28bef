"""The detector's post-processing (csrc/kernels_post.hip) stage by stage: after det.post() on a map of tests/post_cases.py,
ocr_det_post_stages hands out what the production launch sequence left behind - the bitmap, the border starts, the traced
vertices, the per-candidate record border_box_kernel wrote (mini box, ssid, score, mask pixel count) and the gates' outcome -
and every stage is compared with the oracle's (tests/test_post_ref.py proves on the CPU that the cases hold every branch).
Integers and the float chains of minAreaRect / GetMiniBoxes are compared bit for bit; the score within 1 float32 ulp of the
exactly summed mean (the device adds at most 2^16 doubles in [0, 1] in another order: far below half an ulp, so only a
rounding tie can move the result, by one step)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import post_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu

OCR_ERR_ARG, OCR_ERR_CAPACITY = -1, -4
_RUNS = [(name, cfg) for cfg in pc.CONFIGS for name in pc.NAMES]
_IDS = ["%s-%s" % (name, pc.config_id(cfg)) for name, cfg in _RUNS]


@pytest.fixture(scope="module")
def O(built):
    import oracle
    return oracle


@pytest.fixture(scope="module")
def taps(pkg, built):
    """every (case, configuration) once: boxes of det.post() and the stage tap behind it; one handle per configuration"""
    out = {}
    for cfg in pc.CONFIGS:
        mode, compat, dil = cfg
        det = pkg.Det(limit_side_len=960, thresh=pc.THRESH, box_thresh=pc.BOX_THRESH, unclip_ratio=pc.UNCLIP, score_mode=mode,
                      use_dilation=dil, cv_compat=compat)
        assert det.post_stages_raw(0, 0, 0)[0] == OCR_ERR_ARG   # nothing recorded yet; the call arms the tap
        for name in pc.NAMES:
            p = pc.prob(name)
            boxes = det.post(p, p.shape[0], p.shape[1])
            out[(name, cfg)] = (boxes, det.post_stages())
        det.close()
    return out


def _fill(a):
    return pc.bits(a) == 0xFFFFFFFF


@pytest.mark.parametrize("name,cfg", _RUNS, ids=_IDS)
def test_bitmap_and_borders(taps, O, name, cfg):
    mode, compat, dil = cfg
    _, t = taps[(name, cfg)]
    ref = pc.borders(name, dil, O)
    assert np.array_equal(t["bitmap"], ref["bitmap"])
    cs, st = ref["contours"], ref["starts"]
    assert t["ncont_all"] == len(cs) and t["ncont"] == len(cs)
    W = ref["bitmap"].shape[1]
    assert t["starts"].tolist() == [int(y) * W + int(x) + int(h) for x, y, h in st]   # (a hole border starts left of the pixel the scan met)
    assert t["npts"].tolist() == [len(c) for c in cs]
    for i, (c, v) in enumerate(zip(cs, t["verts"])):
        if len(c) <= 2:
            assert v is None
        elif mode == "slow" or len(c) <= pc.SORT_LDS_CAP:
            assert np.array_equal(v, c), "border %d: vertices in contour order" % i
        else:
            assert sorted(map(tuple, v.tolist())) == sorted(map(tuple, c.tolist())), "border %d: vertices as a set" % i


@pytest.mark.parametrize("name,cfg", _RUNS, ids=_IDS)
def test_mini_box(taps, O, name, cfg):
    _, t = taps[(name, cfg)]
    rec = t["record"]
    for i, m in enumerate(pc.borders(name, cfg[2], O)["mini"]):
        if m is None:
            assert _fill(rec[i]).all()
            continue
        assert np.array_equal(pc.bits(rec[i, :8]), pc.bits(m[0].reshape(8))), (i, rec[i, :8], m[0])
        assert pc.bits(rec[i, 8]) == pc.bits(m[1]), (i, rec[i, 8], m[1])
        assert _fill(rec[i, 11])


@pytest.mark.parametrize("name,cfg", _RUNS, ids=_IDS)
def test_score(taps, O, name, cfg):
    _, t = taps[(name, cfg)]
    rec = t["record"]
    for i, s in enumerate(pc.scores(name, cfg, O)):
        if s is None:
            assert _fill(rec[i, 9:11]).all(), i
            continue
        assert not _fill(rec[i, 9:11]).any(), i
        assert rec[i, 10] == s[0], ("cnt", i, rec[i, 10], s[0])
        assert pc.ulp_apart(rec[i, 9], s[1]) <= 1, ("score", i, rec[i, 9], s[1])


@pytest.mark.parametrize("name,cfg", _RUNS, ids=_IDS)
def test_gates(taps, O, name, cfg):
    boxes, t = taps[(name, cfg)]
    want_boxes, want_cand = pc.kept(name, cfg, O)
    assert np.flatnonzero(t["cand_valid"]).tolist() == want_cand.tolist()
    assert set(np.unique(t["cand_valid"]).tolist()) <= {0, 1}
    assert np.array_equal(t["cand_boxes"][t["cand_valid"] != 0], boxes)
    assert np.array_equal(boxes, want_boxes)


def _device_disagrees(taps, O, check, runs=_RUNS):
    return sum(bool(check(taps[r][1], r[0], r[1])) for r in runs)


def test_mutated_references_differ_from_the_device(taps, O):
    """each deliberately wrong reference must be told from the device's values by the comparisons above on at least one case"""
    def score_mut(**mut):
        def check(t, name, cfg):
            return any(s is not None and (t["record"][i, 10] != s[0] or pc.ulp_apart(t["record"][i, 9], s[1]) > 1)
                       for i, s in enumerate(pc.scores(name, cfg, O, **mut)))
        return check

    fast = [r for r in _RUNS if r[1][0] == "fast"]
    # (the other fill rule: fast mode only - on contour polygons the two rules are the same mask, tests/test_post_ref.py)
    assert _device_disagrees(taps, O, score_mut(other_rule=True), fast) >= 1
    assert _device_disagrees(taps, O, score_mut(masked=False)) >= 1
    assert _device_disagrees(taps, O, score_mut(outline=False)) >= 1

    def discovery_order(t, name, cfg):
        cs = pc.borders(name, cfg[2], O)["contours"][::-1]
        return t["npts"].tolist() != [len(c) for c in cs]

    def rotated(t, name, cfg):
        cs = pc.borders(name, cfg[2], O)["contours"]
        return any(v is not None and (cfg[0] == "slow" or len(c) <= pc.SORT_LDS_CAP) and not np.array_equal(v, np.roll(c, 1, axis=0))
                   for c, v in zip(cs, t["verts"]))

    def raw_corners(t, name, cfg):
        return any(m is not None and not np.array_equal(pc.bits(t["record"][i, :8]), pc.bits(m[2].reshape(8)))
                   for i, m in enumerate(pc.borders(name, cfg[2], O)["mini"]))

    assert _device_disagrees(taps, O, discovery_order) >= 1
    assert _device_disagrees(taps, O, rotated) >= 1
    assert _device_disagrees(taps, O, raw_corners) >= 1


def test_refusals_leave_the_handle_usable(pkg, built, O):
    name, cfg = "nested", ("slow", 410, False)
    p = pc.prob(name)
    want = pc.kept(name, cfg, O)[0]
    assert len(want) > 0
    det = pkg.Det(limit_side_len=960, thresh=pc.THRESH, box_thresh=pc.BOX_THRESH, unclip_ratio=pc.UNCLIP, score_mode="slow", cv_compat=410)
    L = pkg.lib()
    assert L.ocr_det_post_stages(None, None) == OCR_ERR_ARG and L.ocr_det_post_stages(det.h, None) == OCR_ERR_ARG
    assert det.post_stages_raw(1 << 16, 1000, 1 << 16)[0] == OCR_ERR_ARG          # before any post call on the handle
    assert np.array_equal(det.post(p, *p.shape), want)
    full = det.post_stages()
    px, nc, nv = p.size, full["ncont"], sum(len(v) for v in full["verts"] if v is not None)
    for caps in ((px - 1, nc, nv), (px, nc - 1, nv), (px, nc, nv - 1)):
        rc, s, _ = det.post_stages_raw(*caps)
        assert rc == OCR_ERR_CAPACITY and (s.rows * s.cols, s.ncont, s.nverts) == (px, nc, nv)   # ... and says what it needs
        assert np.array_equal(det.post(p, *p.shape), want)
    for field in ("bitmap", "starts", "npts", "voff", "verts", "cand_valid", "cand_boxes", "record"):
        assert det.post_stages_raw(px, nc, nv, null=field)[0] == OCR_ERR_ARG, field
    assert np.array_equal(det.post(p, *p.shape), want)
    again = det.post_stages()
    assert all(np.array_equal(full[k], again[k]) for k in ("bitmap", "starts", "npts", "cand_valid", "cand_boxes"))
    assert np.array_equal(pc.bits(full["record"]), pc.bits(again["record"]))
    det.close()
