"""What tests/post_cases.py promises, asserted on the oracle alone (no GPU): every branch the stage tests of
tests/test_gpu_post_stages.py are meant to drive is really in the maps, the references those tests use agree with the oracle's
own scores, and every mutated reference of the sensitivity checks really differs from the true one."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import post_cases as pc  # noqa: E402


@pytest.fixture(scope="module")
def O(built):
    import oracle
    return oracle


def _all(O, dils=(False, True)):
    return [(n, d, pc.borders(n, d, O)) for n in pc.NAMES for d in dils]


def test_maps_are_small_in_contract_and_below_the_candidate_cut(O):
    for name in pc.NAMES:
        p = pc.prob(name)
        assert p.dtype == np.float32 and p.shape[0] <= 192 and p.shape[1] <= 256
        assert np.isfinite(p).all() and p.min() >= 0.0 and p.max() <= 1.0
    for name, dil, b in _all(O):
        assert 0 < len(b["contours"]) < 1000, (name, dil)


def test_rotated_rectangles_at_many_angles_and_through_all_four_edges(O):
    b = pc.borders("rot_rects", False, O)
    H, W = pc.prob("rot_rects").shape
    angles = set()
    out = dict(left=0, right=0, top=0, bottom=0)
    for m in b["mini"]:
        c = m[0]
        e = c[1] - c[0]
        angles.add(round(math.degrees(math.atan2(e[1], e[0])) / 5))
        # an int-truncated corner outside the clamped bounding box: the mask's bounding box clips, and the 4.5.2 rule
        # builds that edge from the clipped end points
        xmin, ymin, xmax, ymax, local = pc.fast_mask_geometry(c, H, W)
        out["left"] += (local[:, 0] < 0).any()
        out["top"] += (local[:, 1] < 0).any()
        out["right"] += (local[:, 0] > xmax - xmin).any()
        out["bottom"] += (local[:, 1] > ymax - ymin).any()
    assert len(angles) >= 12, angles
    assert all(len(pc.borders("rot_rects", d, O)["contours"]) == pc.N_ROT_RECTS[0] == 24 for d in (False, True))  # none merged
    assert all(v >= 1 for v in out.values()), out


def test_holes_that_contain_components_and_the_order_of_contours(O):
    for dil in (False, True):
        b = pc.borders("nested", dil, O)
        cs, st = b["contours"], b["starts"]
        assert st[:, 2].sum() >= 4
        box = [(c[:, 0].min(), c[:, 1].min(), c[:, 0].max(), c[:, 1].max()) for c in cs]
        inside = [(i, j) for i in range(len(cs)) if st[i, 2] for j in range(len(cs)) if not st[j, 2] and
                  box[i][0] < box[j][0] and box[i][1] < box[j][1] and box[i][2] > box[j][2] and box[i][3] > box[j][3]]
        assert inside, "no outer border inside a hole border"
        # the reference's order is the reverse of the raster scan's discovery order: start pixels descend
        key = [(int(y), int(x) + int(h)) for x, y, h in st]
        assert key == sorted(key, reverse=True) and len(set(key)) == len(key)
        # the start is the scan's own knowledge: the first stored vertex of every border is the pixel it started on
        assert all((c[0] == s[:2]).all() for c, s in zip(cs, st))


def test_short_borders_diagonals_and_both_sides_of_the_size_gates(O):
    from scipy import ndimage
    b = pc.borders("nested", False, O)
    sizes = [len(c) for c in b["contours"]]
    assert sizes.count(1) >= 3 and sizes.count(2) >= 3          # dropped by `size() <= 2`
    _, n8 = ndimage.label(b["bitmap"], structure=np.ones((3, 3)))
    _, n4 = ndimage.label(b["bitmap"])
    assert n8 == int((b["starts"][:, 2] == 0).sum()) and n4 >= n8 + 20   # components that hold together by diagonals only
    ssid = [m[1] for m in b["mini"] if m is not None]
    assert sum(s < 3 for s in ssid) >= 2 and sum(s >= 3 for s in ssid) >= 2
    assert any(2.5 <= s < 3 for s in ssid) or any(s == 2 for s in ssid)
    after = [O.unclip_box(m[0], pc.UNCLIP)[1] for m in b["mini"] if m is not None and m[1] >= 3]
    assert sum(s < 5 for s in after) >= 2 and sum(s >= 5 for s in after) >= 2, after
    # ... and some of those that UnClip leaves below 5 did pass the score gate, so the gate is what drops them
    for cfg in pc.CONFIGS:
        if cfg[2]:
            continue
        sc = pc.scores("nested", cfg, O)
        kept = set(pc.kept("nested", cfg, O)[1].tolist())
        small = [i for i, m in enumerate(b["mini"]) if m is not None and m[1] >= 3 and sc[i][1] >= np.float32(pc.BOX_THRESH)
                 and O.unclip_box(m[0], pc.UNCLIP)[1] < 5]
        assert small and not (set(small) & kept)


@pytest.mark.parametrize("dil", [False, True])
def test_a_border_longer_than_the_lds_sort(O, dil):
    sizes = [len(c) for c in pc.borders("comb", dil, O)["contours"]]
    assert max(sizes) > pc.SORT_LDS_CAP and max(sizes) <= 1024   # pow2_ceil(npts) = 1024 > SORT_LDS_CAP
    assert sum(s > pc.SORT_LDS_CAP for s in sizes) == 1 and sum(2 < s <= pc.SORT_LDS_CAP for s in sizes) >= 2


def test_foreground_on_all_four_frame_lines(O):
    for dil in (False, True):
        bm = pc.borders("frame", dil, O)["bitmap"]
        assert bm[0].any() and bm[-1].any() and bm[:, 0].any() and bm[:, -1].any()
    b = pc.borders("frame", False, O)
    H, W = b["bitmap"].shape
    c = max(b["contours"], key=len)
    assert c[:, 0].min() == 0 and c[:, 1].min() == 0 and c[:, 0].max() == W - 1 and c[:, 1].max() == H - 1


def test_bitmap_edge_values(O):
    p = pc.prob("edges")
    bm = pc.borders("edges", False, O)["bitmap"]
    vals = pc.EDGE_VALUES
    want = set()
    for k in range(pc.ITHRESH - 1, pc.ITHRESH + 3):
        v = np.float32(k) / np.float32(255)
        want |= {float(np.nextafter(v, np.float32(0))), float(v), float(np.nextafter(v, np.float32(1)))}
    assert want | {0.0, 1.0} == set(float(v) for v in vals)
    seen = set()
    for v in vals:
        m = p == v
        assert m.any()
        bit = int(int(np.float32(v) * np.float32(255)) > pc.ITHRESH)   # trunc(p * 255) > floor(thresh * 255), in float32
        assert (bm[m] == bit).all(), float(v)
        seen.add((bit, float(v) >= float(np.float32(pc.ITHRESH + 1) / np.float32(255))))
    # both outcomes, and a value whose float32 product lands on the other side of where its real value lies
    assert {b for b, _ in seen} == {0, 1}
    below = np.nextafter(np.float32(pc.ITHRESH + 1) / np.float32(255), np.float32(0))
    assert (bm[p == below] == 0).all() and (bm[p == np.float32(pc.ITHRESH + 1) / np.float32(255)] == 1).all()


@pytest.mark.parametrize("cfg", pc.CONFIGS, ids=pc.config_id)
def test_the_oracles_own_scores_meet_the_bound_of_the_stage_test(O, cfg):
    """score within 1 float32 ulp of float32(fsum(pred[mask]) / cnt): at most 2^16 doubles in [0, 1] summed in any order differ
    from the exact sum by far less than half a float32 ulp of the mean, so only a rounding tie can move the result, by one step"""
    mode, compat, dil = cfg
    on_both_sides = [0, 0]
    for name in pc.NAMES:
        p = pc.prob(name)
        b = pc.borders(name, dil, O)
        for c, m, s in zip(b["contours"], b["mini"], pc.scores(name, cfg, O)):
            if s is None:
                continue
            got = O.polygon_score(c, p, compat) if mode == "slow" else O.box_score_fast(m[0], p, compat)
            assert s[0] > 0 and pc.ulp_apart(got, s[1]) <= 1, (name, got, s)
            on_both_sides[int(s[1] >= np.float32(pc.BOX_THRESH))] += 1
    assert min(on_both_sides) >= 5, on_both_sides


@pytest.mark.parametrize("mode", ["fast", "slow"])
def test_where_the_two_fill_rules_count_different_masks(O, mode):
    """BoxScoreFast fills a rotated quadrilateral: the rules differ at the span ends.  PolygonScoreAcc fills a
    CHAIN_APPROX_SIMPLE contour, whose edges run in the 8 chain directions between points inside the map: every scanline
    crossing is then a whole number, where [ceil(x), floor(x)] and [floor(x + 1/2), floor(x + 1/2)] are the same span, and no
    edge is clipped - the two rules MUST give the same mask in slow mode (so cv_compat cannot change a slow-mode result)."""
    for dil in (False, True):
        differ = 0
        for name in pc.NAMES:
            a, b = pc.scores(name, (mode, 45, dil), O), pc.scores(name, (mode, 410, dil), O)
            differ += sum(x is not None and x != y for x, y in zip(a, b))
        assert (differ >= 5) if mode == "fast" else (differ == 0), (mode, dil, differ)


@pytest.mark.parametrize("cfg", pc.CONFIGS, ids=pc.config_id)
def test_every_mutated_reference_differs_from_the_true_one(O, cfg):
    mode, compat, dil = cfg
    diff = dict(other_rule=0, unmasked=0, no_outline=0, discovery_order=0, rotated=0, raw_corners=0)
    for name in pc.NAMES:
        b = pc.borders(name, dil, O)
        true = pc.scores(name, cfg, O)
        for key, mut in (("other_rule", dict(other_rule=True)), ("unmasked", dict(masked=False)), ("no_outline", dict(outline=False))):
            for t, m in zip(true, pc.scores(name, cfg, O, **mut)):
                if t is not None:
                    diff[key] += t[0] != m[0] or pc.ulp_apart(t[1], m[1]) > 1
        diff["discovery_order"] += [len(c) for c in b["contours"]] != [len(c) for c in b["contours"][::-1]]
        diff["rotated"] += sum(len(c) > 2 and not np.array_equal(c, np.roll(c, 1, axis=0)) for c in b["contours"])
        diff["raw_corners"] += sum(m is not None and not np.array_equal(pc.bits(m[0]), pc.bits(m[2])) for m in b["mini"])
    if mode == "slow":  # (the rules coincide on contour polygons: test_where_the_two_fill_rules_count_different_masks)
        assert diff.pop("other_rule") == 0
    assert all(v >= 1 for v in diff.values()), diff


def test_kept_candidates_are_what_det_post_returns(O):
    for name in pc.NAMES:
        p = pc.prob(name)
        for cfg in pc.CONFIGS:
            mode, compat, dil = cfg
            boxes, cand = pc.kept(name, cfg, O)
            want = O.det_post(p, pc.THRESH, pc.BOX_THRESH, pc.UNCLIP, p.shape[0], p.shape[1], use_dilation=dil, slow=mode == "slow",
                              cv_compat=compat)
            assert np.array_equal(boxes, want) and list(cand) == sorted(set(cand.tolist()))
            sc, mini = pc.scores(name, cfg, O), pc.borders(name, dil, O)["mini"]
            assert all(sc[i] is not None and sc[i][1] >= np.float32(pc.BOX_THRESH) for i in cand)
    assert sum(len(pc.kept(n, c, O)[0]) for n in pc.NAMES for c in pc.CONFIGS) >= 40
