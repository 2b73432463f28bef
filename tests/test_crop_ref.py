"""tools/crop_ref.py, the plain restatement of the crop geometry between detector and recognizer, against the oracle library (the
committed restatement of the reference's OpenCV path) on every case of tests/crop_cases.py the oracle can express - byte for
byte - and against the library's own host arithmetic: the plan of csrc/crop.h bit for bit (ocr_selftest_crop_plan), the
grouping of csrc/rot_groups.h by its properties (ocr_selftest_rotation_groups).  That equality is what lets
tests/test_gpu_crop_ops.py compare the device with crop_ref and carry its mutations.  The launches with a caller-given inverse
matrix (W == 0, saturation, NaN, the block seams) have no oracle entry point - the oracle inverts a forward matrix itself - and
rest on crop_ref alone; every claim a case makes about itself is asserted here."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crop_cases as cc  # noqa: E402

import crop_ref as R  # noqa: E402  (tools/ is on the path: conftest.py)


@pytest.fixture(scope="module")
def O(built):
    import oracle
    return oracle


def _oracle_warp(O, src, M, dh, dw):
    src = np.ascontiguousarray(src)
    M = np.ascontiguousarray(M, dtype=np.float64)
    out = np.zeros((dh, dw, 3), np.uint8)
    O.lib().oracle_warp_perspective(C.c_void_p(src.ctypes.data), src.shape[0], src.shape[1], C.c_size_t(src.strides[0]),
                                    C.c_void_p(M.ctypes.data), C.c_void_p(out.ctypes.data), dh, dw)
    return out


_ref = {}


def _warp_ref(name, mut=()):
    """the outputs of a launch's crops by crop_ref (computed once per (launch, mutation))"""
    key = (name, tuple(mut))
    if key not in _ref:
        L = cc.WARP_BY_NAME[name]
        _ref[key] = [R.warp(cc.crop_source(c), c["m"], c["dw"], c["dh"], c["rot"], c["bw0"], mut) for c in L["crops"]]
    return _ref[key]


# --------------------------------------------------------------------------------------------------------------- plan
@pytest.mark.parametrize("name", list(cc.PLAN_QUADS))
def test_plan_equals_the_library_bit_for_bit_and_the_oracle(O, pkg, name):
    q = cc.PLAN_QUADS[name]
    p = R.plan(cc.PLAN_ROWS, cc.PLAN_COLS, q)
    got = pkg.selftest_crop_plan(cc.PLAN_ROWS, cc.PLAN_COLS, q)
    for k in pkg.CROP_PLAN_FIELDS:
        assert got[k] == p[k], k
    assert np.array_equal(R.bits64(got["minv"]), R.bits64(p["minv"])), (got["minv"], p["minv"])
    assert pkg.rotate_crop_shape(cc.PLAN_ROWS, cc.PLAN_COLS, q) == (p["orows"], p["ocols"])
    if name in cc.PLAN_SHAPES:
        assert (p["dw"], p["dh"], p["rot"]) == cc.PLAN_SHAPES[name]
    if name in ("collinear", "zero_width"):
        assert np.array_equal(R.bits64(p["minv"]), R.bits64([0.0] * 9)), "the singular solve"
    else:
        assert any(v != 0 for v in p["minv"])
    for kind in ("rand", "ramp"):
        img = cc.plan_image(kind)
        want = O.rotate_crop(img, q)
        got_img = R.rotate_crop(img, q)
        assert want.shape == got_img.shape == (p["orows"], p["ocols"], 3)
        assert np.array_equal(got_img, want)
        if name in ("collinear", "zero_width"):
            assert (got_img == img[p["top"], p["left"]]).all(), "every pixel is source pixel (0, 0)"
    # the oracle's own inverse of the forward matrix is the plan's, so the given-minv path and the forward path meet
    img = cc.plan_image()
    src = img[p["top"]:p["top"] + p["sh"], p["left"]:p["left"] + p["sw"]]
    assert np.array_equal(R.warp(src, p["minv"], p["dw"], p["dh"], 0, p["bw0"]), _oracle_warp(O, src, p["fwd"], p["dh"], p["dw"]))


@pytest.mark.parametrize("name", list(cc.PLAN_REFUSED))
def test_refused_boxes(O, pkg, name):
    q = cc.PLAN_REFUSED[name]
    assert R.plan(cc.PLAN_ROWS, cc.PLAN_COLS, q) is None
    assert O.rotate_crop(cc.plan_image(), q) is None
    with pytest.raises(pkg.OcrError, match="no crop inside"):
        pkg.selftest_crop_plan(cc.PLAN_ROWS, cc.PLAN_COLS, q)
    assert pkg.selftest_crop_plan(cc.PLAN_ROWS, cc.PLAN_COLS, cc.PLAN_QUADS["sides_3_4_5"])["dw"] == 5


def test_block_width_at_its_thresholds():
    for (dw, dh), want in {(63, 16): 63, (64, 16): 64, (65, 16): 64, (129, 16): 64, (342, 3): 341, (1025, 1): 1024, (1024, 1): 1024,
                           (341, 3): 341, (500, 17): 64, (5, 4): 5}.items():
        assert R.block_width(dw, dh) == cc.block_width(dw, dh) == want


def test_plan_block_width_of_long_boxes(pkg):
    for dw, dh in ((65, 16), (342, 3), (1025, 1), (341, 3), (64, 15)):
        q = [[0, 0], [dw, 0], [dw, dh], [0, dh]]
        p, got = R.plan(dh, dw, q), pkg.selftest_crop_plan(dh, dw, q)
        assert (got["dw"], got["dh"], got["bw0"]) == (dw, dh, R.block_width(dw, dh)) == (p["dw"], p["dh"], p["bw0"])
        assert np.array_equal(R.bits64(got["minv"]), R.bits64(p["minv"]))


# --------------------------------------------------------------------------------------------------------------- warp
@pytest.mark.parametrize("name,kind,sw,sh,dw,dh,M", cc.FORWARD, ids=[f[0] for f in cc.FORWARD])
def test_warp_equals_the_oracle_on_forward_matrices(O, name, kind, sw, sh, dw, dh, M):
    """the oracle inverts M with the same closed form, so crop_ref.inverse3(M) is the matrix it warps with"""
    src = cc.image(kind, sh, sw, seed=9)
    minv = R.inverse3([float(v) for v in M])
    assert np.array_equal(R.warp(src, minv, dw, dh, 0, R.block_width(dw, dh)), _oracle_warp(O, src, M, dh, dw))


@pytest.mark.parametrize("name", [n for n in cc.WARP_BY_NAME if n.startswith(("identity", "trans_", "shift_", "neg_frac", "tie_"))])
def test_affine_cases_equal_the_oracle(O, name):
    """[1 0 tx; 0 1 ty; 0 0 1] with dyadic tx, ty: the inverse of the forward matrix [1 0 -tx; 0 1 -ty; 0 0 1] is exact"""
    (c,) = cc.WARP_BY_NAME[name]["crops"]
    fwd = [1, 0, -c["m"][2], 0, 1, -c["m"][5], 0, 0, 1]
    assert R.inverse3([float(v) for v in fwd]) == c["m"]   # (up to the sign of its zeros, which no rounding to an integer sees)
    assert np.array_equal(_warp_ref(name)[0], _oracle_warp(O, cc.crop_source(c), fwd, c["dh"], c["dw"]))
    if name.startswith("identity"):
        assert np.array_equal(_warp_ref(name)[0], cc.crop_source(c))


def test_what_the_edge_cases_claim():
    for t in ("_5x4", "_7x3"):
        (c,) = cc.WARP_BY_NAME["w_zero" + t]["crops"]
        src = cc.crop_source(c)
        assert R.source_point(c["m"], 3, 1, c["bw0"]) == (0, 0) and (_warp_ref("w_zero" + t)[0][:, 3] == src[0, 0]).all() and src[0, 0].any()
        for n, want in (("sat_pos", (2 ** 31 - 1, 2 ** 31 - 1)), ("sat_neg", (-2 ** 31, -2 ** 31)), ("sat_mixed", (2 ** 31 - 1, -2 ** 31))):
            (c,) = cc.WARP_BY_NAME[n + t]["crops"]
            assert all(R.source_point(c["m"], x, y, c["bw0"]) == want for x in range(c["dw"]) for y in range(c["dh"])), n
            assert not _warp_ref(n + t)[0].any()
        (c,) = cc.WARP_BY_NAME["nan" + t]["crops"]
        assert 32.0 / c["m"][8] == float("inf") and c["m"][0] * 0 + c["m"][1] * 0 + c["m"][2] == 0.0
        assert R.source_point(c["m"], 0, 0, c["bw0"])[0] == 2 ** 31 - 1                      # 0 * inf: NaN resolves to INT_MAX
        assert R.source_point(c["m"], 0, 0, c["bw0"], ("nan_int_min",))[0] == -2 ** 31
        (c,) = cc.WARP_BY_NAME["neg_frac" + t]["crops"]
        X, Y = R.source_point(c["m"], 0, 0, c["bw0"])
        assert (X, Y, X >> 5, X & 31, Y >> 5, Y & 31) == (-11, -5, -1, 21, -1, 27)
        (c,) = cc.WARP_BY_NAME["tie_1_64" + t]["crops"]
        assert R.source_point(c["m"], 1, 1, c["bw0"]) == (32, 32) and R.source_point(c["m"], 1, 1, c["bw0"], ("round_half_away",)) == (33, 33)
        (c,) = cc.WARP_BY_NAME["tie_m1_64" + t]["crops"]
        assert R.source_point(c["m"], 0, 0, c["bw0"]) == (0, -2)
        for tag, sx in (("m2", -2), ("m1", -1), ("swm1", c["sw"] - 1), ("sw", c["sw"])):
            (s,) = cc.WARP_BY_NAME["shift_x_%s%s" % (tag, t)]["crops"]
            X, _ = R.source_point(s["m"], 0, 0, s["bw0"])
            assert (X >> 5, X & 31) == (sx, 11)
        for tag, sy in (("m2", -2), ("m1", -1), ("shm1", c["sh"] - 1), ("sh", c["sh"])):
            (s,) = cc.WARP_BY_NAME["shift_y_%s%s" % (tag, t)]["crops"]
            _, Y = R.source_point(s["m"], 0, 0, s["bw0"])
            assert (Y >> 5, Y & 31) == (sy, 21)


@pytest.mark.parametrize("dw,dh", cc.SEAMS)
def test_seam_cases_tell_the_block_rule_from_its_neighbours(dw, dh):
    """block base + offset against the direct evaluation; at dh = 1 the two are the same function (crop_cases.SEAM_OTHER has the
    argument) and the case tells the 1024-column block from the 64-column one instead"""
    name = "seam_%dx%d" % (dh, dw)
    (c,) = cc.WARP_BY_NAME[name]["crops"]
    other = cc.SEAM_OTHER.get((dw, dh), 1)
    m, (xt, yt), exact = cc.seam_matrix(dw, dh, other)
    assert m is not None and m == c["m"] and m[6] != 0 and c["bw0"] == R.block_width(dw, dh)
    mut = ("direct",) if other == 1 else ("block_64",)
    want, wrong = _warp_ref(name)[0], _warp_ref(name, mut)[0]
    assert not np.array_equal(want, wrong)
    src = cc.crop_source(c)
    zero, origin = (want, wrong) if exact == other else (wrong, want)   # W a rounding residue: saturated; W == 0: source pixel (0, 0)
    assert src[0, 0].any() and not zero[yt, xt].any() and (origin[yt, xt] == src[0, 0]).all()
    if dh == 1:
        assert np.array_equal(want, _warp_ref(name, ("direct",))[0]), "y = 0: the block base changes nothing"
    inside = (want.reshape(-1, 3) != 0).any(-1).mean()
    assert inside > 0.5, "most of the crop reads the source"
    assert len({tuple(p) for p in want.reshape(-1, 3)}) > 20


def test_launch_layouts():
    for L in cc.WARP_LAUNCHES:
        src, size, out_off, out_bytes = cc.warp_layout(L)
        a, b = cc.warp_buffer(L, 0), cc.warp_buffer(L, 255)
        assert a.size == b.size == size
        for c, (first, stride) in zip(L["crops"], src):
            assert first + (c["sh"] - 1) * stride + 3 * c["sw"] <= size - cc.TAIL
            view = np.lib.stride_tricks.as_strided(a[first:], (c["sh"], 3 * c["sw"]), (stride, 1)).reshape(c["sh"], c["sw"], 3)
            assert np.array_equal(view, cc.crop_source(c))
        assert (a != b).sum() == size - sum(3 * c["sw"] * c["sh"] for c in L["crops"])
        assert out_off[-1] + 3 * L["crops"][-1]["dw"] * L["crops"][-1]["dh"] + cc.OUT_TAIL == out_bytes
    three = cc.WARP_BY_NAME["three_crops"]
    assert [c["dw"] * c["dh"] for c in three["crops"]] == [1, 300, 257] and three["max_pixels"] == 300
    odd = cc.warp_layout(cc.WARP_BY_NAME["strided_odd_offset"])[0][0]
    assert odd[0] & 1 and odd[1] > 15


# ------------------------------------------------------------------------------------------------------------- rotate
@pytest.mark.parametrize("name", [c["name"] for c in cc.ROT_ALL])
def test_rotation_cases_equal_the_oracle(O, name):
    c = cc.ROT_BY_NAME[name]
    stride, size = cc.rot_geometry(c)
    buf = cc.rot_buffer(c)
    assert buf.size == size
    want = buf.copy()
    view = np.lib.stride_tricks.as_strided(want[c["view_off"]:], (c["rows"], c["cols"], 3), (stride, 3, 1))
    for off, st, x, y, w, h in cc.rot_applied(c):
        assert (off, st) == (c["view_off"], stride) and x + w <= c["cols"] and y + h <= c["rows"]
        O.rotate180_inplace(view[y:y + h, x:x + w])
    got = R.rotate180(buf, cc.rot_applied(c))
    assert np.array_equal(got, want)
    if not cc.rot_applied(c):
        assert np.array_equal(got, buf)
    elif name in ("same_roi_twice", "rot_1x1"):
        assert np.array_equal(got, buf)
    else:
        assert not np.array_equal(got, buf)


def test_rotation_shapes_cover_what_the_issue_asks():
    ws, hs = {}, {}
    for c in cc.ROT_CASES:
        x, y, w, h = c["rois"][0]
        assert x == 1 and y == 1
        ws.setdefault(w, set()).add(h & 1)
        hs.setdefault(h, set()).add(w & 1)
    assert set(ws) == set(cc.ROT_WS) and set(hs) == set(cc.ROT_HS)
    assert all(v == {0, 1} for v in ws.values()) and all(v == {0, 1} for v in hs.values())
    assert any(c["stride_extra"] for c in cc.ROT_CASES)
    assert max(cc.rot_geometry(c)[1] for c in cc.ROT_ALL) <= 1030 * 36 * 3


def test_the_chain_depends_on_its_order():
    c = cc.ROT_BY_NAME["chain"]
    a, b, d = c["rois"]
    assert R.intersects(a, b) and R.intersects(b, d) and not R.intersects(a, d)
    buf = cc.rot_buffer(c)
    assert not np.array_equal(R.rotate180(buf, cc.rot_rows(c)), R.rotate180(buf, cc.rot_rows(c)[::-1]))
    assert np.array_equal(R.rotate180(buf, cc.rot_rows(c)[::-1]), R.rotate180(buf, cc.rot_rows(c), ("rot_reverse_order",)))


# ----------------------------------------------------------------------------------------------------------- grouping
@pytest.mark.parametrize("name", list(cc.GROUPING))
def test_grouping_has_its_properties(pkg, name):
    rects, views = cc.GROUPING[name]
    order, seg = pkg.selftest_rotation_groups(rects, views)
    assert R.grouping_faults(rects, views, order, seg) == []
    if name.startswith("launch_"):
        g = cc.ROT_BY_NAME[name[len("launch_"):]]
        assert order == list(range(len(rects))) and seg == g["seg"], "the segments the device test launches with are the library's"
    if name == "two_views_same_rects":
        assert seg == [0, 3, 6] and order == [0, 1, 4, 2, 3, 5]
    if name == "late_merge":
        assert order == [0, 1, 3, 4, 2] and seg == [0, 4, 5]
    if name == "touching_is_not_intersecting":
        assert seg == [0, 1, 2, 3]
    if name == "one":
        assert (order, seg) == ([0], [0, 1])


def test_the_property_check_sees_wrong_groupings(pkg):
    d = (30, 16, 5, 3)
    rects, views = [cc.A, cc.B, cc.A, cc.B, d, d], [0, 0, 1, 1, 0, 1]   # A B | A' B' | D | D'
    good = ([0, 1, 2, 3, 4, 5], [0, 2, 4, 5, 6])
    assert R.grouping_faults(rects, views, *good) == []
    assert R.grouping_faults(rects, views, [0, 1, 4, 2, 3, 5], [0, 3, 5, 6]) == ["every group is connected"]          # two disjoint ROIs in one group
    assert R.grouping_faults(rects, views, [0, 1, 2, 3, 4, 5], [0, 1, 2, 4, 5, 6]) == ["intersecting ROIs of one view share a group"]  # a split chain
    assert "one view per group" in R.grouping_faults(rects, views, [0, 1, 2, 3, 4, 5], [0, 4, 5, 6])
    assert R.grouping_faults(rects, views, [1, 0, 2, 3, 4, 5], [0, 2, 4, 5, 6]) == ["request order inside a group"]
    assert R.grouping_faults(rects, views, [2, 3, 0, 1, 4, 5], [0, 2, 4, 5, 6]) == ["groups ordered by their first ROI"]
    assert R.grouping_faults(rects, views, [0, 1, 2, 3, 4, 4], [0, 2, 4, 5, 6]) == ["partition"]
    assert R.grouping_faults(rects, views, [0, 1, 2, 3, 4, 5], [0, 2, 2, 5, 6]) == ["partition"]
    with pytest.raises(pkg.OcrError, match="count out of range"):
        pkg.selftest_rotation_groups([], [])
    assert pkg.selftest_rotation_groups([(3, 4, 5, 6)], [7]) == ([0], [0, 1])


# -------------------------------------------------------------------------------------------------------------- teeth
def _rot_ref(name, mut=()):
    c = cc.ROT_BY_NAME[name]
    return R.rotate180(cc.rot_buffer(c), cc.rot_applied(c), mut)


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_every_mutation_is_killed_by_its_named_case(mut):
    """crop_cases.KILLED_BY names the case.  The EQUIVALENT ones change no result wherever their rule is reached
    (crop_cases.REACHED_BY), which is asserted instead."""
    assert set(cc.KILLED_BY) == set(R.MUTATIONS)
    if cc.KILLED_BY[mut] is None:
        assert mut in R.EQUIVALENT and cc.REACHED_BY[mut]
        for name in cc.REACHED_BY[mut]:
            if name in cc.WARP_BY_NAME:
                assert all(np.array_equal(a, b) for a, b in zip(_warp_ref(name), _warp_ref(name, (mut,))))
            else:
                assert np.array_equal(_rot_ref(name), _rot_ref(name, (mut,)))
        return
    assert mut not in R.EQUIVALENT
    fam, name = cc.KILLED_BY[mut]
    if fam == "warp":
        assert any(not np.array_equal(a, b) for a, b in zip(_warp_ref(name), _warp_ref(name, (mut,))))
    else:
        assert not np.array_equal(_rot_ref(name), _rot_ref(name, (mut,)))
