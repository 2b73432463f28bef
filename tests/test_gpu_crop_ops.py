"""The crop geometry between detector and recognizer alone: warp_crop_kernel through ocr_selftest_warp_crops (the caller gives the
matrix, the column block and the grid size), rotate180_groups_kernel through ocr_selftest_rotate180_groups (the caller gives the
segments), and ocr_rotate_crop on the boxes of tests/crop_cases.py, at every branch and edge.  Every comparison is byte for byte
against tools/crop_ref.py, which tests/test_crop_ref.py proves equal to the oracle library wherever the oracle can express the
case.  Every warp launch also checks that the output bytes no crop owns and the guard behind the output still hold the fill
pattern and that the source bytes outside the crops (0, then 255) do not reach the result; every rotation compares the whole
buffer, bytes outside the ROIs included."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crop_cases as cc  # noqa: E402

import crop_ref as R  # noqa: E402  (tools/ is on the path: conftest.py)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(pkg, built):
    pkg.check(pkg.lib().ocr_rt_init(0))
    assert pkg.SELFTEST_FILL == R.FILL
    return pkg


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype == np.uint8 and a.shape == b.shape and np.array_equal(a, b)


def _untouched(guard):
    return guard.size == 256 and (guard == R.FILL).all()


_cache = {}


def _run_warp(dev, L, outside):
    key = ("warp", L["name"], outside)
    if key not in _cache:
        _, _, out_off, out_bytes = cc.warp_layout(L)
        _cache[key] = dev.selftest_warp_crops(cc.warp_buffer(L, outside), cc.warp_descs(L), L["max_pixels"], out_off, out_bytes)
    return _cache[key]


def _want_warp(L, mut=()):
    """the whole output buffer of a launch by crop_ref: the crops back to back, the fill behind them"""
    _, _, out_off, out_bytes = cc.warp_layout(L)
    want = np.full(out_bytes, R.FILL, np.uint8)
    for c, at in zip(L["crops"], out_off):
        w = R.warp(cc.crop_source(c), c["m"], c["dw"], c["dh"], c["rot"], c["bw0"], mut).reshape(-1)
        want[at:at + w.size] = w
    return want


def _run_rot(dev, c):
    key = ("rot", c["name"])
    if key not in _cache:
        _cache[key] = dev.selftest_rotate180_groups(cc.rot_buffer(c), cc.rot_rows(c), c["seg"])
    return _cache[key]


# --------------------------------------------------------------------------------------------------------------- warp
@pytest.mark.parametrize("name", [L["name"] for L in cc.WARP_LAUNCHES])
def test_warp_launch(dev, name):
    L = cc.WARP_BY_NAME[name]
    want = _want_warp(L)
    (g0, u0), (g1, u1) = _run_warp(dev, L, 0), _run_warp(dev, L, 255)
    _, _, out_off, _ = cc.warp_layout(L)
    for c, at in zip(L["crops"], out_off):
        n = c["dw"] * c["dh"] * 3
        assert _same(g0[at:at + n], want[at:at + n]), (c["dw"], c["dh"], c["rot"])
    assert _same(g0, want), "a byte no crop owns lost the fill"
    assert _same(g1, want), "bytes outside the source crops reach the result"
    assert _untouched(u0) and _untouched(u1), "a write behind the output"


def test_a_grid_smaller_than_a_crop_leaves_its_rest_untouched(dev):
    """max_pixels sizes grid.x: with 256, one workgroup per crop, only the first 256 pixels of the 300-pixel and of the 257-pixel
    crop are written"""
    L = dict(cc.WARP_BY_NAME["three_crops"], max_pixels=256)
    want = _want_warp(L)
    _, _, out_off, out_bytes = cc.warp_layout(L)
    want[out_off[1] + 256 * 3:out_off[2]] = R.FILL
    want[out_off[2] + 256 * 3:out_off[2] + 257 * 3] = R.FILL
    got, guard = dev.selftest_warp_crops(cc.warp_buffer(L, 0), cc.warp_descs(L), 256, out_off, out_bytes)
    assert _same(got, want) and _untouched(guard)


@pytest.mark.parametrize("name", list(cc.PLAN_QUADS))
def test_rotate_crop_of_the_plan_cases(dev, name):
    """ocr_rotate_crop: the plan of csrc/crop.h (tests/test_crop_ref.py has it bit for bit) and the launch as the product makes it"""
    q = np.array(cc.PLAN_QUADS[name], np.int32)
    for kind in ("rand", "ramp"):
        img = cc.plan_image(kind)
        (got,) = dev.rotate_crops(img, [q])
        assert _same(got, R.rotate_crop(img, q))
    wide = np.zeros((cc.PLAN_ROWS, cc.PLAN_COLS + 3, 3), np.uint8) + 0x77
    wide[:, 2:2 + cc.PLAN_COLS] = cc.plan_image()
    (got,) = dev.rotate_crops(wide[:, 2:2 + cc.PLAN_COLS], [q])   # a strided host image
    assert _same(got, R.rotate_crop(cc.plan_image(), q))


def test_rotate_crop_of_all_plan_cases_in_one_call(dev):
    img = cc.plan_image()
    quads = [np.array(q, np.int32) for q in cc.PLAN_QUADS.values()]
    for got, q in zip(dev.rotate_crops(img, quads), quads):
        assert _same(got, R.rotate_crop(img, q))


# ----------------------------------------------------------------------------------------------------------- rotation
@pytest.mark.parametrize("name", [c["name"] for c in cc.ROT_ALL])
def test_rotation_launch(dev, name):
    c = cc.ROT_BY_NAME[name]
    got = _run_rot(dev, c)
    want = R.rotate180(cc.rot_buffer(c), cc.rot_applied(c))
    stride, _ = cc.rot_geometry(c)
    inside = np.zeros(want.size, bool)
    for off, st, x, y, w, h in cc.rot_applied(c):
        for r in range(y, y + h):
            inside[off + r * st + 3 * x:off + r * st + 3 * (x + w)] = True
    assert _same(got[inside], want[inside]), "the ROIs"
    assert _same(got[~inside], cc.rot_buffer(c)[~inside]), "a byte outside the ROIs changed"
    assert _same(got, want)


def test_rotation_through_the_product_api_groups_as_the_launch_cases(dev):
    """ocr_rotate180_rois on the group cases: rot_groups.h chooses the segments itself"""
    for c in cc.ROT_GROUPS:
        if len(c["seg"]) < 2:
            continue
        stride, _ = cc.rot_geometry(c)
        buf = cc.rot_buffer(c)
        view = np.lib.stride_tricks.as_strided(buf[c["view_off"]:], (c["rows"], c["cols"], 3), (stride, 3, 1))
        got = dev.rotate180_rois(view, c["rois"])
        want = R.rotate180(buf, cc.rot_rows(c))
        wview = np.lib.stride_tricks.as_strided(want[c["view_off"]:], (c["rows"], c["cols"], 3), (stride, 3, 1))
        assert _same(got, np.ascontiguousarray(wview)), c["name"]


# -------------------------------------------------------------------------------------------------------------- teeth
@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_mutated_reference_differs_from_the_device(dev, mut):
    """the case tests/crop_cases.KILLED_BY names for the mutation (tests/test_crop_ref.py shows that it changes the reference
    there).  A mutation of crop_ref.EQUIVALENT cannot change any result: for it the device must agree with the mutated reference
    wherever the rule is reached."""
    if cc.KILLED_BY[mut] is None:
        assert mut in R.EQUIVALENT
        for name in cc.REACHED_BY[mut]:
            if name in cc.WARP_BY_NAME:
                assert _same(_run_warp(dev, cc.WARP_BY_NAME[name], 0)[0], _want_warp(cc.WARP_BY_NAME[name], (mut,)))
            else:
                c = cc.ROT_BY_NAME[name]
                assert _same(_run_rot(dev, c), R.rotate180(cc.rot_buffer(c), cc.rot_applied(c), (mut,)))
        return
    fam, name = cc.KILLED_BY[mut]
    if fam == "warp":
        assert not _same(_run_warp(dev, cc.WARP_BY_NAME[name], 0)[0], _want_warp(cc.WARP_BY_NAME[name], (mut,)))
    else:
        c = cc.ROT_BY_NAME[name]
        assert not _same(_run_rot(dev, c), R.rotate180(cc.rot_buffer(c), cc.rot_applied(c), (mut,)))


# ----------------------------------------------------------------------------------------------------------- refusals
def _refused(dev, call):
    with pytest.raises(dev.OcrError, match=r"error -1: \S"):   # OCR_ERR_ARG with a message
        call()


def test_refusals_leave_the_next_call_working(dev):
    """whatever the launchers do not define is refused with OCR_ERR_ARG before it reaches the device"""
    L = cc.WARP_BY_NAME["strided_odd_offset"]
    buf, descs = cc.warp_buffer(L, 0), cc.warp_descs(L)
    _, _, out_off, out_bytes = cc.warp_layout(L)
    want = _want_warp(L)
    ok = lambda d=descs, mp=L["max_pixels"], off=out_off, nb=out_bytes, b=buf: dev.selftest_warp_crops(b, d, mp, off, nb)
    edit = lambda **k: [dict(descs[0], **k)]
    bads = [dict(d=[], off=[]), dict(mp=0), dict(mp=-3), dict(d=edit(bw0=0)), dict(d=edit(rot=2)), dict(d=edit(sw=0)), dict(d=edit(sh=-1)),
            dict(d=edit(dw=0)), dict(d=edit(dh=1 << 20)), dict(d=edit(sstride=14)), dict(d=edit(src_off=buf.size)), dict(d=edit(sh=40)),
            dict(d=edit(src_off=descs[0]["src_off"] + cc.TAIL + 1)), dict(off=[out_bytes - 3]), dict(nb=10), dict(nb=0)]
    for bad in bads:
        _refused(dev, lambda: ok(**bad))
        assert _same(ok()[0], want), bad

    c = cc.ROT_BY_NAME["chain"]
    rbuf, rows = cc.rot_buffer(c), cc.rot_rows(c)
    rwant = R.rotate180(rbuf, rows)
    rot = lambda r=rows, seg=c["seg"], b=rbuf: dev.selftest_rotate180_groups(b, r, seg)
    redit = lambda i, v: [rows[0][:i] + (v,) + rows[0][i + 1:]] + rows[1:]
    rbads = [dict(r=np.zeros((0, 6), np.int64), seg=[0]), dict(r=redit(2, 38)), dict(r=redit(3, 20)), dict(r=redit(4, 0)), dict(r=redit(5, -1)),
             dict(r=redit(2, -1)), dict(r=redit(0, -1)), dict(r=redit(0, rbuf.size)), dict(r=redit(1, 30)), dict(seg=[0, 4]), dict(seg=[1, 3]),
             dict(seg=[0, 2, 1]), dict(seg=[0, 1, 3]),            # A | B C: two groups that share pixels
             dict(r=[rows[0], (1,) + rows[1][1:]], seg=[0, 1, 2])]  # two views over the same bytes, a group each
    for bad in rbads:
        _refused(dev, lambda: rot(**bad))
        assert _same(rot(), rwant), bad

    img = cc.plan_image()
    good = np.array(cc.PLAN_QUADS["sides_3_4_5"], np.int32)
    for name, q in cc.PLAN_REFUSED.items():
        with pytest.raises(dev.OcrError, match="no crop inside"):
            dev.rotate_crops(img, [good, np.array(q, np.int32)])
        with pytest.raises(dev.OcrError, match="no crop inside"):
            dev.selftest_crop_plan(cc.PLAN_ROWS, cc.PLAN_COLS, q)
        assert _same(dev.rotate_crops(img, [good])[0], R.rotate_crop(img, good)), name
    with pytest.raises(dev.OcrError, match="outside the image"):
        dev.rotate180_rois(img, [(20, 10, 5, 5)])
    assert _same(dev.rotate180_rois(img, [(19, 10, 5, 5)]).reshape(-1), R.rotate180(img.reshape(-1), [(0, 3 * cc.PLAN_COLS, 19, 10, 5, 5)]))
