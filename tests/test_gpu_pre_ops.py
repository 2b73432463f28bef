"""The resize-and-normalise launches of csrc/kernels_pre.hip alone (det_pre_kernel<1|4>, line_pre_kernel<1|4>,
line_pre_ragged_kernel, all on resize_px_scaled), through ocr_selftest_det_pre / _line_pre / _line_pre_ragged, at every branch
and edge (tests/pre_cases.py).  Every comparison is bit for bit against tools/pre_ref.py, which tests/test_pre_ref.py proves
equal to the oracle library on these very cases; f32 values are compared as uint32.  Every case also checks that the guard
region behind the output and every slot no descriptor names still hold the fill pattern, and that the bytes of the parent
buffer outside the images / ROIs (0, then 255) do not reach the result."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pre_cases as pc  # noqa: E402

import pre_ref as R  # noqa: E402  (tools/ is on the path: conftest.py)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(pkg, built):
    pkg.check(pkg.lib().ocr_rt_init(0))
    assert (pkg.SELFTEST_FILL, pkg.PAD_REC, pkg.PAD_CLS) == (R.FILL, R.PAD_REC, R.PAD_CLS)
    return pkg


def _same(a, b):
    a, b = R.bits(a), R.bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def _untouched(guard):
    return guard.size == 256 and (guard == R.FILL).all()


_STAGE = {"rec": 1, "cls": 2}
_cache = {}


def _run_det(dev, c, outside):
    key = ("det", c["name"], outside)
    if key not in _cache:
        stride, img_bytes, _ = pc.det_geometry(c)
        _cache[key] = dev.selftest_det_pre(pc.det_buffer(c, outside), c["off"], stride, img_bytes, c["N"], c["sh"], c["sw"], c["dh"], c["dw"])
    return _cache[key]


def _run_line(dev, c, outside):
    key = ("line", c["name"], outside)
    if key not in _cache:
        rows = pc.parent_rows(pc.parent_image(c["kind"]), c["lines"], outside)
        _cache[key] = dev.selftest_line_pre(rows, pc.PARENT_W, c["lines"], pc.IMG_H, c["imgW"], c["nslots"], c["pad"], _STAGE[c["stage"]])
    return _cache[key]


def _run_ragged(dev, c, outside):
    key = ("ragged", c["name"], outside)
    if key not in _cache:
        rows = pc.parent_rows(pc.parent_image(c["kind"]), c["lines"], outside)
        _cache[key] = dev.selftest_line_pre_ragged(rows, pc.PARENT_W, c["lines"], pc.IMG_H)
    return _cache[key]


def _view(c):
    return pc.parent_view(pc.parent_rows(pc.parent_image(c["kind"]), c["lines"]))


# ----------------------------------------------------------------------------------------------------------- detector
@pytest.mark.parametrize("name", [c["name"] for c in pc.DET_CASES])
def test_det_launch(dev, name):
    c = pc.DET_BY_NAME[name]
    want_x, want_tap = R.det_pre(pc.det_images(c), c["dh"], c["dw"])
    x0, tap0, gx0, gt0 = _run_det(dev, c, 0)
    x1, tap1, gx1, gt1 = _run_det(dev, c, 255)
    assert _same(tap0, want_tap), "u8 tap"
    assert _same(x0, want_x), "f32 tensor"
    assert _same(tap0, tap1) and _same(x0, x1), "bytes outside the images reach the result"
    assert _untouched(gx0) and _untouched(gt0) and _untouched(gx1) and _untouched(gt1), "a write behind the output"


_DET_API = [("max", 128, [(128, 256)]), ("max", 128, [(128, 128)]), ("max", 128, [(100, 300)]), ("min", 64, [(20, 50)]),
            ("max", 128, [(64, 64)] * 3)]


@pytest.mark.parametrize("limit_type,side,shapes", _DET_API, ids=["halving", "identity", "generic", "upscale", "batch3"])
def test_det_through_the_product_api(dev, limit_type, side, shapes):
    """what Det.run reaches: det.resized() against pre_ref and against the oracle's tap; no network output is asserted"""
    import oracle as O
    imgs = [pc.image("rand", h, w, seed=40 + i) for i, (h, w) in enumerate(shapes)]
    det = dev.Det(limit_type=limit_type, limit_side_len=side, max_batch=len(imgs))
    try:
        det.run_batch(imgs)
        rh, rw, _, _ = O.det_resize_shape(shapes[0][0], shapes[0][1], limit_type, side)
        assert det.last_shape() == (len(imgs), rh, rw)
        for i, im in enumerate(imgs):
            got = det.resized(i)
            assert _same(got, R.resize(im, rh, rw))
            assert _same(got, O.det_preprocess(im, rh, rw)[1])
    finally:
        det.close()


# -------------------------------------------------------------------------------------------------------------- lines
@pytest.mark.parametrize("name", [c["name"] for c in pc.LINE_LAUNCHES])
def test_line_launch(dev, name):
    c = pc.LINE_BY_NAME[name]
    want = R.line_pre(_view(c), c["lines"], pc.IMG_H, c["imgW"], c["nslots"], c["pad"], c["stage"])
    got, guard = _run_line(dev, c, None)
    named = {q[5] for q in c["lines"]}
    for q in c["lines"]:
        assert _same(got[q[5]], want[q[5]]), q
    for s in set(range(c["nslots"])) - named:
        assert (got[s].view(np.uint8) == R.FILL).all(), "slot %d is named by no line" % s
    assert _same(got, want) and _untouched(guard)
    (g0, u0), (g1, u1) = _run_line(dev, c, 0), _run_line(dev, c, 255)
    assert _same(g0, want) and _same(g1, want), "bytes outside the ROIs reach the result"
    assert _untouched(u0) and _untouched(u1)


@pytest.mark.parametrize("name", [c["name"] for c in pc.RAGGED_LAUNCHES])
def test_ragged_line_launch(dev, name):
    c = pc.RAGGED_BY_NAME[name]
    want = R.line_pre_ragged(_view(c), c["lines"], pc.IMG_H)
    for outside in (None, 0, 255):
        got, guard = _run_ragged(dev, c, outside)
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert _same(g, w), (outside, i, c["lines"][i])
        assert _untouched(guard)


# -------------------------------------------------------------------------------------------------------------- teeth
@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_mutated_reference_differs_from_the_device(dev, mut):
    """the case tests/pre_cases.KILLED_BY names for the mutation (tests/test_pre_ref.py shows that it changes the reference
    there).  `no_area` cannot change any result (pre_ref.EQUIVALENT has the arithmetic): for it the device must agree with the
    mutated reference on every halving case - a kernel without the area branch would be the same function."""
    if pc.KILLED_BY[mut] is None:
        assert mut in R.EQUIVALENT
        for name in pc.HALVINGS:
            c = pc.DET_BY_NAME[name]
            assert _same(_run_det(dev, c, 0)[1], R.det_pre(pc.det_images(c), c["dh"], c["dw"], mut=(mut,))[1])
        return
    fam, name = pc.KILLED_BY[mut]
    if fam == "det":
        c = pc.DET_BY_NAME[name]
        x, tap = R.det_pre(pc.det_images(c), c["dh"], c["dw"], mut=(mut,))
        got = _run_det(dev, c, 0)
        assert not _same(got[1], tap) and not _same(got[0], x)
    elif fam == "line":
        c = pc.LINE_BY_NAME[name]
        assert not _same(_run_line(dev, c, None)[0], R.line_pre(_view(c), c["lines"], pc.IMG_H, c["imgW"], c["nslots"], c["pad"], c["stage"], mut=(mut,)))
    else:
        c = pc.RAGGED_BY_NAME[name]
        want = R.line_pre_ragged(_view(c), c["lines"], pc.IMG_H, mut=(mut,))
        assert any(not _same(g, w) for g, w in zip(_run_ragged(dev, c, None)[0], want))


# ----------------------------------------------------------------------------------------------------------- refusals
def _refused(dev, call):
    with pytest.raises(dev.OcrError, match=r"error -1: \S") as e:   # OCR_ERR_ARG with a message
        call()
    return str(e.value)


def test_refusals_leave_the_next_call_working(dev):
    """whatever the launchers do not define is refused with OCR_ERR_ARG before it reaches the device"""
    c = pc.DET_BY_NAME["up_3x3"]
    stride, img_bytes, _ = pc.det_geometry(c)
    buf = pc.det_buffer(c, 0)
    ok = lambda **k: dev.selftest_det_pre(buf, *[k.get(n, v) for n, v in (("off", 0), ("stride", stride), ("img_bytes", img_bytes), ("N", 1), ("sh", 3),
                                                                          ("sw", 3), ("dh", 32), ("dw", 32))])
    for bad in (dict(N=0), dict(sh=0), dict(sw=-1), dict(dh=0), dict(dw=0), dict(stride=8), dict(off=buf.size), dict(N=2, img_bytes=4),
                dict(N=3), dict(sh=40), dict(dw=1 << 20)):
        _refused(dev, lambda: ok(**bad))
        assert _same(ok()[1], R.det_pre(pc.det_images(c), 32, 32)[1]), bad

    lc = pc.LINE_BY_NAME["w320_rec_pad0_c"]
    img = pc.parent_image()
    rows = pc.parent_rows(img, lc["lines"])
    want = R.line_pre(pc.parent_view(rows), lc["lines"], pc.IMG_H, 320, 5, R.PAD_REC)
    line = lambda lines=lc["lines"], cols=pc.PARENT_W, imgH=pc.IMG_H, imgW=320, nslots=5, pad=0, stage=1, parent=rows: \
        dev.selftest_line_pre(parent, cols, lines, imgH, imgW, nslots, pad, stage)
    q = lc["lines"][0]
    edit = lambda i, v: [q[:i] + (v,) + q[i + 1:]] + lc["lines"][1:]
    bads = [dict(lines=edit(4, 0)), dict(lines=edit(4, 321)), dict(lines=edit(0, 81)), dict(lines=edit(1, 25)), dict(lines=edit(0, -1)),
            dict(lines=edit(2, 0)), dict(lines=edit(3, -5)), dict(lines=edit(5, 5)), dict(lines=edit(5, -1)), dict(lines=edit(5, 0)),
            dict(imgH=0), dict(imgW=0), dict(nslots=2), dict(pad=2), dict(stage=0), dict(cols=402), dict(parent=rows[:, :1199].copy())]
    for bad in bads:
        _refused(dev, lambda: line(**bad))
        assert _same(line()[0], want), bad

    rc = pc.RAGGED_BY_NAME["r_eight_mixed"]
    rrows = pc.parent_rows(pc.parent_image(rc["kind"]), rc["lines"])
    rwant = R.line_pre_ragged(pc.parent_view(rrows), rc["lines"], pc.IMG_H)
    q = rc["lines"][2]
    redit = lambda i, v: rc["lines"][:2] + [q[:i] + (v,) + q[i + 1:]] + rc["lines"][3:]
    for lines in (redit(4, 0), redit(4, q[5] + 1), redit(5, 0), redit(0, 399), redit(3, 0)):
        _refused(dev, lambda: dev.selftest_line_pre_ragged(rrows, pc.PARENT_W, lines, pc.IMG_H))
        got = dev.selftest_line_pre_ragged(rrows, pc.PARENT_W, rc["lines"], pc.IMG_H)[0]
        assert all(_same(g, w) for g, w in zip(got, rwant))
    _refused(dev, lambda: dev.selftest_line_pre_ragged(rrows, pc.PARENT_W, rc["lines"], 0))
    _refused(dev, lambda: dev.selftest_line_pre_ragged(rrows, pc.PARENT_W, rc["lines"], pc.IMG_H, stage=3))
