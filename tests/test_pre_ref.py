"""tools/pre_ref.py, the plain restatement of what the resize-and-normalise kernels compute, against the oracle library (the
committed restatement of the reference's OpenCV path) on every case tests/test_gpu_pre_ops.py runs on the device: bit for
bit, u8 bytes and f32 bit patterns.  That equality is what lets the GPU tests compare with pre_ref and carry its mutations.
Plus: the resize against exact rational bilinear interpolation, every mutation against the case named for it, and the
normalisation table against float64."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pre_cases as pc  # noqa: E402
from bilinear_exact import fixed_against_exact, float64_bilinear  # noqa: E402

import pre_ref as R  # noqa: E402  (tools/ is on the path: conftest.py)

EXACT_PIXELS = 2100  # up to this many destination pixels the rational evaluation visits every one


def _eq(a, b):
    a, b = R.bits(a), R.bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def _oracle_tables(O):
    """the oracle's own normalised value per (channel, byte), read off identity resizes of images that hold every byte"""
    v = np.arange(256, dtype=np.uint8)
    strip = np.repeat(np.repeat(v[None, :, None], pc.IMG_H, 0), 3, 2)          # [48, 256, 3], column = value
    rec = O.rec_preprocess(strip, pc.IMG_H, 256)[0].transpose(1, 0).copy()     # 48 * 256 / 48 = 256 columns: a copy
    lo, hi = O.cls_preprocess(strip[:, :192]), O.cls_preprocess(strip[:, 64:])
    cls = np.concatenate([lo[0, :192], hi[0, 128:]], 0).transpose(1, 0).copy()
    det = O.det_preprocess(strip, pc.IMG_H, 256)[0][0].transpose(1, 0).copy()
    return {"det": det, "rec": rec, "cls": cls}


def _oracle_line(O, tables, view, q, tensor_w, pad, stage):
    x, y, w, h, rw = (int(v) for v in q[:5])
    u8 = O.resize_u8c3(view[y:y + h, x:x + w], pc.IMG_H, rw)
    out = np.empty((pc.IMG_H, tensor_w, 3), np.float32)
    for c in range(3):
        out[:, :rw, c] = tables[stage][c][u8[..., c]]
        out[:, rw:, c] = np.float32(0) if pad == R.PAD_CLS else tables[stage][c][0]
    return out, u8


@pytest.fixture(scope="module")
def O(built):
    import oracle
    return oracle


@pytest.fixture(scope="module")
def tables(O):
    return _oracle_tables(O)


def test_norm_table_equals_the_oracle_and_float64(O, tables):
    """(v / 255 - mean) / std in float64 against the 3 x 256 entries of each stage's table.  make_norm_lut rounds at: the f32
    constants e = f32(1/255), a = f32(1) / f32(std) and b = f32(-mean_f32 * a) (relative 2^-24 each, mean_f32 and std_f32
    themselves another 2^-24 from the decimal literals), ONE f32 product f = v * e, and ONE fused multiply-add f * a + b
    rounded once.  With x = v / 255 <= 1, A = 1 / std, B = mean / std and u = 2^-24 (second-order terms in the .0x):
      |f - x| <= 2.01u x    (e, the product)
      |a - A| <= 2.01u A    (std_f32, the division)
      |b + B| <= 4.02u B    (mean_f32, a, the rounding of the product)
      |f a - x A| <= 4.03u x A, so the exact fma argument is within 4.03u x A + 4.02u B of x A - B,
    and the one rounding of the fma adds at most u |result| <= 1.01u |x A - B| + (second order).
    Bound used: u * (4.03 x A + 4.02 B + 1.01 |x A - B|); no figure of the device enters it.  The oracle's own table is checked
    against it before pre_ref's."""
    u = 2.0 ** -24
    for stage, (mean, std) in R.STAGES.items():
        lut = R.norm_lut(stage)
        assert _eq(lut, tables[stage]), stage   # pre_ref's exactly rounded fma == the oracle's fmaf
        for c in range(3):
            x = np.arange(256, dtype=np.float64) / 255.0
            A, B = 1.0 / std[c], mean[c] / std[c]
            want = (x - mean[c]) / std[c]
            bound = u * (4.03 * x * A + 4.02 * B + 1.01 * np.abs(want))
            assert (np.abs(tables[stage][c].astype(np.float64) - want) <= bound).all(), ("oracle", stage, c)
            assert (np.abs(lut[c].astype(np.float64) - want) <= bound).all(), (stage, c)


@pytest.mark.parametrize("name", [c["name"] for c in pc.DET_CASES])
def test_det_cases_equal_the_oracle(O, name):
    c = pc.DET_BY_NAME[name]
    imgs = pc.det_images(c)
    x, tap = R.det_pre(imgs, c["dh"], c["dw"])
    for i, im in enumerate(imgs):
        assert _eq(tap[i], O.resize_u8c3(im, c["dh"], c["dw"]))
        ox, otap = O.det_preprocess(im, c["dh"], c["dw"])
        assert _eq(tap[i], otap) and _eq(x[i], ox)
    # the buffer the device test uploads holds exactly these images
    stride, img_bytes, size = pc.det_geometry(c)
    buf = pc.det_buffer(c, 255)
    assert buf.size == size
    for i, im in enumerate(imgs):
        at = c["off"] + i * img_bytes
        assert np.array_equal(np.lib.stride_tricks.as_strided(buf[at:], (c["sh"], 3 * c["sw"]), (stride, 1)).reshape(c["sh"], c["sw"], 3), im)


@pytest.mark.parametrize("name", [c["name"] for c in pc.LINE_LAUNCHES])
def test_line_launches_equal_the_oracle(O, tables, name):
    c = pc.LINE_BY_NAME[name]
    view = pc.parent_view(pc.parent_rows(pc.parent_image(c["kind"]), c["lines"]))
    got = R.line_pre(view, c["lines"], pc.IMG_H, c["imgW"], c["nslots"], c["pad"], c["stage"])
    named = set()
    direct = 0
    for q in c["lines"]:
        x, y, w, h, rw, slot = q
        want, u8 = _oracle_line(O, tables, view, q, c["imgW"], c["pad"], c["stage"])
        assert _eq(R.resize(view[y:y + h, x:x + w], pc.IMG_H, rw), u8)
        assert _eq(got[slot], want), q
        named.add(slot)
        if rw == pc.natural_w(h, w, pc.IMG_H, c["imgW"]):  # the stage's own width rule: the oracle's whole function
            if c["pad"] == R.PAD_REC:
                assert _eq(got[slot], O.rec_preprocess(view[y:y + h, x:x + w], pc.IMG_H, c["imgW"]))
                direct += 1
            elif c["imgW"] == 192:
                assert _eq(got[slot], O.cls_preprocess(view[y:y + h, x:x + w]))
                direct += 1
    for s in set(range(c["nslots"])) - named:
        assert (got[s].view(np.uint8) == R.FILL).all()
    if name.endswith(("_a", "_b")) and (c["pad"] == R.PAD_REC or c["imgW"] == 192):
        assert direct >= 1, "the launch holds a line at its natural width"


@pytest.mark.parametrize("name", [c["name"] for c in pc.RAGGED_LAUNCHES])
def test_ragged_launches_equal_the_oracle(O, tables, name):
    c = pc.RAGGED_BY_NAME[name]
    view = pc.parent_view(pc.parent_rows(pc.parent_image(c["kind"]), c["lines"]))
    got = R.line_pre_ragged(view, c["lines"], pc.IMG_H)
    for g, q in zip(got, c["lines"]):
        x, y, w, h, rw, tw = q
        assert 1 <= rw <= tw
        assert _eq(g, _oracle_line(O, tables, view, q, tw, R.PAD_REC, "rec")[0]), q
        if rw == pc.natural_w(h, w, pc.IMG_H, tw):
            assert _eq(g, O.rec_preprocess(view[y:y + h, x:x + w], pc.IMG_H, tw))


def _bilinear_cases():
    """(name, source image, dh, dw) of every resize of the case lists that takes the bilinear branch"""
    out = []
    for c in pc.DET_CASES:
        if (c["sh"], c["sw"]) != (c["dh"], c["dw"]) and not (c["sh"] == 2 * c["dh"] and c["sw"] == 2 * c["dw"]):
            out.append((c["name"], pc.det_images(c)[0], c["dh"], c["dw"]))
    seen = set()
    for c in pc.LINE_LAUNCHES + pc.RAGGED_LAUNCHES:
        img = pc.parent_image(c["kind"])
        for q in c["lines"]:
            x, y, w, h, rw = q[:5]
            key = (c["kind"], x, y, w, h, rw)
            if key in seen or (h, w) == (pc.IMG_H, rw) or (h, w) == (2 * pc.IMG_H, 2 * rw):
                continue
            seen.add(key)
            out.append(("%s_%d_%d_%dx%d_to_%d" % (c["kind"], x, y, h, w, rw), img[y:y + h, x:x + w], pc.IMG_H, rw))
    return out


_BILINEAR = _bilinear_cases()


@pytest.mark.parametrize("name", [b[0] for b in _BILINEAR])
def test_resize_within_one_of_exact_rational_bilinear(name):
    """Small destinations: the rational evaluation at every pixel.  Larger ones: a float64 evaluation of the same interpolation
    (its error is below 1e-9 grey levels) screens every pixel - |got - e| < 1.5 - 1e-6 implies that got is within 1 of the
    exactly rounded value - and the rational evaluation decides the pixels the screen cannot, the four border rows and columns
    and a 7 x 11 lattice."""
    _, img, dh, dw = next(b for b in _BILINEAR if b[0] == name)
    got = R.resize(img, dh, dw)
    if dh * dw <= EXACT_PIXELS:
        worst, _, _ = fixed_against_exact(img, got, dh, dw)
        assert worst <= 1
        return
    d = np.abs(got.astype(np.float64) - float64_bilinear(img, dh, dw))
    unsure = set((int(y), int(x)) for y, x in zip(*np.nonzero((d >= 1.5 - 1e-6).any(-1))))
    assert len(unsure) <= 64, "the fixed-point result strays from the interpolation"
    pts = unsure | {(y, x) for y in (0, 1, dh - 2, dh - 1) for x in range(dw)} | {(y, x) for y in range(dh) for x in (0, 1, dw - 2, dw - 1)}
    pts |= {(y, x) for y in range(0, dh, 7) for x in range(0, dw, 11)}
    worst, _, _ = fixed_against_exact(img, got, dh, dw, sorted(pts))
    assert worst <= 1


def _mutated_differs(mut):
    fam, name = pc.KILLED_BY[mut]
    if fam == "det":
        c = pc.DET_BY_NAME[name]
        imgs = pc.det_images(c)
        (x0, t0), (x1, t1) = R.det_pre(imgs, c["dh"], c["dw"]), R.det_pre(imgs, c["dh"], c["dw"], mut=(mut,))
        return not _eq(t0, t1) and not _eq(x0, x1)
    c = (pc.LINE_BY_NAME if fam == "line" else pc.RAGGED_BY_NAME)[name]
    view = pc.parent_view(pc.parent_rows(pc.parent_image(c["kind"]), c["lines"]))
    if fam == "line":
        a = R.line_pre(view, c["lines"], pc.IMG_H, c["imgW"], c["nslots"], c["pad"], c["stage"])
        b = R.line_pre(view, c["lines"], pc.IMG_H, c["imgW"], c["nslots"], c["pad"], c["stage"], mut=(mut,))
        return not _eq(a, b)
    a, b = R.line_pre_ragged(view, c["lines"], pc.IMG_H), R.line_pre_ragged(view, c["lines"], pc.IMG_H, mut=(mut,))
    return any(not _eq(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_every_mutation_is_killed_by_its_named_case(mut):
    """pre_cases.KILLED_BY names the case.  `no_area` is the one mutation no case can kill: at an exact halving the bilinear
    fixed-point formula IS the area mean (pre_ref.EQUIVALENT); that is proved here over every pair of row sums instead, and the
    halving cases must indeed not tell the two apart."""
    assert set(pc.KILLED_BY) == set(R.MUTATIONS)
    if pc.KILLED_BY[mut] is None:
        assert mut in R.EQUIVALENT
        a, b = np.meshgrid(np.arange(511, dtype=np.int64), np.arange(511, dtype=np.int64))   # a, b: the sums of a row's two taps
        assert np.array_equal(((1024 * ((1024 * a) >> 4)) >> 16) + ((1024 * ((1024 * b) >> 4)) >> 16) + 2 >> 2, (a + b + 2) >> 2)
        assert R._fixed(np.float32([0.5]), ())[0] == 1024
        assert pc.HALVINGS
        for name in pc.HALVINGS:
            c = pc.DET_BY_NAME[name]
            imgs = pc.det_images(c)
            assert _eq(R.det_pre(imgs, c["dh"], c["dw"])[1], R.det_pre(imgs, c["dh"], c["dw"], mut=(mut,))[1])
        return
    assert mut not in R.EQUIVALENT
    assert _mutated_differs(mut)
