"""Per-character evidence of the recognizer (ocr_rec_run_chars / ocr_pipe_run_chars): the CTC step, run length and
probability of every kept character, the top-k classes of that step's logits row (ctc_topk_kernel), and the characters'
quads in source-image coordinates.  DESIGN.md section 4b has the semantics, the tie rule and what is bit-exact."""
import math
import os

import numpy as np
import pytest

from tail_ref import collapse as _collapse  # (tools/ is on the path: conftest.py)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Relative error of the shipped pmax (the head's f32 chains) against the float64 softmax maximum of
# the same f32 logits, over the rows of all 192 kept characters of the two mobile configurations below: 2.52e-7 at
# (48, 320, 6) and 3.78e-7 at (28, 192, 16), measured on the oracle's head, whose (logits, pmax) the device's equal bit for
# bit (test_gpu_parity.test_rec_ids_scores_and_steps; the mobile test below prints the figure of its tapped rows); the 12
# kept characters of the four wider strips that test adds stay below it (2.14e-7 / 1.91e-7).  Rounded up.  Rank r > 0 of alt_probs is ocr_expf(x_r - x_0) * pmax: it inherits that error and adds one ocr_expf and one
# product, for which four f32 ulps (4 * 2^-23) are allowed.
PMAX_REL_ERR = 4e-7
ALT_REL_TOL = PMAX_REL_ERR + 4 * 2.0 ** -23


# ------------------------------------------------------------------------------------------ top-k kernel alone
def _rank(x, k):
    """numpy's ranking: stable arg sort of -x (NaN last, ties by index); ids padded with -1"""
    order = np.argsort(-x.astype(np.float64), kind="stable")[:k]
    return np.concatenate([order, np.full(k - len(order), -1)]).astype(np.int32)


def _topk_rows(C, rs):
    rows = []
    for _ in range(3):
        rows.append(rs.randn(C).astype(np.float32) * 3)
    rows.append(np.full(C, 1.25, np.float32))                       # all equal: ids 0..k-1
    r = rs.randn(C).astype(np.float32); r[C - 1] = 50.0; rows.append(r)          # the maximum in the last column
    r = rs.randn(C).astype(np.float32)                               # the k best owned by one lane (dword loads: c mod 64)
    for j, c in enumerate(range(5 % C, C, 64)):
        if j < 8:
            r[c] = 40.0 - j
    rows.append(r)
    r = rs.randn(C).astype(np.float32)                               # ... and by one lane of the 16-byte form (c // 4 mod 64)
    for j, c in enumerate([0, 1, 2, 3, 256, 257, 258, 259]):
        if c < C:
            r[c] = 30.0 + (j % 3)
    rows.append(r)
    r = rs.randn(C).astype(np.float32); r[:min(8, C)] = 20.0 - np.arange(min(8, C)); rows.append(r)   # the k best in columns 0..k-1
    r = rs.randn(C).astype(np.float32)                               # duplicates straddling lanes 31 / 32
    for c, v in ((31, 9.0), (32, 9.0), (95, 8.0), (96, 8.0), (33, 9.0)):
        if c < C:
            r[c] = v
    rows.append(r)
    r = rs.randn(C).astype(np.float32); r[rs.rand(C) < 0.5] = -np.inf; rows.append(r)                 # -inf entries
    r = rs.randn(C).astype(np.float32); r[0] = -np.inf; r[C // 2] = np.nan; rows.append(r)            # one NaN
    r = rs.randn(C).astype(np.float32); r[C - 1] = np.nan; r[: C - 1] = np.minimum(r[: C - 1], 1.0); rows.append(r)
    return np.stack(rows)


@pytest.mark.parametrize("C", [1, 7, 64, 65, 127, 6625])
def test_topk_kernel_alone(pkg, built, C):
    rs = np.random.RandomState(100 + C)
    x = _topk_rows(C, rs)
    n = x.shape[0]
    p0 = (rs.rand(n) * 0.9 + 0.05).astype(np.float32)
    for pitch in sorted({C, (C + 7) // 8 * 8}):
        buf = np.full((n, pitch), 77.0, np.float32)      # the pad columns hold large values: they must never be read as classes
        buf[:, :C] = x
        for k in (1, 5, 8):
            ids, probs = pkg.selftest_topk(buf, p0, k, ncols=C)
            for i in range(n):
                want = _rank(x[i], k)
                assert np.array_equal(ids[i], want), (C, pitch, k, i, ids[i], want)
                if i == 3:
                    assert np.array_equal(ids[i][:min(k, C)], np.arange(min(k, C)))
                assert probs[i, 0].tobytes() == p0[i].tobytes()            # rank 0: the caller's p0, bit for bit
                for r in range(1, k):
                    if want[r] < 0:
                        assert probs[i, r] == 0.0
                        continue
                    d = float(np.float64(x[i, want[r]]) - np.float64(x[i, want[0]]))
                    if math.isnan(d):
                        assert math.isnan(probs[i, r]) or math.isnan(x[i, want[0]])
                        continue
                    # the head's exp clamps its argument at -87 (ocr_common.h); its argument is the f32 difference (half an
                    # ulp of |d|), the polynomial is good to 2 ulps, the product rounds once; below f32's normal range only
                    # an absolute bound makes sense
                    ref = math.exp(max(d, -87.0)) * float(p0[i])
                    tol = ref * (abs(max(d, -87.0)) * 2.0 ** -24 + 4 * 2.0 ** -23) + 2e-38
                    assert abs(float(probs[i, r]) - ref) <= tol, (C, pitch, k, i, r, probs[i, r], ref)


def test_topk_argument_checks(pkg, built):
    x = np.zeros((1, 8), np.float32)
    for k in (0, 9):
        with pytest.raises(pkg.OcrError):
            pkg.selftest_topk(x, [0.5], k)


# ------------------------------------------------------------------------------------------ mobile recognizer
def _crops():
    import oracle as O
    from synth_data import cfg2_sample
    img, prob, _ = cfg2_sample(0)
    boxes = O.det_post(prob, 0.3, 0.5, 2.0, 960, 960)
    crops = []
    for b in boxes:
        r = O.crop_rect(b, 960, 960)
        if r:
            x, y, w, h = r
            crops.append(img[y:y + h, x:x + w])
    return crops


def _mobile_T(w):
    """CTC steps of the mobile recognizer for tensor width w (plans/rec.plan: stride-2 3x3 conv, stride-2 3x3 depthwise, 2-wide pool)"""
    a = (w - 1) // 2 + 1
    return ((a - 1) // 2 + 1) // 2


_ORACLE = {}


def _oracle_steps(h, w, bn):
    if (h, w, bn) not in _ORACLE:
        from pipeline import Pipeline
        _ORACLE[(h, w, bn)] = Pipeline(rec_batch_num=bn, rec_img_h=h, rec_img_w=w).rec_run(_crops())
    return _ORACLE[(h, w, bn)]


def _wide_lines():
    """four strips of the sample image wider than either rec_img_w / rec_img_h: each is a batch, and a tensor width, of its own"""
    from synth_data import cfg2_sample
    img = cfg2_sample(0)[0]
    return [img[200 + 60 * k:240 + 60 * k, 100:100 + 40 * r] for k, r in enumerate((8, 10, 13, 17))]


def _oracle_wide(h, w, bn):
    if ("wide", h, w, bn) not in _ORACLE:
        from pipeline import Pipeline
        po = Pipeline(rec_batch_num=bn, rec_img_h=h, rec_img_w=w)
        _ORACLE[("wide", h, w, bn)] = [po.rec_run([s]) for s in _wide_lines()]
    return _ORACLE[("wide", h, w, bn)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_against_steps(ids, chars, steps_of):
    """steps / nsteps / probs of every line == the numpy collapse of that line's per-step (amax, pmax); probs bitwise"""
    for i, c in enumerate(chars):
        am, pm = steps_of(i)
        wi, ws, wn, wp = _collapse(am, pm)
        assert np.array_equal(ids[i], wi), i
        assert np.array_equal(c["steps"], ws) and np.array_equal(c["nsteps"], wn), i
        assert np.array_equal(_bits(c["probs"]), _bits(wp)), i
        assert c["geom"][0] == len(am)


def _check_topk_on_rows(rec, ids, chars, lines, k, amax_of=None, measure=None):
    """alt_ids == numpy's ranking of the tapped logits row, for every kept character of `lines`; arg max of the row == amax"""
    checked = 0
    for i in lines:
        c = chars[i]
        for j, st in enumerate(c["steps"]):
            row = rec.logits_row(i, int(st))
            assert np.array_equal(c["alt_ids"][j], _rank(row, k)), (i, j)
            if amax_of is not None:
                assert int(np.argmax(row)) == int(amax_of(i)[st])
            if measure is not None:
                x = row.astype(np.float64)
                e = np.exp(x - x.max())
                p = e / e.sum()
                measure["pmax"] = max(measure["pmax"], abs(float(c["probs"][j]) - p.max()) / p.max())
                for r in range(1, k):
                    ref = p[c["alt_ids"][j][r]]
                    measure["alt"] = max(measure["alt"], abs(float(c["alt_probs"][j][r]) - ref) / ref)
            checked += 1
    return checked


@pytest.mark.parametrize("h,w,bn", [(48, 320, 6), (28, 192, 16)])
def test_rec_chars_mobile_fp32(pkg, built, h, w, bn):
    crops = _crops()
    assert len(crops) == 32
    to, so, steps = _oracle_steps(h, w, bn)
    rec = pkg.Rec(rec_batch_num=bn, rec_img_h=h, rec_img_w=w)
    tg, sg = rec.run(crops)
    t0, s0, c0 = rec.run_chars(crops, topk=0)
    assert all(np.array_equal(a, b) for a, b in zip(tg, t0)) and np.array_equal(_bits(sg), _bits(s0))
    assert all(np.array_equal(a, b) for a, b in zip(to, t0)) and np.array_equal(so, s0)
    _check_against_steps(t0, c0, lambda i: steps[i])
    for i, c in enumerate(c0):
        am, _ = rec.steps(i)
        T, tensor_w, resize_w = c["geom"]
        assert T == len(am) == _mobile_T(tensor_w) and 0 < resize_w <= tensor_w and tensor_w >= w
    t5, s5, c5 = rec.run_chars(crops, topk=5)
    assert all(np.array_equal(a, b) for a, b in zip(t0, t5)) and np.array_equal(_bits(s0), _bits(s5))
    for a, b, ids in zip(c0, c5, t5):
        assert np.array_equal(a["steps"], b["steps"]) and np.array_equal(a["nsteps"], b["nsteps"])
        assert np.array_equal(_bits(a["probs"]), _bits(b["probs"])) and a["geom"] == b["geom"]
        assert b["alt_ids"].shape == (len(ids), 5)
        assert np.array_equal(b["alt_ids"][:, 0], ids)
        assert np.array_equal(_bits(b["alt_probs"][:, 0]), _bits(b["probs"]))
    # tapped rows: every kept character of lines of different tensor widths.  The 32 crops all fit rec_img_w (one tensor
    # width per configuration), so the first line with characters stands for that width and four wider strips of the same
    # image, each a call - and so a batch and a tensor width - of its own, give four more
    first = next(i for i in range(len(crops)) if len(t5[i]))
    m = dict(pmax=0.0, alt=0.0)
    assert _check_topk_on_rows(rec, t5, c5, [first], 5, amax_of=lambda i: steps[i][0], measure=m) > 0
    widths = {c5[first]["geom"][1]}
    ow, nchars = _oracle_wide(h, w, bn), 0
    for strip, (wt, ws, wsteps) in zip(_wide_lines(), ow):
        tw, sw, cw = rec.run_chars([strip], topk=5)
        assert np.array_equal(tw[0], wt[0]) and np.array_equal(_bits(sw), _bits(ws))
        _check_against_steps(tw, cw, lambda i: wsteps[i])
        assert cw[0]["geom"][0] == _mobile_T(cw[0]["geom"][1]) and cw[0]["geom"][1] > w
        assert np.array_equal(cw[0]["alt_ids"][:, 0], tw[0]) and np.array_equal(_bits(cw[0]["alt_probs"][:, 0]), _bits(cw[0]["probs"]))
        nchars += _check_topk_on_rows(rec, tw, cw, [0], 5, amax_of=lambda i: wsteps[i][0], measure=m)
        widths.add(cw[0]["geom"][1])
    assert len(widths) >= 5 and nchars > 0, widths
    print("rec %dx%d: rel. error of pmax against the float64 softmax maximum %.3g, of alt_probs[r>0] %.3g (allowed %.3g)"
          % (h, w, m["pmax"], m["alt"], ALT_REL_TOL))
    assert m["pmax"] <= PMAX_REL_ERR, m
    assert m["alt"] <= ALT_REL_TOL, m
    # the default call afterwards is still the default call (the head goes back to its fused form)
    tg2, sg2 = rec.run(crops)
    assert all(np.array_equal(a, b) for a, b in zip(tg, tg2)) and np.array_equal(_bits(sg), _bits(sg2))
    rec.close()


def _blank_model_dir(tmp_path):
    """the recognizer's graph with the seeded weights and a CTC head that answers "blank" at every step (the blank class's
    bias raised far above every logit): every line then yields no character.  (With the seeded weights alone every input,
    flat ones included, yields a few characters.)"""
    import shutil
    import synth_weights
    from pdmodel import write_params
    src = os.path.join(ROOT, "models", "rec")
    dst = str(tmp_path / "rec_blank")
    os.makedirs(dst)
    shutil.copy(os.path.join(src, "inference.pdmodel"), dst)
    params = synth_weights.synth_params(os.path.join(src, "inference.pdmodel"))
    bias = np.array(params["linear_85.b_0"], np.float32)
    assert bias.size == 6625
    bias.reshape(-1)[0] += 1000.0
    params["linear_85.b_0"] = bias
    write_params(os.path.join(dst, "synthetic.pdiparams"), params)
    return dst


def test_rec_chars_lines_without_characters(pkg, built, tmp_path):
    crops = _crops()[:3]
    rec = pkg.Rec(model_dir=_blank_model_dir(tmp_path), label_path=os.path.join(ROOT, "models", "rec", "ppocr_keys_v1.txt"),
                  rec_batch_num=6, rec_img_h=48, rec_img_w=320)
    tg, sg = rec.run(crops)
    for topk in (0, 5):
        t, s, c = rec.run_chars(crops, topk=topk)
        assert all(len(a) == 0 for a in tg) and all(len(a) == 0 for a in t)          # lens == 0
        assert np.array_equal(_bits(sg), _bits(s)) and not s.any()
        for i, ch in enumerate(c):
            assert len(ch["steps"]) == len(ch["nsteps"]) == len(ch["probs"]) == 0 and ch["geom"][0] == len(rec.steps(i)[0]) > 0
            if topk:
                assert ch["alt_ids"].shape == (0, 5) and ch["alt_probs"].shape == (0, 5)
    rec.close()


def test_rec_chars_mobile_shapes_and_capacity(pkg, built):
    """the three launch shapes in one call (ragged lines, an over-wide line as a uniform launch of its own) and a max_len
    below a line's length"""
    crops = _crops()[:5]
    rs = np.random.RandomState(5)
    wide = rs.randint(0, 256, (48, 3300, 3)).astype(np.uint8)       # wider than the ragged attention kernel takes
    flat = [np.full((48, 64, 3), v, np.uint8) for v in (255, 0, 128)] + [np.full((4, 4, 3), 200, np.uint8)]
    allc = crops + [wide] + flat
    rec = pkg.Rec(rec_batch_num=6, rec_img_h=48, rec_img_w=320)
    tg, sg = rec.run(allc)
    t5, s5, c5 = rec.run_chars(allc, topk=5)
    assert all(np.array_equal(a, b) for a, b in zip(tg, t5)) and np.array_equal(_bits(sg), _bits(s5))
    _check_against_steps(t5, c5, rec.steps)
    iw = len(crops)
    assert c5[iw]["geom"][1] >= 3300 and c5[iw]["geom"][0] == _mobile_T(c5[iw]["geom"][1])
    for c, ids in zip(c5, t5):
        assert np.array_equal(c["alt_ids"][:, 0], ids) and np.array_equal(_bits(c["alt_probs"][:, 0]), _bits(c["probs"]))
    assert len(t5[iw]) > 0
    _check_topk_on_rows(rec, t5, c5, [iw], 5, amax_of=lambda i: rec.steps(i)[0])
    longest = max(len(t) for t in t5)
    assert longest > 1
    with pytest.raises(pkg.OcrError, match="max_len"):
        rec.run_chars(allc, max_len=longest - 1, topk=5)
    with pytest.raises(pkg.OcrError, match="max_len"):
        rec.run(allc, max_len=longest - 1)
    for k in (-1, 9):
        with pytest.raises(pkg.OcrError, match="topk"):
            rec.run_chars(crops, topk=k)
    rec.close()


def test_rec_chars_mobile_fp16(pkg, built):
    crops = _crops()[:12]
    rec = pkg.Rec(rec_batch_num=6, rec_img_h=48, rec_img_w=320, precision="fp16")
    t0, s0, c0 = rec.run_chars(crops, topk=0)
    t5, s5, c5 = rec.run_chars(crops, topk=5)
    _check_against_steps(t5, c5, rec.steps)
    for a, b, i0, i5 in zip(c0, c5, t0, t5):
        assert np.array_equal(i0, i5) and np.array_equal(a["steps"], b["steps"])
        assert np.array_equal(b["alt_ids"][:, 0], i5) and np.array_equal(_bits(b["alt_probs"][:, 0]), _bits(b["probs"]))
    lines = [i for i in range(len(crops)) if len(t5[i])][:4]
    assert _check_topk_on_rows(rec, t5, c5, lines, 5, amax_of=lambda i: rec.steps(i)[0]) > 0
    rec.close()


# ------------------------------------------------------------------------------------------ server recognizer
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_rec_chars_server(pkg, built, precision):
    import synth_weights
    synth_weights.ensure_server(ROOT)
    rs = np.random.RandomState(11)
    crops = [rs.randint(0, 256, (48, 320, 3)).astype(np.uint8) for _ in range(4)]
    rec = pkg.Rec(model_dir=os.path.join(ROOT, "models_server", "rec"), label_path=os.path.join(ROOT, "models", "rec", "ppocr_keys_v1.txt"),
                  rec_batch_num=16, rec_img_h=48, rec_img_w=320, precision=precision)
    tg, sg = rec.run(crops)
    t0, s0, c0 = rec.run_chars(crops, topk=0)
    t5, s5, c5 = rec.run_chars(crops, topk=5)
    assert sum(len(t) for t in t5) > 0
    _check_against_steps(t5, c5, rec.steps)               # the device taps of the same call (T = 80)
    assert all(c["geom"][:2] == (80, 320) and 0 < c["geom"][2] <= 320 for c in c5)
    for b, ids in zip(c5, t5):
        assert np.array_equal(b["alt_ids"][:, 0], ids) and np.array_equal(_bits(b["alt_probs"][:, 0]), _bits(b["probs"]))
    _check_topk_on_rows(rec, t5, c5, range(4), 5, amax_of=lambda i: rec.steps(i)[0])
    if precision == "fp32":
        assert all(np.array_equal(a, b) for a, b in zip(tg, t0)) and np.array_equal(_bits(sg), _bits(s0))
        assert all(np.array_equal(a, b) for a, b in zip(t0, t5)) and np.array_equal(_bits(s0), _bits(s5))
        for a, b in zip(c0, c5):
            assert np.array_equal(a["steps"], b["steps"]) and np.array_equal(a["nsteps"], b["nsteps"])
            assert np.array_equal(_bits(a["probs"]), _bits(b["probs"]))
    rec.close()


# ------------------------------------------------------------------------------------------ pipeline: character quads
def _line_geometry(cw, ch, imgH=28, imgW=192):
    """CrnnResizeImg geometry of a line that is a batch of its own (rec_batch_num = 1): tensor_w, resize_w (ocr_rec.cpp:47-57)"""
    f = np.float32
    max_wh = max(f(imgW * 1.0 / imgH), f(cw * 1.0 / ch))
    bw = int(f(imgH) * max_wh)
    ratio = f(cw) / f(ch)
    rw = int(math.ceil(f(imgH) * ratio))
    return max(bw, imgW), min(rw, bw)


def _inverse_homography(box):
    """destination (warp pixel) -> source (image) of Utility::GetRotateCropImage, by solving the 8x8 system in float64"""
    b = np.asarray(box, np.float64).reshape(4, 2)
    dw = int(math.sqrt((b[0, 0] - b[1, 0]) ** 2 + (b[0, 1] - b[1, 1]) ** 2))
    dh = int(math.sqrt((b[0, 0] - b[3, 0]) ** 2 + (b[0, 1] - b[3, 1]) ** 2))
    dst = np.array([[0, 0], [dw, 0], [dw, dh], [0, dh]], np.float64)
    A, rhs = np.zeros((8, 8)), np.zeros(8)
    for i in range(4):
        u, v = dst[i]
        x, y = b[i]
        A[i] = [u, v, 1, 0, 0, 0, -u * x, -v * x]
        A[i + 4] = [0, 0, 0, u, v, 1, -u * y, -v * y]
        rhs[i], rhs[i + 4] = x, y
    m = np.append(np.linalg.solve(A, rhs), 1.0).reshape(3, 3)
    return m, dw, dh


def _quad_ref(step, nsteps, T, tensor_w, resize_w, cw, ch, turned, rows, cols, origin=None, box=None):
    s = tensor_w / T
    xa = min(max(step * s, 0.0), float(resize_w))
    xb = min(max((step + nsteps) * s, 0.0), float(resize_w))
    sx = cw / resize_w
    xa, xb = xa * sx, xb * sx
    out = []
    if box is not None:
        m, dw, dh = _inverse_homography(box)
        rot = float(dh) >= float(dw) * 1.5
    for x, y in ((xa, 0.0), (xb, 0.0), (xb, float(ch)), (xa, float(ch))):
        if turned:
            x, y = cw - x, ch - y
        if box is None:
            X, Y = origin[0] + x, origin[1] + y
        else:
            u, v = (dw - y, x) if rot else (x, y)
            p = m @ np.array([u, v, 1.0])
            X, Y = p[0] / p[2], p[1] / p[2]
        out.append([min(max(math.floor(X + 0.5), 0), cols - 1), min(max(math.floor(Y + 0.5), 0), rows - 1)])
    return np.array(out, np.int64)


_PIPE_IMGS = {}


def _pipe_images(card):
    if not _PIPE_IMGS:
        from synth_data import cfg2_sample
        _PIPE_IMGS["imgs"] = [card, np.ascontiguousarray(card[::-1, ::-1]), cfg2_sample(0)[0]]
    return _PIPE_IMGS["imgs"]


@pytest.mark.parametrize("phases", [1, 2])
@pytest.mark.parametrize("crop_mode", [0, 1])
@pytest.mark.parametrize("cls_on", [False, True])
def test_pipeline_char_quads(pkg, built, card, cls_on, crop_mode, phases):
    import oracle as O
    imgs = _pipe_images(card)
    assert imgs[2].shape[:2] == (960, 960)
    pipe = pkg.Pipe(enable_cls=cls_on, crop_mode=crop_mode, phases=phases, rec_batch_num=1)
    plain = pipe.run(imgs)
    got = pipe.run_chars(imgs)
    pipe.close()
    cls = pkg.Cls() if cls_on else None
    nchars = nturned = 0
    for img, g, w in zip(imgs, got, plain):
        rows, cols = img.shape[:2]
        assert len(g) == len(w)
        for a, b in zip(g, w):                                      # words / ids are Pipe.run's
            assert np.array_equal(a["box"], b["box"]) and np.array_equal(a["ids"], b["ids"])
            assert np.float32(a["confidence"]).tobytes() == np.float32(b["confidence"]).tobytes()
        # the crops the recognizer read, and which of them the classifier turned (one pass over all crops before any rotation)
        geo = []
        for a in g:
            if crop_mode == 0:
                r = O.crop_rect(a["box"], rows, cols)
                assert r is not None
                geo.append(dict(w=r[2], h=r[3], origin=(r[0], r[1]), box=None))
            else:
                ch, cw = pkg.rotate_crop_shape(rows, cols, a["box"])
                geo.append(dict(w=cw, h=ch, origin=None, box=a["box"]))
        turned = [0] * len(g)
        if cls_on and g:
            if crop_mode == 0:
                crops = [img[q["origin"][1]:q["origin"][1] + q["h"], q["origin"][0]:q["origin"][0] + q["w"]] for q in geo]
            else:
                crops = pkg.rotate_crops(img, np.stack([a["box"] for a in g]))
            turned = [int(v) for v in cls.run(crops)[0]]
        if img is imgs[1]:
            nturned += sum(turned)
        for a, q, t in zip(g, geo, turned):
            assert len(a["chars"]) == len(a["ids"])
            tensor_w, resize_w = _line_geometry(q["w"], q["h"])
            T = _mobile_T(tensor_w)
            s = np.float32(0)
            centres = []
            for c in a["chars"]:
                assert 0 <= c["step"] < T and 1 <= c["nsteps"] <= T - c["step"]
                want = _quad_ref(c["step"], c["nsteps"], T, tensor_w, resize_w, q["w"], q["h"], bool(t), rows, cols, q["origin"], q["box"])
                if crop_mode == 0:
                    assert np.array_equal(c["quad"], want), (c, want)
                else:
                    assert np.abs(c["quad"] - want).max() <= 1, (c, want)
                s = np.float32(s + np.float32(c["prob"]))
                centres.append(c["quad"].mean(axis=0))
                nchars += 1
            if a["chars"]:                                          # the probabilities are the terms of the word's score
                assert np.float32(s / np.float32(len(a["chars"]))).tobytes() == np.float32(a["confidence"]).tobytes()
            # along p0 -> p1 in reading order; a turned crop comes back mirrored (a 90-degree-turned crop reads along p0 -> p3)
            bx = a["box"].astype(np.float64)
            upright = crop_mode == 0 or not (int(np.hypot(*(bx[0] - bx[3]))) >= 1.5 * int(np.hypot(*(bx[0] - bx[1]))))
            if len(centres) > 1 and upright:
                proj = np.array(centres) @ (bx[1] - bx[0])
                d = np.diff(proj)
                assert (d <= 0).all() if t else (d >= 0).all(), (t, proj)
    assert nchars > 0
    if cls_on:
        assert nturned > 0                                          # the image fed upside down: its crops were turned
    if cls is not None:
        cls.close()
