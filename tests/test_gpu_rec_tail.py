"""The recognizer's tail launches alone, on designed data (ocr_selftest_softmax_argmax / _head_combine / _srv_argmax / _ctc_reduce /
_ctc / _topk_lines, each calling the launch function production binds), against tools/tail_ref.py - proved equal to the oracle
library on these very cases by tests/test_tail_ref.py.

Exact: every arg max; the mobile kernels' pmax and probs (one canonical f32 order); everything the collapse
writes.  Bounded: the server kernels' pmax (hardware exp2), by srv_ref.ctc_tail / ctc_fold, derived from the rounding points; the
mobile pmax is also held to net_ref's softmax bound against float64.  The worst error over bound of each family is printed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tail_cases as tc  # noqa: E402

import net_ref  # noqa: E402
import srv_ref  # noqa: E402
import tail_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

HEADS = tc.head_cases()
COLLAPSE = tc.collapse_cases()
_REF = {}


def _ref32(name):
    if name not in _REF:
        _REF[name] = R.softmax32(HEADS[name][0], probs=True)
    return _REF[name]


def _clean(*guards):
    for g in guards:
        assert g.size == 256 and (g == R.FILL).all(), "guard bytes overwritten"


def _eq(a, b):
    a, b = R.bits(a), R.bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def _padded(x, ld):
    buf = np.full((x.shape[0], ld), 77.0, np.float32)   # pad columns hold large values: they must never count as classes
    buf[:, :x.shape[1]] = x
    return buf


def _lds(C, one_pass):
    return sorted({(C + 3) & ~3, ((C + 3) & ~3) + 8}) if one_pass else sorted({C, C + 3})


# ------------------------------------------------------------------------------------------------------------ mobile heads
@pytest.mark.parametrize("name", sorted(HEADS))
def test_softmax_argmax_kernel_bit_for_bit(pkg, built, name):
    x, want = HEADS[name]
    amax, pmax, probs = _ref32(name)
    out = pkg.selftest_softmax_argmax(x, probs=True)
    _clean(out["amax"][1], out["pmax"][1], out["probs"][1])
    assert np.array_equal(out["amax"][0], want) and np.array_equal(out["amax"][0], amax)
    assert _eq(out["pmax"][0], pmax) and _eq(out["probs"][0], probs)
    out = pkg.selftest_softmax_argmax(x)              # production's form: no probabilities written
    assert np.array_equal(out["amax"][0], amax) and _eq(out["pmax"][0], pmax)


@pytest.mark.parametrize("name", sorted(HEADS))
def test_head_combine_equals_the_unfused_head(pkg, built, name):
    """the fused head's second half on the canonical group partials: the same arg max and the same pmax bits as the unfused kernel"""
    x, want = HEADS[name]
    amax, pmax, _ = _ref32(name)
    m, s, idx = R.group_partials(x)
    (a, ga), (p, gp) = pkg.selftest_head_combine(m, s, idx)
    _clean(ga, gp)
    assert np.array_equal(a, want) and np.array_equal(a, amax) and _eq(p, pmax)
    un = pkg.selftest_softmax_argmax(x)
    assert np.array_equal(un["amax"][0], a) and _eq(un["pmax"][0], p)


def test_mobile_probabilities_exact_and_inside_the_float64_bound(pkg, built):
    worst = 0.0
    for C in tc.HEAD_C:
        x = tc.random_rows(C)
        amax, pmax, probs = R.softmax32(x, probs=True)
        out = pkg.selftest_softmax_argmax(x, probs=True)
        assert np.array_equal(out["amax"][0], amax) and _eq(out["pmax"][0], pmax) and _eq(out["probs"][0], probs)
        (a, _), (p, _) = pkg.selftest_head_combine(*R.group_partials(x))
        assert np.array_equal(a, amax) and _eq(p, pmax)
        y, bound = net_ref.Ref.softmax(None, x.astype(np.float64))
        i = np.arange(len(x))
        ratio = float((np.abs(out["pmax"][0].astype(np.float64) - y[i, amax]) / bound[i, amax]).max())
        worst = max(worst, ratio, float((np.abs(out["probs"][0].astype(np.float64) - y) / bound).max()))
    print("mobile softmax_argmax / head_combine: worst |p - float64| / bound = %.3f" % worst)
    assert worst <= 1


# ------------------------------------------------------------------------------------------------------------ server heads
@pytest.mark.parametrize("one_pass", [False, True])
@pytest.mark.parametrize("name", sorted(HEADS))
def test_server_arg_max_exact(pkg, built, name, one_pass):
    x, want = HEADS[name]
    for ld in _lds(x.shape[1], one_pass):
        (a, ga), (p, gp) = pkg.selftest_srv_argmax(_padded(x, ld), ncols=x.shape[1], one_pass=one_pass)
        _clean(ga, gp)
        assert np.array_equal(a, want), (ld, np.nonzero(a != want)[0][:4])
        _, ref, bound = srv_ref.ctc_tail(x, "one_pass" if one_pass else "two_pass")
        assert (np.abs(p - ref) <= bound).all()


def test_server_probabilities_inside_the_derived_bounds(pkg, built):
    worst = {"two_pass": 0.0, "one_pass": 0.0, "ctc_reduce": 0.0}
    for C in tc.HEAD_C:
        x = tc.random_rows(C)
        for kind in ("two_pass", "one_pass"):
            amax, ref, bound = srv_ref.ctc_tail(x, kind)
            for ld in _lds(C, kind == "one_pass"):
                (a, _), (p, _) = pkg.selftest_srv_argmax(_padded(x, ld), ncols=C, one_pass=kind == "one_pass")
                assert np.array_equal(a, amax)
                worst[kind] = max(worst[kind], float((np.abs(p - ref) / bound).max()))
        m, s, idx = R.srv_partials(x)
        part = R.pack_partials(m, s, idx)                 # (what the device folds: the partials as f32)
        m32, s32 = part[..., 0].astype(np.float64), part[..., 1].astype(np.float64)
        for step in ((1, 2) if part.shape[1] > 1 else (1,)):   # (C = 2 has one slot)
            want, _ = R.srv_fold(m32, s32, idx, step=step)
            ref, bound = srv_ref.ctc_fold(m32[:, ::step], s32[:, ::step])
            (a, ga), (p, gp) = pkg.selftest_ctc_reduce(part, step=step)
            _clean(ga, gp)
            assert np.array_equal(a, want)
            worst["ctc_reduce"] = max(worst["ctc_reduce"], float((np.abs(p - ref) / bound).max()))
    for k, v in worst.items():
        print("server %s: worst |p - float64| / bound = %.3f" % (k, v))
    assert max(worst.values()) <= 1


@pytest.mark.parametrize("name", sorted(HEADS))
def test_ctc_reduce_arg_max_exact(pkg, built, name):
    x, want = HEADS[name]
    m, s, idx = R.srv_partials(x)
    (a, ga), (p, gp) = pkg.selftest_ctc_reduce(R.pack_partials(m, s, idx))
    _clean(ga, gp)
    assert np.array_equal(a, want)
    ref, bound = srv_ref.ctc_fold(m, np.float32(s).astype(np.float64))
    assert (np.abs(p - ref) <= bound).all()


# ------------------------------------------------------------------------------------ mobile fused head, through its binder
@pytest.fixture(scope="module")
def mob_weights(built, tmp_path_factory):
    """the mobile recognizer's weights with the head linear's replaced by tail_cases.mob_int_head (exact in f16 and f32)"""
    import oracle
    from pdmodel import write_params
    params = dict(oracle.load_weights("rec"))
    head = [ln for ln in oracle.plan_text("rec").splitlines() if ln.startswith("linear ")][-1].split()
    wn = [f[2:] for f in head if f.startswith("w=")][0]
    bn = [f for f in head if f.startswith("ep=bias:")][0][len("ep=bias:"):]
    assert params[wn].shape == (tc.MOB_K, tc.MOB_C) and params[bn].shape == (tc.MOB_C,)
    params[wn], params[bn] = tc.mob_int_head()
    path = str(tmp_path_factory.mktemp("rec_int") / "int_head.pdiparams")
    write_params(path, params)
    return path


def _mob(pkg, weights, precision, X, rows, mode):
    lines, w = tc.MOB_SHAPES[rows]
    out = pkg.selftest_rec_head(weights, precision, X, lines, tc.MOB_H, w, mode=mode)
    _clean(out["amax"][1], out["pmax"][1])
    assert "linear" in out["names"][0] and "softmax" in out["names"][1], out["names"]
    assert out["names"][2] == ("logits_fused" if mode == 0 else "logits_stored"), out["names"]   # the binder's own choice
    return out


@pytest.mark.parametrize("rows", sorted(tc.MOB_SHAPES))
def test_mobile_fused_head_exact_logits(pkg, built, mob_weights, rows):
    """conv_finish<OUT_HEAD> + head_combine_kernel as Net::bind binds them with RecStage's sinks, on small-integer inputs and weights
    (K = 120): the logits never reach memory but are known exactly.  fp32: amax exact, pmax the canonical order's bits, and the
    unfused head (logits kept) gives the same amax, the same pmax bits and the exact integers as logits."""
    W, b = tc.mob_int_head()
    X, which = tc.mob_int_rows(rows, seed=rows)
    y = (X.astype(np.float64) @ W + b).astype(np.float32)
    want = y.argmax(1)
    amax, pmax = R.softmax32(y)
    assert np.array_equal(amax, want)
    fused = _mob(pkg, mob_weights, "fp32", X, rows, 0)
    a, p = fused["amax"][0], fused["pmax"][0]
    assert np.array_equal(a, want), [(tc.MOB_DESIGNS[which[r]][0], a[r], want[r]) for r in np.nonzero(a != want)[0][:6]]
    assert _eq(p, pmax)
    kept = _mob(pkg, mob_weights, "fp32", X, rows, 1)
    assert np.array_equal(kept["logits"], y)
    assert np.array_equal(kept["amax"][0], a) and _eq(kept["pmax"][0], p)
    for mut in ("last_maximum", "tie_to_later_group"):        # teeth: here the device decides inside a group too
        if rows >= 12:
            assert not np.array_equal(a, R.first_maximum(y, mut=(mut,), group=32)[0])


@pytest.mark.parametrize("rows", [5, 256])
def test_mobile_fused_head_fp16(pkg, built, mob_weights, rows):
    """precision fp16: the same exact logits (small integers are exact in f16, the products accumulate in f32); amax exact, fused ==
    unfused, with and without probabilities; pmax held to float64 fed the device's own logits, by net_ref's softmax bound"""
    W, b = tc.mob_int_head()
    X, which = tc.mob_int_rows(rows, seed=rows)
    y = (X.astype(np.float64) @ W + b).astype(np.float32)
    want = y.argmax(1)
    fused = _mob(pkg, mob_weights, "fp16", X, rows, 0)
    assert np.array_equal(fused["amax"][0], want)
    worst = 0.0
    for mode in (1, 2):
        un = _mob(pkg, mob_weights, "fp16", X, rows, mode)
        assert np.array_equal(un["logits"], y) and np.array_equal(un["amax"][0], want)
        ref, bound = net_ref.Ref.softmax(None, un["logits"].astype(np.float64))
        i = np.arange(rows)
        for got in (un["pmax"][0], fused["pmax"][0]):
            worst = max(worst, float((np.abs(got.astype(np.float64) - ref[i, want]) / bound[i, want]).max()))
    print("mobile fused / unfused head, fp16, %d rows: worst |pmax - float64| / bound = %.3f" % (rows, worst))
    assert worst <= 1


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_mobile_fused_head_random_rows_with_a_margin(pkg, built, mob_weights, precision):
    """random f16-valued rows (exact in both precisions) on the integer weights (exact in both): the reference is the float64
    product; amax compared where the top-2 margin exceeds twice the linear's bound; at most 1 % of the rows may be left out"""
    W, b = tc.mob_int_head()
    A = tc.mob_random_rows(256)
    y = A.astype(np.float64) @ W + b
    top = np.sort(y, 1)[:, -2:]
    bound = srv_ref.linear_f32_bound(A.astype(np.float64), W.astype(np.float64), b, y).max(1)
    sure = (top[:, 1] - top[:, 0]) > 2 * bound
    print("mobile fused head, random rows, %s: %.2f %% of 256 rows left out of the margin-guarded comparison" % (precision, 100 * (1 - sure.mean())))
    assert 1 - sure.mean() <= 0.01
    out = _mob(pkg, mob_weights, precision, A, 256, 0)
    a, p = out["amax"][0], out["pmax"][0]
    assert np.array_equal(a[sure], y.argmax(1)[sure])
    assert ((0 <= a) & (a < tc.MOB_C)).all() and np.isfinite(p).all() and (p > 0).all() and (p <= 1).all()


def test_mobile_head_entry_refusals(pkg, built, mob_weights):
    X, _ = tc.mob_int_rows(4)
    for bad in (lambda: pkg.selftest_rec_head(mob_weights, "fp32", X, 1, tc.MOB_H, 40),            # 5 steps, 4 rows
                lambda: pkg.selftest_rec_head(mob_weights, "fp32", X[:, :100], 1, tc.MOB_H, 32),   # K is not the linear's
                lambda: pkg.selftest_rec_head(mob_weights, "int8", X, 1, tc.MOB_H, 32),
                lambda: pkg.selftest_rec_head(mob_weights, "fp32", X, 3, tc.MOB_H, 32),            # rows % lines
                lambda: pkg.selftest_rec_head(mob_weights, "fp32", X, 1, tc.MOB_H, 4),
                lambda: pkg.selftest_rec_head(mob_weights, "fp32", X, 1, tc.MOB_H, 32, mode=3)):
        with pytest.raises(pkg.OcrError, match="error -1"):
            bad()
        W, b = tc.mob_int_head()
        out = pkg.selftest_rec_head(mob_weights, "fp32", X, 1, tc.MOB_H, 32)
        assert np.array_equal(out["amax"][0], (X.astype(np.float64) @ W + b).argmax(1))


# ------------------------------------------------------------------------------------ server fused head, through its binding
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def int_head_dir(built, tmp_path_factory):
    """the server recognizer's seeded weights with the CTC head's replaced by tail_cases.srv_int_head (exact in f16)"""
    import shutil
    import synth_weights
    from pdmodel import read_params, write_params
    src = synth_weights.ensure_server(ROOT)[1]
    plan = os.path.join(ROOT, "cpp-paddle-ocr_amd", "plans", "srv_rec.plan")
    params = dict(read_params(src, sorted(n for n, _ in synth_weights.server_param_table(plan))))
    assert params["ctc_fc.w"].shape == (tc.SRV_K, tc.SRV_C)
    params["ctc_fc.w"], params["ctc_fc.b"] = tc.srv_int_head()
    d = tmp_path_factory.mktemp("srv_rec_int")
    write_params(str(d / "synthetic.pdiparams"), params)
    shutil.copy(os.path.join(os.path.dirname(src), "arch.txt"), str(d / "arch.txt"))
    return str(d)


def _run_head(net, x0, X, ctc):
    """binds the network on x0 with the head in partial mode (or not), replaces the head linear's input rows by X and runs that
    launch alone, then the tail launch the recognizer stage issues -> (amax, pmax, slots, step, logits or None)"""
    net.set_ctc(ctc)
    net.forward(x0)
    ls = net.launches()
    idx = max(i for i, (name, o, ins) in enumerate(ls) if o == ls[-1][1])     # the launch that writes the network's output
    name, o, ins = ls[idx]
    assert ("_ctc" in name) == bool(ctc), name                                 # the binder names the partial-mode launch so
    n, h, w = x0.shape[0], 1, X.shape[0] // x0.shape[0]
    net.upload(ins[0], X.reshape(n, h, w, tc.SRV_K))
    net.run_launches(idx, 1)
    a, p, slots, step = net.ctc_tail()
    return a, p, slots, step, (None if ctc else net.fetch(-1).reshape(-1, tc.SRV_C))


@pytest.mark.parametrize("lines", [1, 7])
def test_server_fused_head_exact_logits(pkg, built, int_head_dir, lines):
    """the matrix kernel's ctc_part epilogue + ctc_reduce_kernel with the handle's own ctc_slots() / ctc_step(), on small-integer
    inputs and weights (K = 384, the plan's): the logits never reach memory but are known exactly, ties are true ties.  One line (80 rows) sits
    below the matrix tile, seven (560 rows) cross the 256-thread blocks of the fold.  The unfused head of the same handle must agree."""
    W, b = tc.srv_int_head()
    net = pkg.SrvNet("rec", "fp16", model_dir=int_head_dir)
    try:
        x0 = np.random.RandomState(lines).randn(lines, 48, 320, 3).astype(np.float32)
        net.set_ctc(True)
        net.forward(x0)
        rows = len(net.ctc_tail()[0])
        assert rows % lines == 0 and rows >= 40 * lines and (lines > 1 or rows < 128)
        X, which = tc.srv_int_rows(rows)
        y = X.astype(np.float64) @ W + b
        want = y.argmax(1)                                        # first maximum (no NaN)
        a, p, slots, step, _ = _run_head(net, x0, X, True)
        assert slots == (tc.SRV_C + 63) // 64 and 1 <= step <= slots
        assert np.array_equal(a, want), [(tc.SRV_DESIGNS[which[r]][0], a[r], want[r]) for r in np.nonzero(a != want)[0][:6]]
        _, ref, bound = srv_ref.ctc_head(y, slots, step)
        r_fused = float((np.abs(p - ref) / bound).max())
        a2, p2, s2, _, logits = _run_head(net, x0, X, False)
        assert s2 == 0 and np.array_equal(logits, y.astype(np.float32))      # the unfused linear: the exact integers
        assert np.array_equal(a2, a)
        _, ref2, bound2 = srv_ref.ctc_tail(logits, "one_pass")
        r_unfused = float((np.abs(p2 - ref2) / bound2).max())
        print("server fused head (%d rows, step %d): worst |p - float64| / bound = %.3f; unfused on the device's logits %.3f"
              % (rows, step, r_fused, r_unfused))
        assert r_fused <= 1 and r_unfused <= 1
        # teeth: inside a slot and across tiles the first maximum is decided by the device here
        for mut in ("last_maximum", "tie_to_later_group"):
            assert not np.array_equal(a, R.first_maximum(y, mut=(mut,), group=64)[0])
    finally:
        net.close()


def test_server_fused_head_random_rows_with_a_margin(pkg, built, int_head_dir):
    """random f16 rows: the reference is the float64 product with the weights as the f16 build holds them (small integers: exactly);
    amax is compared where the float64 top-2 margin exceeds twice the linear's own bound (srv_ref.linear_f32_bound); at most 1 % of
    the rows may be left out"""
    W, b = tc.srv_int_head()
    net = pkg.SrvNet("rec", "fp16", model_dir=int_head_dir)
    try:
        x0 = np.random.RandomState(7).randn(7, 48, 320, 3).astype(np.float32)
        net.set_ctc(True)
        net.forward(x0)
        rows = len(net.ctc_tail()[0])
        A = tc.srv_random_rows(rows)
        y = A.astype(np.float64) @ W + b
        top = np.sort(y, 1)[:, -2:]
        bound = srv_ref.linear_f32_bound(A.astype(np.float64), W.astype(np.float64), b, y).max(1)
        sure = (top[:, 1] - top[:, 0]) > 2 * bound
        print("server fused head, random rows: %.2f %% of %d rows left out of the margin-guarded comparison" % (100 * (1 - sure.mean()), rows))
        assert 1 - sure.mean() <= 0.01
        a, p, slots, step, _ = _run_head(net, x0, A, True)
        assert np.array_equal(a[sure], y.argmax(1)[sure])
        assert ((0 <= a) & (a < tc.SRV_C)).all() and np.isfinite(p).all() and (p > 0).all() and (p <= 1 + 1e-6).all()
    finally:
        net.close()


# ------------------------------------------------------------------------------------- rows without a maximum, column limit
@pytest.mark.parametrize("C", tc.DEGENERATE_C)
def test_rows_without_a_maximum(pkg, built, C):
    """amax inside [0, C) - the first maximum, a NaN never being one, column 0 where there is none; pmax 0 where
    there is none and never inf.  The mobile kernels give the f32 restatement's bits; the server kernels may give NaN where a NaN or
    +inf entered their sums."""
    names, x = tc.degenerate_rows(C)
    amax, pmax = R.softmax32(x)
    none = [names.index(n) for n in ("all_neg_inf", "all_nan", "nan_and_neg_inf")]
    out = pkg.selftest_softmax_argmax(x)
    assert np.array_equal(out["amax"][0], amax) and _eq(out["pmax"][0], pmax)
    (a, _), (p, _) = pkg.selftest_head_combine(*R.group_partials(x))
    assert np.array_equal(a, amax) and _eq(p, pmax)
    m, s, idx = R.srv_partials(x)
    got = {"ctc_reduce": pkg.selftest_ctc_reduce(R.pack_partials(m, s, idx))}
    for one_pass in (False, True):
        got["one_pass" if one_pass else "two_pass"] = pkg.selftest_srv_argmax(_padded(x, (C + 3) & ~3), ncols=C, one_pass=one_pass)
    for k, ((a, ga), (p, gp)) in got.items():
        _clean(ga, gp)
        assert np.array_equal(a, amax), (k, a, amax)
        assert not np.isinf(p).any(), (k, p)
        assert (p[none] == 0).all(), (k, p[none])
        i = names.index("plain")
        if k == "ctc_reduce":
            ref, bound = srv_ref.ctc_fold(m[i:i + 1], np.float32(s[i:i + 1]).astype(np.float64))
        else:
            _, ref, bound = srv_ref.ctc_tail(x[i:i + 1], k)
        assert abs(float(p[i]) - float(ref[0])) <= float(bound[0]), k
        for n in ("one_finite_last", "one_finite_first"):
            assert p[names.index(n)] == 1.0, (k, n)


def test_more_columns_than_the_kernel_takes_are_refused(pkg, built):
    with pytest.raises(pkg.OcrError, match="8192"):
        pkg.selftest_softmax_argmax(np.zeros((1, 8193), np.float32))
    x = np.zeros((5, 8192), np.float32)
    x[:, 8191] = 1.0
    x[2, 17] = 1.0
    out = pkg.selftest_softmax_argmax(x)
    amax, pmax = R.softmax32(x)
    assert list(out["amax"][0]) == [8191, 8191, 17, 8191, 8191] and _eq(out["pmax"][0], pmax)


# ------------------------------------------------------------------------------------------------------------ collapse
@pytest.mark.parametrize("chars", [False, True])
@pytest.mark.parametrize("name", sorted(COLLAPSE))
def test_collapse_bit_for_bit(pkg, built, name, chars):
    c = COLLAPSE[name]
    want = R.ctc(c["amax"], c["pmax"], c["lines"], c["max_len"], chars=chars)
    forms = [dict(lines=c["lines"])] + ([dict(T=c["T"])] if c["T"] else [])     # a uniform batch also goes through the ragged launch
    for form in forms:
        got = pkg.selftest_ctc(c["amax"], c["pmax"], c["max_len"], chars=chars, **form)
        assert set(got) == set(want)
        for k, (v, g) in got.items():
            _clean(g)
            assert _eq(v, want[k]), (name, k, form.keys())   # (the reference holds the fill past the stored count)


# ------------------------------------------------------------------------------------------------------------ chunking
def test_launches_split_at_65535_lines(pkg, built):
    n, C, k, T, ml = 65535 + 3, 8, 3, 3, 3
    rs = np.random.RandomState(7)
    near = np.r_[0:4, 65530:n]
    # the top-k launch, max_len 1 (one row per line) ...
    rows = rs.randn(n, C).astype(np.float32)
    p0 = (rs.rand(n) * 0.9 + 0.05).astype(np.float32)
    ids, probs = pkg.selftest_topk(rows, p0, k)
    want = np.argsort(-rows.astype(np.float64), axis=1, kind="stable")[:, :k]
    assert np.array_equal(ids, want) and _eq(probs[:, 0], p0)
    # ... and max_len 3 with lens 0, 1, 3 across the split: six pointers move with the chunk
    rows = rs.randn(n * T, C).astype(np.float32)
    lens = (np.arange(n) % 3 == 1) * 1 + (np.arange(n) % 3 == 2) * 3
    steps = np.tile(rs.permutation(T).astype(np.int32), (n, 1))
    steps[::2] = steps[::2, ::-1]
    p0 = (rs.rand(n, ml) * 0.9 + 0.05).astype(np.float32)
    (ids, gi), (probs, gp) = pkg.selftest_topk_lines(rows, T, lens, steps, p0, k)
    _clean(gi, gp)
    live = np.arange(ml)[None, :] < lens[:, None]
    src = rows.reshape(n, T, C)[np.arange(n)[:, None], steps]                  # [n, ml, C]: the row behind character j
    want = np.argsort(-src.astype(np.float64), axis=2, kind="stable")[:, :, :k]
    assert np.array_equal(ids[live], want[live]) and _eq(probs[live][:, 0], p0[live])
    assert (ids[~live].view(np.uint8) == R.FILL).all() and (probs[~live].view(np.uint8) == R.FILL).all()
    assert {int(v) for v in lens[near]} == {0, 1, 3}
    # the collapse, one step per line
    amax = rs.choice([0, 3, 5], n).astype(np.int32)
    pmax = (rs.rand(n) * 0.9 + 0.05).astype(np.float32)
    for chars in (False, True):
        got = pkg.selftest_ctc(amax, pmax, 2, T=1, chars=chars)
        keep = amax > 0
        assert np.array_equal(got["lens"][0], keep.astype(np.int32)) and np.array_equal(got["ids"][0][keep, 0], amax[keep])
        assert _eq(got["scores"][0], np.where(keep, pmax, np.float32(0)).astype(np.float32))
        assert (got["ids"][0][~keep].view(np.uint8) == R.FILL).all() and (np.ascontiguousarray(got["ids"][0][:, 1]).view(np.uint8) == R.FILL).all()
        for v, g in got.values():
            _clean(g)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_next_call_working(pkg, built):
    x, want = HEADS["ties_C129"]
    m, s, idx = R.srv_partials(x)
    part = R.pack_partials(m, s, idx)
    gm, gs, gidx = R.group_partials(x)
    c = COLLAPSE["n65_T40"]
    L = pkg.lib()
    bad = [
        lambda: pkg.selftest_softmax_argmax(np.zeros((0, 4), np.float32)),
        lambda: pkg.selftest_softmax_argmax(np.zeros((4, 0), np.float32)),
        lambda: pkg.selftest_softmax_argmax(np.zeros((2, 9000), np.float32)),
        lambda: pkg.selftest_head_combine(gm[:0], gs[:0], gidx[:0]),
        lambda: pkg.selftest_srv_argmax(x, ncols=x.shape[1] + 1),                      # ld < C
        lambda: pkg.selftest_srv_argmax(x, one_pass=True),                             # ld = 129: not a multiple of 4
        lambda: pkg.selftest_srv_argmax(_padded(x, 130), ncols=129, one_pass=True),
        lambda: pkg.selftest_srv_argmax(x[:0]),
        lambda: pkg.selftest_ctc_reduce(part, step=0),
        lambda: pkg.selftest_ctc_reduce(part, step=part.shape[1] + 1),
        lambda: pkg.selftest_ctc_reduce(part[:0]),
        lambda: pkg.selftest_ctc(c["amax"], c["pmax"], 0, T=40),
        lambda: pkg.selftest_ctc(c["amax"], c["pmax"], 6, T=0),
        lambda: pkg.selftest_ctc(c["amax"], c["pmax"], 6, T=41),                       # nlines * T is not the step count
        lambda: pkg.selftest_ctc(c["amax"], c["pmax"], 6, lines=[(0, 40), (len(c["amax"]) - 39, 40)]),
        lambda: pkg.selftest_ctc(c["amax"], c["pmax"], 6, lines=[(-1, 2)]),
        lambda: pkg.selftest_ctc(c["amax"], c["pmax"], 6, lines=[(0, -1)]),
        lambda: pkg.selftest_ctc(c["amax"], c["pmax"], 6, lines=np.zeros((0, 2), np.int32)),
        lambda: pkg.selftest_topk_lines(np.zeros((2, 8), np.float32), 2, [1], [[2]], [[0.5]], 1),     # a step outside the line
        lambda: pkg.selftest_topk_lines(np.zeros((2, 8), np.float32), 2, [-1], [[0]], [[0.5]], 1),
        lambda: pkg.selftest_topk_lines(np.zeros((2, 8), np.float32), 2, [1], [[0]], [[0.5]], 9),
        lambda: L.ocr_selftest_softmax_argmax(None, 1, 1, None, None, None),
        lambda: L.ocr_selftest_head_combine(None, None, None, 1, 1, None, None),
        lambda: L.ocr_selftest_srv_argmax(None, 1, 1, 1, 0, None, None),
        lambda: L.ocr_selftest_ctc_reduce(None, 1, 1, 1, None, None),
        lambda: L.ocr_selftest_ctc(None, None, 1, 1, 1, None, 1, 0, None, None, None, None, None, None),
        lambda: L.ocr_selftest_topk_lines(None, 1, 1, 1, 1, None, None, None, 1, 1, None, None),
    ]
    amax, pmax, _ = _ref32("ties_C129")
    want_ctc = R.ctc(c["amax"], c["pmax"], c["lines"], c["max_len"], chars=True)
    for i, call in enumerate(bad):
        try:
            rc = call()
        except pkg.OcrError as e:
            assert getattr(e, "code", None) == -1 or "error -1" in str(e), (i, str(e))      # OCR_ERR_ARG
            assert str(e).rstrip().split(":")[-1].strip(), "a refusal carries a message"
        else:
            assert rc == -1 and L.ocr_last_error(), i                                        # the raw null-pointer calls
        out = pkg.selftest_softmax_argmax(x)
        assert np.array_equal(out["amax"][0], want) and _eq(out["pmax"][0], pmax), i
    (a, _), _ = pkg.selftest_ctc_reduce(part)
    (a2, _), _ = pkg.selftest_srv_argmax(_padded(x, 132), ncols=129, one_pass=True)
    (a3, _), (p3, _) = pkg.selftest_head_combine(gm, gs, gidx)
    assert np.array_equal(a, want) and np.array_equal(a2, want) and np.array_equal(a3, want) and _eq(p3, pmax)
    got = pkg.selftest_ctc(c["amax"], c["pmax"], c["max_len"], T=40, chars=True)
    assert all(_eq(got[k][0], want_ctc[k]) for k in want_ctc)


# ------------------------------------------------------------------------------------------------------------ teeth
@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_the_device_disagrees_with_every_mutated_reference(pkg, built, mut):
    fam, name = tc.KILLED_BY[mut]
    if fam == "head":
        x, _ = HEADS[name]
        bad = R.softmax32(x, mut=(mut,))[0]
        m, s, idx = R.srv_partials(x)
        got = [pkg.selftest_softmax_argmax(x)["amax"][0], pkg.selftest_head_combine(*R.group_partials(x))[0][0],
               pkg.selftest_srv_argmax(x)[0][0], pkg.selftest_srv_argmax(_padded(x, (x.shape[1] + 3) & ~3), ncols=x.shape[1], one_pass=True)[0][0]]
        for a in got:
            assert not np.array_equal(a, bad)
        m2, s2, idx2 = R.srv_partials(x, mut=(mut,))
        assert not np.array_equal(pkg.selftest_ctc_reduce(R.pack_partials(m, s, idx))[0][0], R.srv_fold(m2, s2, idx2, mut=(mut,))[0])
        return
    c = COLLAPSE[name]
    bad = R.ctc(c["amax"], c["pmax"], c["lines"], c["max_len"], chars=True, mut=(mut,))
    key = {"collapse_across_blank": "ids", "score_over_stored": "scores", "open_last_run": "nsteps"}[mut]
    for form in (dict(T=c["T"]), dict(lines=c["lines"])):
        for chars in ((True,) if key == "nsteps" else (False, True)):
            got = pkg.selftest_ctc(c["amax"], c["pmax"], c["max_len"], chars=chars, **form)
            assert not _eq(got[key][0], bad[key])
