"""tools/tail_ref.py, the plain restatement of the recognizer's tail (row softmax + arg max, the server fold, the greedy CTC
collapse), against the oracle library on every case tests/test_gpu_rec_tail.py runs on the device: the f32 softmax bit for bit,
the collapse id for id and score bit for bit.  Plus: every designed branch occurs in the case tables, every mutation changes the
reference on the case named for it, and the server bound of srv_ref.ctc_tail holds for an f32 evaluation done on the CPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tail_cases as tc  # noqa: E402

import tail_ref as R  # noqa: E402  (tools/ is on the path: conftest.py)

HEADS = tc.head_cases()
COLLAPSE = tc.collapse_cases()


def _eq(a, b):
    a, b = R.bits(a), R.bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


@pytest.fixture(scope="module")
def O(built):
    import oracle
    return oracle


def _oracle_softmax(O, x):
    """the oracle library's softmax op on the rows of x: a plan `linear -> softmax` on a zero input, the row as the linear's bias
    (0 * 0 + .. + 0, then + b: the logits ARE the bias, bit for bit)"""
    rows, Cn = x.shape
    plan = ("plan tail ntensors=3\nlinear i=0 o=1 cin=3 cout=%d w=w ep=bias:b\nsoftmax i=1 o=2 c=%d\noutput i=2\n" % (Cn, Cn))
    out = np.empty_like(x)
    net = O.OracleNet("tail", weights={"w": np.zeros((3, Cn), np.float32), "b": x[0]}, plan=plan)
    L = O.lib()
    for r in range(rows):
        b = np.ascontiguousarray(x[r])
        L.oracle_net_set_param(net.h, b"b", b.ctypes.data, 1, (C.c_int * 1)(Cn))
        out[r] = net.run(np.zeros((1, 1, 1, 3), np.float32)).reshape(Cn)
        assert _eq(net.tensor(1).reshape(Cn), b)
    return out


def test_expf_equals_the_oracle(O):
    L = O.lib()
    rs = np.random.RandomState(5)
    x = np.concatenate([rs.uniform(-90, 90, 20000), rs.uniform(-1, 1, 5000), [0.0, -0.0, -87.0, 88.0, -200.0, 200.0, np.nan, -np.inf,
                                                                              np.inf]]).astype(np.float32)
    want = np.array([L.oracle_expf(C.c_float(float(v))) for v in x], np.float32)
    assert _eq(R.expf(x), want)


@pytest.mark.parametrize("name", sorted(HEADS))
def test_softmax_and_arg_max_equal_the_oracle(O, name):
    x, want = HEADS[name]
    x = x[:48]                                    # (the row-count cases repeat their rows)
    amax, pmax, probs = R.softmax32(x, probs=True)
    assert np.array_equal(amax, want[:48])        # the designed first maximum
    assert np.array_equal(amax, x.argmax(1))      # the oracle pipeline's arg max of the logits (oracle/pipeline.py)
    q = _oracle_softmax(O, x)
    assert _eq(probs, q)
    assert _eq(pmax, q[np.arange(len(x)), amax])


@pytest.mark.parametrize("Cn", tc.HEAD_C)
def test_random_rows_equal_the_oracle_and_float64(O, Cn):
    x = tc.random_rows(Cn)
    amax, pmax, probs = R.softmax32(x, probs=True)
    q = _oracle_softmax(O, x)
    assert _eq(probs, q) and np.array_equal(amax, x.argmax(1)) and _eq(pmax, q[np.arange(len(x)), amax])
    i64, p64 = R.softmax64(x)
    import net_ref
    y, bound = net_ref.Ref.softmax(None, x.astype(np.float64))
    assert np.array_equal(i64, amax)
    assert (np.abs(pmax - p64) <= bound[np.arange(len(x)), amax]).all()
    # the server fold of the same rows is the same number
    m, s, idx = R.srv_partials(x)
    a2, p2 = R.srv_fold(m, s, idx)
    assert np.array_equal(a2, amax) and np.allclose(p2, p64, rtol=1e-12, atol=0)


@pytest.mark.parametrize("Cn", tc.DEGENERATE_C)
def test_rows_without_a_maximum(O, Cn):
    """the contract of DESIGN.md section 4 on the degenerate rows: amax inside [0, C), never a NaN's column unless none is left;
    pmax never inf; where the oracle's own values are finite they are the reference's, bit for bit"""
    names, x = tc.degenerate_rows(Cn)
    amax, pmax, probs = R.softmax32(x, probs=True)
    q = _oracle_softmax(O, x)
    assert _eq(probs, q)                          # the full softmax is the oracle's on every row, inf and all
    assert ((0 <= amax) & (amax < Cn)).all() and not np.isinf(pmax).any() and not np.isnan(pmax).any()
    want = dict(all_neg_inf=0, one_finite_last=Cn - 1, one_finite_first=0, pos_inf=Cn // 2, two_pos_inf=1, all_nan=0, nan_and_neg_inf=0,
                nan_first=Cn - 1, nan_last=0, nan_before_max=Cn // 2)
    for i, n in enumerate(names):
        if n in want:
            assert amax[i] == want[n], n
        own = q[i, amax[i]]
        if n in ("all_neg_inf", "all_nan", "nan_and_neg_inf"):
            assert pmax[i] == 0
        elif np.isinf(own):
            assert pmax[i] == 0, n
        else:
            assert _eq(pmax[i:i + 1], np.array([own], np.float32)), n
        if not np.isnan(x[i]).any():
            assert amax[i] == x[i].argmax(), n     # without NaN this is the oracle pipeline's np.argmax
    m, s, idx = R.srv_partials(x)
    a2, p2 = R.srv_fold(m, s, idx)
    assert np.array_equal(a2, amax) and not np.isinf(p2).any()


def test_fused_and_unfused_forms_are_one_function():
    """group_partials + combine IS softmax32; the partials of a row say where its maximum sits"""
    for name in ("ties_C257", "ties_C6625", "rows_5"):
        x, want = HEADS[name]
        m, s, idx = R.group_partials(x)
        a, p, _, _ = R.combine(m, s, idx)
        a2, p2 = R.softmax32(x)
        assert np.array_equal(a, a2) and _eq(p, p2) and np.array_equal(a, want)


@pytest.mark.parametrize("name", sorted(COLLAPSE))
def test_collapse_equals_the_oracle(O, name):
    c = COLLAPSE[name]
    big = 4096                                     # no cut: the oracle's whole decode
    got = R.ctc(c["amax"], c["pmax"], c["lines"], big, chars=True)
    cut = R.ctc(c["amax"], c["pmax"], c["lines"], c["max_len"], chars=True)
    plain = R.ctc(c["amax"], c["pmax"], c["lines"], c["max_len"])
    for li, (s0, T) in enumerate(c["lines"]):
        am, pm = c["amax"][s0:s0 + T], c["pmax"][s0:s0 + T]
        ids, score = O.ctc_decode(am, pm)
        n = got["lens"][li]
        if ids is None:                            # the reference `continue`s on a NaN score: an empty line (0 / 0)
            assert n == 0 and got["scores"][li] == 0
        else:
            assert n == len(ids) and np.array_equal(got["ids"][li, :n], ids)
            assert _eq(got["scores"][li:li + 1], np.array([score], np.float32))
        # the cut keeps the count and the score and the first max_len of everything
        k = min(n, c["max_len"])
        assert cut["lens"][li] == n and _eq(cut["scores"][li:li + 1], got["scores"][li:li + 1])
        for key in ("ids", "steps", "nsteps", "probs"):
            assert _eq(cut[key][li, :k], got[key][li, :k])
            assert (cut[key][li, k:].view(np.uint8) == R.FILL).all()
        assert _eq(plain["ids"][li], cut["ids"][li])
        # per-character evidence: the step holds the id, probs is pmax there, the run is a run of that id
        for j in range(k):
            st, rn = cut["steps"][li, j], cut["nsteps"][li, j]
            assert (am[st:st + rn] == cut["ids"][li, j]).all() and (st + rn == T or am[st + rn] != cut["ids"][li, j])
            assert cut["probs"][li, j].tobytes() == pm[st].tobytes()


def test_every_designed_branch_occurs():
    """asserted on the tables, not assumed"""
    # arg max: where the maximum sits, per C
    for Cn in tc.HEAD_C:
        names, x, want = tc.tie_rows(Cn)
        at = dict(zip(names, want))
        assert at["first"] == 0 and at["last"] == Cn - 1 and at["all_equal"] == 0 and (x[names.index("all_equal")] == x[0, 0] * 0 + 3).all()
        if Cn > 128:
            i = names.index("tie_127_128")
            assert at["group_end"] == 127 and at["group_start"] == 128 and x[i, 127] == x[i, 128] == x[i].max() and at["tie_127_128"] == 127
            i = names.index("tie_two_groups")
            hit = np.nonzero(x[i] == x[i].max())[0]
            assert len(hit) == 2 and hit[0] // 128 != hit[1] // 128 and at["tie_two_groups"] == hit[0]
        if Cn > 64:
            i = names.index("tie_63_64")
            assert at["slot_end"] == 63 and at["slot_start"] == 64 and x[i, 63] == x[i, 64] == x[i].max()
        if Cn > 194:
            i = names.index("tie_two_slots")
            hit = np.nonzero(x[i] == x[i].max())[0]
            assert len(hit) == 2 and hit[0] // 64 != hit[1] // 64
        for i in range(len(names)):               # every row: the designed columns alone hold the maximum
            assert (x[i] == x[i].max()).sum() == (Cn if names[i] == "all_equal" else 2 if names[i].startswith("tie") else 1), (Cn, names[i])
    assert set(tc.HEAD_C) == {2, 127, 128, 129, 255, 257, 6625}
    assert {len(HEADS["rows_%d" % r][0]) for r in tc.HEAD_ROWS} == {1, 3, 4, 5, 255, 256, 257}
    # collapse
    assert {(len(c["lines"]), c["T"]) for c in COLLAPSE.values() if c["T"]} >= {(n, T) for n in (1, 63, 64, 65, 130) for T in (1, 2, 40)}
    rag = COLLAPSE["ragged_66"]
    assert {T for _, T in rag["lines"]} == {1, 2, 40, 83}
    firsts = [s for s, _ in rag["lines"]]
    assert firsts != sorted(firsts) and min(firsts) > 0
    owned = np.zeros(len(rag["amax"]), int)
    for s0, T in rag["lines"]:
        owned[s0:s0 + T] += 1
    assert owned.max() == 1 and (owned == 0).any()
    for name in ("n65_T40", "ragged_66"):
        c = COLLAPSE[name]
        ref = R.ctc(c["amax"], c["pmax"], c["lines"], c["max_len"], chars=True)
        d, ml = c["designed"], c["max_len"]
        line = lambda k: c["amax"][c["lines"][d[k]][0]:][:40]
        assert ref["lens"][d["all_blank"]] == 0 and ref["scores"][d["all_blank"]] == 0
        assert ref["lens"][d["one_class"]] == 1 and ref["nsteps"][d["one_class"], 0] == 40
        assert ref["lens"][d["a_a_blank_a"]] == 2 and list(line("a_a_blank_a")[:4]) == [tc.A, tc.A, 0, tc.A]
        assert ref["lens"][d["a_b_a"]] == 3
        assert ref["steps"][d["char_at_0"], 0] == 0 and ref["lens"][d["char_at_0"]] == 1
        assert ref["steps"][d["char_at_last"], 0] == 39 and ref["lens"][d["char_at_last"]] == 1
        assert [ref["lens"][d["count_%d" % k]] for k in (ml - 1, ml, ml + 1, 3 * ml)] == [ml - 1, ml, ml + 1, 3 * ml]
        # the run of the last stored character: closed at the line's end, by a blank, and by a cut character (with and without repeats after it)
        assert ref["lens"][d["cut_then_runs"]] == ml + 1 and ref["nsteps"][d["cut_then_runs"], ml - 1] == 4
        assert ref["lens"][d["cut_no_repeat"]] == ml + 1 and ref["nsteps"][d["cut_no_repeat"], ml - 1] == 2
        assert ref["nsteps"][d["count_%d" % ml], ml - 1] == 1 + (ml - 1) % 3
    assert COLLAPSE["n65_T40_maxlen1"]["max_len"] == 1
    # degenerate rows
    for Cn in tc.DEGENERATE_C:
        names, x = tc.degenerate_rows(Cn)
        assert {"all_neg_inf", "one_finite_last", "pos_inf", "all_nan", "nan_first", "nan_before_max"} <= set(names)
        assert np.isneginf(x[names.index("all_neg_inf")]).all() and np.isnan(x[names.index("all_nan")]).all()
        assert np.isposinf(x[names.index("pos_inf")]).sum() == 1 and np.isnan(x[names.index("nan_first")]).sum() == 1


def _mutated(mut):
    fam, name = tc.KILLED_BY[mut]
    if fam == "head":
        x, _ = HEADS[name]
        m, s, idx = R.srv_partials(x)
        m2, s2, idx2 = R.srv_partials(x, mut=(mut,))
        return (R.softmax32(x), R.softmax32(x, mut=(mut,))), (R.srv_fold(m, s, idx), R.srv_fold(m2, s2, idx2, mut=(mut,)))
    c = COLLAPSE[name]
    return ((R.ctc(c["amax"], c["pmax"], c["lines"], c["max_len"], chars=True),
             R.ctc(c["amax"], c["pmax"], c["lines"], c["max_len"], chars=True, mut=(mut,))),)


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_every_mutation_is_killed_by_its_named_case(mut):
    assert set(tc.KILLED_BY) == set(R.MUTATIONS) and not R.EQUIVALENT
    for good, bad in _mutated(mut):
        if isinstance(good, dict):
            key = {"collapse_across_blank": "ids", "score_over_stored": "scores", "open_last_run": "nsteps"}[mut]
            assert not _eq(good[key], bad[key])
            if mut == "collapse_across_blank":
                assert not _eq(good["lens"], bad["lens"])
        else:
            assert not np.array_equal(good[0], bad[0])       # the arg max itself moves, in the mobile and in the server form


def test_server_bounds_hold_for_an_f32_evaluation():
    """srv_ref.ctc_tail / ctc_fold are derived for f32 evaluations with a 1-ulp exp2: a numpy f32 evaluation in the kernels' orders
    (np.exp2 rounded to f32 is within 1 ulp) must sit inside them - so the bound is not vacuous on the CPU either"""
    import srv_ref
    for Cn in (129, 6625):
        x = tc.random_rows(Cn)
        f = np.float32
        L2E = f(1.44269504088896341)
        # one-pass form: per lane an online softmax over its 4-column pieces, then the lanes folded
        amax, p, bound = srv_ref.ctc_tail(x, "one_pass")
        got = np.empty(len(x), f)
        for r in range(len(x)):
            ms, ss = [], []
            for lane in range(64):
                m, s = f(-np.inf), f(0)
                for c in range(4 * lane, Cn, 256):
                    v = x[r, c:min(c + 4, Cn)]
                    lm = max(m, v.max())
                    acc = f(0) if m == -np.inf else f(s * np.exp2(f(f(m - lm) * L2E)).astype(f))
                    for e in v:
                        acc = f(acc + np.exp2(f(f(e - lm) * L2E)).astype(f))
                    m, s = lm, acc
                ms.append(m); ss.append(s)
            M = max(ms)
            tot = f(0)
            for m, s in zip(ms, ss):
                if m > -np.inf:
                    tot = f(tot + f(s * np.exp2(f(f(m - M) * L2E)).astype(f)))
            got[r] = f(1) / tot
        assert (np.abs(got.astype(np.float64) - p) <= bound).all()
        assert np.array_equal(amax, x.argmax(1))
        m, s, idx = R.srv_partials(x)
        pf, bf = srv_ref.ctc_fold(m, s)
        assert np.allclose(pf, p, rtol=1e-12, atol=0) and (bf > 0).all()


def test_server_int_head_designs_and_random_margin():
    """the exact-logit head of the fused server launch: every design's columns - and only they - hold the row's maximum, all partial
    sums stay far below 2^24; and the random rows of the margin-guarded comparison leave out at most 1 % on the reference alone"""
    import srv_ref
    W, b = tc.srv_int_head()
    X, which = tc.srv_int_rows(280)
    assert set(which) == set(range(len(tc.SRV_DESIGNS))) and (np.abs(X) @ np.abs(W)).max() + 1 < 2 ** 24
    y = X.astype(np.float64) @ W + b
    for r in range(len(X)):
        name, cols = tc.SRV_DESIGNS[which[r]]
        hit = np.nonzero(y[r] == y[r].max())[0]
        if cols is None:
            assert hit[0] == 0 and len(hit) > 1000
        else:
            assert list(hit) == sorted(cols), (r, name)
    names = dict(tc.SRV_DESIGNS)
    assert names["tie_63_64"] == (63, 64) and names["last"] == (tc.SRV_C - 1,) and len({c // 128 for c in names["tie_two_tiles"]}) == 4
    A = tc.srv_random_rows(280)
    y = A.astype(np.float64) @ W + b
    top = np.sort(y, 1)[:, -2:]
    bound = srv_ref.linear_f32_bound(A.astype(np.float64), W.astype(np.float64), b, y).max(1)
    out = (top[:, 1] - top[:, 0]) <= 2 * bound
    assert out.mean() <= 0.01, out.mean()



def test_mobile_int_head_designs_and_random_margin():
    """the same for the mobile head (K = 120): designs, exactness, the steps formula behind MOB_SHAPES, and the margin share"""
    import srv_ref
    W, b = tc.mob_int_head()
    assert (np.abs(W).sum(0).max() + 1) * 2 < 2 ** 24
    for seed in range(12):                                   # (a single row still meets every design over the seeds)
        X, which = tc.mob_int_rows(257, seed)
        y = X.astype(np.float64) @ W + b
        for r in range(0, len(X), 1 if seed == 0 else 64):
            name, cols = tc.MOB_DESIGNS[which[r]]
            hit = np.nonzero(y[r] == y[r].max())[0]
            assert (hit[0] == 0 and len(hit) > 1000) if cols is None else list(hit) == sorted(cols), (r, name)
        assert np.abs(y - y.max(1, keepdims=True)).max() < 80       # far from ocr_expf's clamp
    d = dict(tc.MOB_DESIGNS)
    assert d["tie_half_waves"][0] >> 2 & 1 != d["tie_half_waves"][1] >> 2 & 1 and d["tie_tiles_31_32"][0] // 32 != d["tie_tiles_31_32"][1] // 32
    assert len({c // 128 for c in d["tie_two_groups"]}) == 4 and d["last_group"] == (51 * 128 - 1, 51 * 128)
    for rows, (lines, w) in tc.MOB_SHAPES.items():
        a = (w - 1) // 2 + 1
        assert lines * ((((a - 1) // 2 + 1)) // 2) == rows
    A = tc.mob_random_rows(256)
    y = A.astype(np.float64) @ W + b
    top = np.sort(y, 1)[:, -2:]
    bound = srv_ref.linear_f32_bound(A.astype(np.float64), W.astype(np.float64), b, y).max(1)
    assert ((top[:, 1] - top[:, 0]) <= 2 * bound).mean() <= 0.01

