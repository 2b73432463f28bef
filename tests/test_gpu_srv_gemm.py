"""The server GEMM family alone, on the synthetic plans of tests/srv_gemm_cases.py, under EVERY tile configuration of the library's
table (SrvNet.configs(), pinned per net with set_config - no child process, no environment knob):
  * f32 twin: every tensor of every plan and shape bit-identical to the oracle's run of the same plan text;
  * f16 build: which (configuration, op) pairs run is exactly what the case table predicts from the kernels' stated rules; a strict
    refusal names the op, the configuration and the dispatch's reason; every op that runs is within its per-element bound
    (srv_ref.check_tensors on the device's own inputs: the derivation tests/test_gpu_srv_ops.py uses) and bit-identical to the
    default binding's result - so to every other configuration's;
  * the production binding's fused launches (MLP, head tail, concat folded into the halo form), the CTC partials, hostile rows at
    tile edges, the seven srv_ref.GEMM_MUTATIONS rejected on device results, and refusals / bad arguments leaving the handle usable."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import srv_gemm_cases as G  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def _table():
    """the configuration table, from the library (no GPU needed to read it)"""
    from __graft_entry__ import load_package
    try:
        return load_package().SrvNet.configs()
    except Exception:  # (not built yet: collection must not fail - the tests themselves ask for `built`)
        return []


CFGS = _table()
CFG_IDS = [c[0] for c in CFGS] or [0]
NAME = {c[0]: c[1] for c in CFGS}


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return str(tmp_path_factory.mktemp("srv_gemm"))


def _net(pkg, work, P, text, precision="fp16"):
    import synth_weights
    key = ("file", text)
    if key not in _CACHE:
        path = os.path.join(work, "p%d.pdiparams" % len(_CACHE))
        synth_weights.write_params(path, P.weights(text))
        _CACHE[key] = path
    return pkg.SrvNet.from_plan(text, _CACHE[key], precision)


def _fetch_all(net, P, text):
    tids = [int(ln.rsplit("o=", 1)[1]) for ln in text.splitlines() if ln and ln[0] != "#" and not ln.startswith(("plan ", "output "))]
    t = {tid: net.fetch(tid).astype(np.float64) for tid in tids}
    t[0] = net.fetch(net.num_tensors()).astype(np.float64)
    return t


def _ref(text, P, half=True):
    import srv_ref
    key = ("ref", text, half)
    if key not in _CACHE:
        _CACHE[key] = srv_ref.Ref(text, P.weights(text), half=half)
    return _CACHE[key]


def _base(pkg, work, name, shape):
    """the f16 build's keep_all run under the default choice of configurations, once per (plan, shape): (P, text, tensors)"""
    key = ("base", name, shape)
    if key not in _CACHE:
        P = G.plan(name, shape)
        text = P.text()
        net = _net(pkg, work, P, text)
        net.forward(G.x_of(name, shape), keep_all=True)
        _CACHE[key] = (P, text, _fetch_all(net, P, text))
        net.close()
    return _CACHE[key]


def _oracle(name, shape):
    import oracle as O
    key = ("oracle", name, shape)
    if key not in _CACHE:
        P = G.plan(name, shape)
        text = P.text()
        net = O.OracleNet("synthetic", weights=P.weights(text), plan=text)
        net.run(G.x_of(name, shape))
        _CACHE[key] = (P, text, {op["o"]: net.tensor(op["o"]) for op in P.ops if op["live"]})
    return _CACHE[key]


def _report(title, worst):
    print("%s: worst err/bound  %s" % (title, "  ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


PLAN_SHAPES = [(n, s) for n in "ABC" for s in G.SHAPES[n]] + [("T%d" % c[1], s) for c in G.CTC_HEADS for s in G.CTC_SHAPES]


@pytest.mark.parametrize("cid", CFG_IDS)
def test_f32_twin_equals_the_oracle_under_every_configuration(pkg, built, work, cid):
    """set_config(id, strict=False) on the f32 twin (an id whose twin does not take an op falls back): keep_all, every plan and
    shape, N > 1 included - every tensor bit-identical to OracleNet on the same plan text"""
    assert cid in NAME, "the library must be built before the tests are collected: the parameters are its configuration table"
    nets = {}
    for name, shape in PLAN_SHAPES:
        P, text, want = _oracle(name, shape)
        if text not in nets:
            nets[text] = _net(pkg, work, P, text, "fp32")
            nets[text].set_config(cid, strict=False)
        net = nets[text]
        net.forward(G.x_of(name, shape), keep_all=True)
        for tid, w in want.items():
            got = net.fetch(tid)
            assert got.shape == w.shape and np.array_equal(got, w), (NAME.get(cid), name, shape, tid)
    for net in nets.values():
        net.close()


@pytest.mark.parametrize("cid", CFG_IDS)
def test_f16_build_under_every_configuration(pkg, built, work, cid):
    """plans A and B, every shape, keep_all: the launches that carry this configuration's full name are exactly the predicted ones;
    each is within its bound on the device's own inputs, finite, and bit-identical to the default binding's result.  Strict: the
    accepted ops bind, every refused op is refused alone with its reason"""
    import srv_ref
    assert cid in NAME, "the library must be built before the tests are collected: the parameters are its configuration table"
    tile = G.tile_of(NAME[cid])
    tag = "[%s]" % NAME[cid]
    worst, ran, refused = {}, 0, 0
    for name in "AB":
        for shape in G.SHAPES[name]:
            P, text, base = _base(pkg, work, name, shape)
            net = _net(pkg, work, P, text)
            net.set_config(cid, strict=False)
            net.forward(G.x_of(name, shape), keep_all=True)
            by_out = {o: nm for nm, o, _ in net.launches()}
            t = _fetch_all(net, P, text)
            net.close()
            want = {op["o"] for op in G.gemm_ops(P) if G.predicted_refusal(tile, op) is None}
            got = {o for o, nm in by_out.items() if nm.endswith(tag)}
            assert got == want, (NAME[cid], name, shape, sorted(got ^ want))
            assert all(by_out[op["o"]].endswith("]") for op in G.gemm_ops(P))   # (the others fell back to another configuration)
            ran += len(got)
            refused += len(G.gemm_ops(P)) - len(got)
            ref = _ref(text, P)
            res = srv_ref.check_tensors(ref, t)
            for k, (kind, r) in res.items():
                o = srv_ref.gi(ref.ops[k], "o")
                assert r <= 1.0, (NAME[cid], name, shape, ref.ops[k]["kv"], r)
                if o in got:
                    worst[kind] = max(worst.get(kind, 0.0), r)
            for tid, b in base.items():
                assert np.array_equal(t[tid], b), (NAME[cid], name, shape, tid)
    _report("fp16 cfg %d %s (%d launches on it, %d fell back)" % (cid, NAME[cid], ran, refused), worst)
    # ---- strict
    for name, shape in (("A", G.SHAPES["A"][-1]), ("B", G.SHAPES["B"][-1])):
        P, full, base = _base(pkg, work, name, shape)
        x = G.x_of(name, shape)
        if tile["form"] == "halo":   # (the producers are 1x1 convs: the first of them is refused)
            net = _net(pkg, work, P, full)
            net.set_config(cid, strict=True)
            with pytest.raises(pkg.OcrError, match=r"op 0 .*%s refused: %s" % (NAME[cid], G.REASON_HALO)) as e:
                net.forward(x, keep_all=True)
            assert e.value.code == -1 and net.launches() == []
            net.set_config(-1)
            net.forward(x, keep_all=True)
            assert all(np.array_equal(net.fetch(tid).astype(np.float64), b) for tid, b in base.items() if tid)
            net.close()
            continue
        no = [op for op in P.tests() if G.predicted_refusal(tile, op) is not None]
        sub = P.text(only=G.accepted_labels(P, tile), with_out=not any(op["role"] == "out" for op in no))
        net = _net(pkg, work, P, sub)
        net.set_config(cid, strict=True)
        net.forward(x, keep_all=True)
        for nm, o, _ in net.launches():
            if "[" in nm:
                assert nm.endswith(tag), nm
                assert np.array_equal(net.fetch(o).astype(np.float64), base[o]), nm
        net.close()
        for op in no:
            mini = P.text(only=[op["label"]], with_out=op["role"] == "out")
            net = _net(pkg, work, P, mini)
            net.set_config(cid, strict=True)
            with pytest.raises(pkg.OcrError, match=r"op \d+ .*tile configuration %s refused: %s" % (NAME[cid], G.REASON_BIG)) as e:
                net.forward(x, keep_all=True)
            assert e.value.code == -1 and net.launches() == [], op["label"]
            net.set_config(-1)            # the handle stays usable: the default run's bits
            net.forward(x, keep_all=True)
            assert np.array_equal(net.fetch(op["o"]).astype(np.float64), base[op["o"]]), op["label"]
            net.close()


def _upload_random(net, tid, seed):
    import srv_ref
    shp = net.fetch(tid).shape
    u = srv_ref.f16(np.random.RandomState(seed).randn(*shp))
    net.upload(tid, u)
    return u


def test_fused_launches_of_the_production_binding(pkg, built, work):
    """keep_all=False on plans B and C: the fused MLP at every token count (C = 192, 256; C = 64 stays two launches), the head tail,
    and the concat of 1 - 4 sources folded into the halo form, each run alone on uploaded inputs against the reference of the ops
    it replaces; a concat source read with its neighbour's shift is rejected on the device's result"""
    import srv_ref
    from test_srv_gemm_cases import mutated_ratio  # noqa: F401
    worst, seen, mut_worst = {}, set(), 0.0
    for name in "BC":
        for shape in G.SHAPES[name]:
            P = G.plan(name, shape)
            text = P.text()
            ref = _ref(text, P)
            net = _net(pkg, work, P, text)
            net.forward(G.x_of(name, shape), keep_all=False)
            ls = net.launches()
            names = [nm for nm, _, _ in ls]
            if name == "C":
                assert sum(".mlp_192_768_192@" in n for n in names) == 1 and sum(".mlp_256_1024_256@" in n for n in names) == 1, names
                assert not any(".mlp_64" in n for n in names) and sum("linear1x1_64_256_" in n for n in names) == 1 and sum("linear1x1_256_64_" in n for n in names) == 1, names
            else:
                depths = [d for d in (1, 2, 3, 4) if any(op["label"] == "cat%d_c3" % d and op["live"] for op in P.ops)]
                assert sum(".head_tail_64_64_1@" in n for n in names) == 1 and sum("_cat[halo16x16x64]" in n for n in names) == len(depths), names
                assert not any(".concat_" in n or ".deconv" in n for n in names), names
            for i, (nm, out, ins) in enumerate(ls):
                if not (".mlp_" in nm or ".head_tail_" in nm or "_cat[" in nm):
                    continue
                oi = int(nm.split(".")[0])
                op = ref.ops[oi]
                u = {tid: _upload_random(net, tid, 1000 * i + tid) for tid in ins}
                net.run_launches(i, 1)
                got = net.fetch(out).astype(np.float64)
                for tid in ins:
                    assert np.array_equal(net.fetch(tid).astype(np.float64), u[tid]), (nm, tid)
                if ".mlp_" in nm:
                    y, b = ref.mlp(op, ref.ops[oi + 1], u[ins[0]])
                    k = "mlp_%d" % op["W"].shape[0]
                elif ".head_tail_" in nm:
                    y, b = ref.head_tail(op, ref.ops[oi + 1], u[ins[0]])
                    k = "head_tail"
                else:
                    cat = ref.ops[oi - 1]
                    tt = dict(u)
                    tt[srv_ref.gi(op, "i")] = ref.op(cat, u)[0]
                    y, b = ref.op(op, tt)
                    k = "conv3x3_cat%d" % len(ins)
                    if len(ins) > 1:
                        tm = dict(u)
                        tm[srv_ref.gi(op, "i")] = ref.op(cat, u, mut={"concat_next_shift": True})[0]
                        ym, bm = ref.op(op, tm)
                        mut_worst = max(mut_worst, srv_ref.ratio(got, ym, bm))
                r = srv_ref.ratio(got, y, b)
                assert r <= 1.0, (nm, shape, r)
                worst[k] = max(worst.get(k, 0.0), r)
                seen.add((k, shape))
            net.close()
    _report("fused launches", worst)
    assert {k for k, _ in seen} == {"mlp_192", "mlp_256", "head_tail", "conv3x3_cat1", "conv3x3_cat2", "conv3x3_cat3", "conv3x3_cat4"}, seen
    assert mut_worst > 1.0, mut_worst


def test_ctc_partials_under_every_configuration(pkg, built, work):
    """set_ctc(1) on output linears of 13, 64 and 200 columns, every configuration that takes linears (strict): the tail's arg max is
    the first maximum of the logits the same net gives with CTC off, its probability is inside srv_ref.ctc_head's bound, and both
    are bit-identical across configurations"""
    import srv_ref
    assert len(CFGS) >= 21, "the library must be built before the tests are collected"
    worst = 0.0
    for cin, cout in G.CTC_HEADS:
        P = G.plan("T%d" % cout)
        text = P.text()
        net = _net(pkg, work, P, text)
        for shape in G.CTC_SHAPES:
            x = G.x_of("T%d" % cout, shape)
            net.set_ctc(False)
            net.set_config(-1)
            y = net.forward(x).reshape(-1, cout).astype(np.float64)
            first = None
            for cid, cname, _ in CFGS:
                if G.tile_of(cname)["form"] == "halo":
                    continue
                net.set_ctc(True)
                net.set_config(cid, strict=True)
                net.forward(x)
                nm = net.launches()[-1][0]
                assert nm.endswith("_ctc[%s]" % cname), nm
                a, p, slots, step = net.ctc_tail()
                assert slots == (cout + 63) // 64 and step == 1
                assert np.array_equal(a, y.argmax(1)), (cname, shape)
                _, pr, pb = srv_ref.ctc_head(y, slots, step)
                worst = max(worst, float((np.abs(p - pr) / pb).max()))
                if first is None:
                    first = (a, p)
                assert np.array_equal(a, first[0]) and np.array_equal(p, first[1]), (cname, shape)
        net.close()
    print("CTC partials: worst err/bound %.3f" % worst)
    assert worst <= 1.0


def test_hostile_rows_at_the_tile_edges(pkg, built, work):
    """the 448 -> 13 and 96 -> 576 linears at M = 257 under every configuration: rows that drive outputs past +-65504 and rows of f16
    subnormals (test_gpu_srv_ops._gemm_hostile) in the last row of every full tile (63, 127, 191, 255) and in the only row of the
    partial one (256)"""
    import srv_ref
    from test_gpu_srv_ops import _gemm_hostile
    assert len(CFGS) >= 21, "the library must be built before the tests are collected"
    shape = (1, 257, 1)
    P = G.plan("A")
    text = P.text(only=["l448_13", "l96_576"], with_out=False)
    ref = _ref(text, P)
    net = _net(pkg, work, P, text)
    worst = {}
    for label in ("l448_13", "l96_576"):
        op = ref.by_out(P.tid(label))
        src = srv_ref.gi(op, "i")
        cin = op["W"].shape[0]
        H = _gemm_hostile(op, (6, cin), np.random.RandomState(5)).reshape(6, cin)   # rows 1, 4: clamp; 2, 5: subnormal
        for variant, rows in enumerate(({63: 1, 127: 2, 191: 4, 255: 5, 256: 1}, {63: 2, 127: 1, 191: 5, 255: 4, 256: 2})):
            X = srv_ref.f16(np.random.RandomState(6 + variant).randn(257, cin))
            for r, h in rows.items():
                X[r] = H[h]
            u = X.reshape(1, 257, 1, cin)
            y, b = ref.op(op, {src: u})
            assert np.abs(y).max() == 65504.0   # (the clamp rows do reach the clamp)
            first = None
            for cid, cname, _ in CFGS:
                if G.tile_of(cname)["form"] == "halo":
                    continue
                net.set_config(cid, strict=True)
                net.forward(G.x_of("A", shape), keep_all=True)
                i = next(k for k, (nm, o, _) in enumerate(net.launches()) if o == P.tid(label))
                assert net.launches()[i][0].endswith("[%s]" % cname)
                net.upload(src, u)
                net.run_launches(i, 1)
                got = net.fetch(P.tid(label)).astype(np.float64)
                r = srv_ref.ratio(got, y, b)
                assert r <= 1.0, (label, cname, variant, r)
                worst[label] = max(worst.get(label, 0.0), r)
                first = got if first is None else first
                assert np.array_equal(got, first), (label, cname, variant)
    net.close()
    _report("hostile rows at tile edges", worst)


def test_the_checker_rejects_the_gemm_mutations_on_device_results(pkg, built, work):
    """on the device's own tensors (the default binding's keep_all runs of plans A and B), every mutated reference is rejected
    somewhere: a last row computed from the row before it, the last column dropped, the last K tile left out, a padding tap read
    from the neighbouring row or image, deconv taps swapped, the addup residual one column to the right (the folded concat's
    mutation runs in test_fused_launches_of_the_production_binding too)"""
    import srv_ref
    from test_srv_gemm_cases import mutated_ratio
    worst = {m: 0.0 for m in srv_ref.GEMM_MUTATIONS}
    for name in "AB":
        for shape in G.SHAPES[name]:
            P, text, t = _base(pkg, work, name, shape)
            ref = _ref(text, P)
            for mut in srv_ref.GEMM_MUTATIONS:
                for op in srv_ref.gemm_mutation_sites(ref, mut):
                    worst[mut] = max(worst[mut], mutated_ratio(ref, op, t, mut))
    print("GEMM mutations on device results: err/bound " + "  ".join("%s %.3g" % kv for kv in worst.items()))
    assert min(worst.values()) > 1.0, worst


def test_bad_arguments_leave_nothing_behind(pkg, built, work):
    import synth_weights
    P = G.plan("A")
    text = P.text(only=["l64_64"])
    path = os.path.join(work, "bad.pdiparams")
    synth_weights.write_params(path, P.weights(text))
    with pytest.raises(pkg.OcrError, match="null argument") as e:
        pkg.SrvNet.from_plan(None, path)
    assert e.value.code == -1
    early = text.replace("linear i=%d " % P.tid("l64_64"), "linear i=%d " % (P.nt - 1))   # the follower's input: a tensor nothing has written
    with pytest.raises(pkg.OcrError, match="is read before it is written") as e:
        pkg.SrvNet.from_plan(early, path)
    assert e.value.code == -1
    missing = text.replace("w=l64_64.w", "w=nothing.w")
    with pytest.raises(pkg.OcrError, match="missing parameter nothing.w") as e:
        pkg.SrvNet.from_plan(missing, path)
    assert e.value.code == -2
    with pytest.raises(pkg.OcrError) as e:
        pkg.SrvNet.from_plan(text, os.path.join(work, "no_such.pdiparams"))
    assert e.value.code == -2
    net = pkg.SrvNet.from_plan(text, path)
    x = G.x_of("A", (1, 3, 21))
    want = net.forward(x, keep_all=True)
    before = net.launches()
    for bad in (len(NAME) + 50, max(NAME) + 1, 10, -2):
        with pytest.raises(pkg.OcrError, match="no such tile configuration") as e:
            net.set_config(bad)
        assert e.value.code == -1
    assert net.launches() == before and np.array_equal(net.forward(x, keep_all=True), want)
    net.close()
